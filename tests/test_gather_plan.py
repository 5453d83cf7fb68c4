"""The multi-GPU gather's planning on the CPU, as a program of its own.

tests/cpp/gather_plan_main.cpp includes eray_amd/csrc/gather_plan.hpp — the header comm.cpp and
its kernels plan with, which makes no HIP call — and checks every rank's schedule for 1..8, 63 and
64 ranks (each send meets one receive of its size, packs apart and inside the buffer, the roots'
frames, the headers' count and places) and the ranks' rectangle layouts (at most eight rectangles,
inside the rank's rows, covering the objects' rectangles, bytes = rows x row bytes) for block and
band splits, short last bands included.  No GPU and no library: build_host() compiles it with g++.
"""
from tests.accel_emul import run_built


def test_gather_planning_program():
    r = run_built("gather_plan_main", [], timeout=120)
    assert r.returncode == 0 and "gather_plan: 0 failed checks" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
