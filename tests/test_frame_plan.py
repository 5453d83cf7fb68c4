"""The frame calls' planning on the CPU, as a program of its own.

tests/cpp/frame_plan_main.cpp includes eray_amd/csrc/frame_plan.hpp — the header capi_frames.cpp
decides with before it touches the GPU (the rows a call reaches, the render-parameter and ring
checks with their messages, the frames per launch, the ring slot of every launch, the split of a
call's frames into graph chunks, a remainder and plain launches, the ring beyond the Infinity
Cache), which makes no HIP call — and checks it against plain restatements: banded and contiguous
row ranges for camera heights 4..64, the image fit for sizes 1..20, every rejecting branch's status
and exact message, the ring's argument rules, the automatic frames per launch around 1920x1080 and
3840x2160, and, for 1..64 slots, every allowed frames-per-launch and 0..200, 255, 256 and 257
frames, that the plans' walks render every frame exactly once into its own slot without wrapping,
in the static ring's form and the camera paths'.  No GPU and no library: build_host() compiles it
with g++.
"""
from tests.accel_emul import run_built


def test_frame_plan_program():
    r = run_built("frame_plan_main", [], timeout=120)
    assert r.returncode == 0 and "0 failed checks" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert "frame_plan: 0 checks" not in r.stdout
