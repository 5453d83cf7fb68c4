"""The screen bins' sizing on the CPU, as a program of its own.

tests/cpp/bin_layout_main.cpp includes eray_amd/csrc/bin_layout.hpp — the header bins.hip's
allocation and launch chain, the setups and the kernels size the bins with, which makes no HIP
call — and sweeps camera sizes from 1 to 65536 pixels, every row phase, short and full row ranges,
one and three binned objects, one and sixteen cameras and two capacities against plain
restatements: every camera row and pixel column maps into the bin grid, every detail sub-block's
bin index lies below nbins, and the finaliser's grid covers the keys with no idle workgroup.  No GPU
and no library: build_host() compiles it with g++.
"""
from tests.accel_emul import run_built


def test_bin_layout_program():
    r = run_built("bin_layout_main", [], timeout=120)
    assert r.returncode == 0 and "0 failed checks" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert "bin_layout: 0 checks" not in r.stdout
