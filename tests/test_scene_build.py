"""What the scene upload decides before it touches the GPU, on the CPU, as a program of its own.

tests/cpp/scene_build_main.cpp includes eray_amd/csrc/scene_build.hpp and texel_prog.hpp — the
headers capi_scene.cpp's sync_scene builds the scene with (the texel graphs' check with its
messages, their expansion into the instruction trees, the descriptors, the raw arrays' layout) and
the kernels evaluate the trees with (texel_program), none of which makes a HIP call — and checks
them against plain restatements: 240 seeded random shader graphs of 2 to 8 nodes run as Graph::run
does, every node's whole image by the node formulas, against the compiled program of each of the
five outputs at every texel of the root image and at uv values that saturate and wrap, on f32 bit
patterns; the trees' sizes, rgb's shared inputs and the 32-node limit (31 compile, 63 are refused);
every rejecting branch of the graph check with its status and exact message; every field of the
descriptors of scenes of 0, 1, 3 and 17 objects around the 256-face boundary with textures, the
example material, graphs and 0..3 lights; which scenes reflect; and that the raw arrays' slices
tile the scene's array once and return the objects' arrays.  No GPU and no library: build_host()
compiles it with g++.
"""
from tests.accel_emul import run_built


def test_scene_build_program():
    r = run_built("scene_build_main", [], timeout=120)
    assert r.returncode == 0 and "0 failed checks" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert "scene_build: 0 checks" not in r.stdout
