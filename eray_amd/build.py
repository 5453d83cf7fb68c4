"""Build recipe of the product library eray_amd/lib/liberay_hip.so (gfx950 only).

    python -m eray_amd.build [--jobs N] [--verbose]

Compiles the HIP kernels and the C-ABI layer with hipcc for gfx950 and links them into one
shared library next to this package, so it travels to the GPU box with the repository.
Floating-point flags are part of the contract: -ffp-contract=off keeps a*b+c unfused so the
kernels reproduce the reference's f32 results bit-for-bit; hipcc's defaults already give
correctly rounded f32 division/sqrt and keep f32 denormals.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
OBJ = os.path.join(PKG, "_obj")
LIB_DIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIB_DIR, "liberay_hip.so")

SOURCES = ["render.hip", "setup.hip", "trace.hip", "rays.hip", "bins.hip", "shaderlib.hip", "capi.cpp", "capi_scene.cpp",
           "capi_debug.cpp", "capi_setup.cpp", "capi_frames.cpp", "capi_rays.cpp", "comm.cpp", "gather_debug.cpp", "objload.cpp", "accel_build.cpp", "accel_check.cpp", "accel_dev.hip"]
ARCH = "gfx950"
CXXFLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
            f"--offload-arch={ARCH}", "-I" + os.path.join(ROOT, "include"),
            # the first 15 kernel-argument dwords arrive in SGPRs (frame_kernel's FrameHot + band word)
            "-mllvm", "-amdgpu-kernarg-preload-count=15"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the eray_amd HIP library cannot be built")


def _newer(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _headers() -> list[str]:
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h"))]
    hs.append(os.path.join(ROOT, "include", "eray_hip.h"))
    return hs


def build(jobs: int = 4, verbose: bool = False, force: bool = False) -> str:
    """Build the product library (the only build: no diagnostic variants of the kernels)."""
    obj_dir = OBJ
    lib_path = LIB
    extra: list[str] = []
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(LIB_DIR, exist_ok=True)
    cc = hipcc()
    headers = _headers()
    objs, cmds = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(obj_dir, src + ".o")
        objs.append(o)
        if force or not _newer(o, [s] + headers):
            lang = [] if src.endswith(".hip") else ["-x", "hip"]
            cmds.append([cc, *CXXFLAGS, *extra, *lang, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"compile failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        return r.stderr

    with cf.ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
        for warn in ex.map(run, cmds):
            if warn.strip() and verbose:
                print(warn, file=sys.stderr)
    if force or cmds or not _newer(lib_path, objs):
        # RCCL for the multi-GPU gather (comm.cpp); under PyTorch the loader reuses torch's copy
        # (same SONAME librccl.so.1), so one RCCL serves the process
        run([cc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", lib_path, *objs, "-L/opt/rocm/lib", "-lrccl",
             "-Wl,-rpath,/opt/rocm/lib"])
    return lib_path


HOST_SOURCES = ["image.cpp", "graph.cpp", "shaderlib.cpp", "engine.cpp"]
HOST_LIB = os.path.join(LIB_DIR, "liberay_host.so")
BIN_DIR = os.path.join(PKG, "bin")
ROCM_LIB = "/opt/rocm/lib"


# the CPU programs of the ray-query hierarchy (tests/cpp/accel_*_main.cpp over tests/cpp/accel_emul.hpp): f32 as the
# kernels compute it (no fused multiply-add); what all but accel_walk_main compile with, and what they depend on
# (with every header that tests/cpp/ holds: the programs' shared part)
ACCEL_WALK_FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-pthread"]
ACCEL_DEV_SOURCES = [os.path.join(CSRC, "accel_build.cpp"), os.path.join(CSRC, "accel_check.cpp")]
ACCEL_DEV_HEADERS = ["accel_build.hpp", "accel_walk.hpp", "accel_margin.hpp", "accel_layout.hpp", "accel_check.hpp"]
TESTS_CPP = os.path.join(ROOT, "tests", "cpp")
WALK_MAIN = os.path.join(TESTS_CPP, "accel_walk_main.cpp")
DEV_MAIN = os.path.join(TESTS_CPP, "accel_dev_main.cpp")
REFIT_MAIN = os.path.join(TESTS_CPP, "accel_refit_main.cpp")
REFIT_ASYNC_MAIN = os.path.join(TESTS_CPP, "accel_refit_async_main.cpp")
REFIT_HOSTTREE_MAIN = os.path.join(TESTS_CPP, "accel_refit_hosttree_main.cpp")
UPDATE_ARGS_MAIN = os.path.join(TESTS_CPP, "update_args_main.cpp")  # (its test also builds it with the sanitizers)
# the header-only programs of tests/cpp/ (no library, no GPU): name, the headers each depends on beside its
# own source, and whether build_host() builds it only where that source is present (a tests/ directory older
# than the program still gets everything it runs; the program's Python test fails without it)
_INC = os.path.join(ROOT, "include", "eray_hip.h")
HEADER_PROGRAMS = [
    ("update_args_main", ["rays_args.hpp", _INC], False),  # the update's argument checks
    ("gather_plan_main", ["gather_plan.hpp", "band_rows.hpp", _INC], False),  # the multi-GPU gather's planning
    ("bin_layout_main", ["bin_layout.hpp", "band_rows.hpp"], True),  # the screen bins' sizing
    ("frame_plan_main", ["frame_plan.hpp", "frame_params.hpp", "bin_layout.hpp", "band_rows.hpp", _INC], True),  # the frame calls' planning
    ("scene_build_main", ["scene_build.hpp", "texel_prog.hpp", "device_math.hpp", "glibc_cosf.hpp", "glibc_powf.hpp",
                          "frame_params.hpp", _INC], True),  # the scene upload's descriptors and texel programs
]


def build_host(jobs: int = 4, verbose: bool = False, force: bool = False) -> list[str]:
    """The C++ host (include/eray/, eray_amd/host/): liberay_host.so over the C-ABI library,
    the eray_main CLI (main.rs) and the tests/cpp/ test binaries (test_host, test_rays, test_accel, test_accel_dev, test_reach, test_update,
    test_refit_hosttree, accel_walk_main, accel_dev_main, accel_refit_main, accel_refit_hosttree_main, accel_refit_async_main,
    update_args_main, gather_plan_main, bin_layout_main, frame_plan_main, scene_build_main).  Plain g++: the
    host code never includes HIP headers."""
    hip_lib = build(jobs, verbose, force)
    host = os.path.join(PKG, "host")
    cxx = shutil.which("g++") or "g++"
    flags = ["-std=c++17", "-O2", "-fPIC", "-Wall", "-I" + os.path.join(ROOT, "include")]
    headers = [os.path.join(ROOT, "include", "eray", f) for f in os.listdir(os.path.join(ROOT, "include", "eray"))]
    headers.append(os.path.join(ROOT, "include", "eray_hip.h"))
    obj_dir = os.path.join(OBJ, "host")
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(BIN_DIR, exist_ok=True)
    link = ["-L" + LIB_DIR, "-leray_hip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/../lib",
            "-Wl,-rpath-link," + ROCM_LIB, "-Wl,-rpath," + ROCM_LIB]

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"host build failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")

    objs, cmds = [], []
    for src in HOST_SOURCES:
        s, o = os.path.join(host, src), os.path.join(obj_dir, src + ".o")
        objs.append(o)
        if force or not _newer(o, [s] + headers):
            cmds.append([cxx, *flags, "-c", s, "-o", o])
    with cf.ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
        list(ex.map(run, cmds))
    if force or cmds or not _newer(HOST_LIB, objs + [hip_lib]):
        run([cxx, "-shared", "-o", HOST_LIB, *objs, *link])
    outs = [HOST_LIB]
    for name, src in (("eray_main", os.path.join(host, "main.cpp")),
                      ("test_host", os.path.join(ROOT, "tests", "cpp", "test_host.cpp")),
                      ("test_rays", os.path.join(ROOT, "tests", "cpp", "test_rays.cpp")),
                      ("test_accel", os.path.join(ROOT, "tests", "cpp", "test_accel.cpp")),
                      ("test_accel_dev", os.path.join(ROOT, "tests", "cpp", "test_accel_dev.cpp")),
                      ("test_reach", os.path.join(ROOT, "tests", "cpp", "test_reach.cpp")),
                      ("test_update", os.path.join(ROOT, "tests", "cpp", "test_update.cpp")),
                      ("test_refit_hosttree", os.path.join(ROOT, "tests", "cpp", "test_refit_hosttree.cpp"))):
        exe = os.path.join(BIN_DIR, name)
        if force or not _newer(exe, [src, HOST_LIB] + headers):
            run([cxx, *flags, src, "-o", exe, "-L" + LIB_DIR, "-leray_host", *link])
        outs.append(exe)
    # the ray-query hierarchy on the CPU (what the programs share is tests/cpp/accel_emul.hpp): the builder and
    # the shared walk; the device-side builder, its refit and the refit on the stream emulated with the headers
    # their kernels share, and the checker.  No GPU library.  (The header-only programs follow.)
    accel_deps = [os.path.join(TESTS_CPP, f) for f in sorted(os.listdir(TESTS_CPP)) if f.endswith(".hpp")]
    accel_deps += [os.path.join(CSRC, h) for h in ACCEL_DEV_HEADERS]
    for name, main_src, more in (("accel_walk_main", WALK_MAIN, [os.path.join(CSRC, "accel_build.cpp")]),
                                 ("accel_dev_main", DEV_MAIN, ACCEL_DEV_SOURCES),
                                 ("accel_refit_main", REFIT_MAIN, ACCEL_DEV_SOURCES),
                                 ("accel_refit_hosttree_main", REFIT_HOSTTREE_MAIN, ACCEL_DEV_SOURCES),
                                 ("accel_refit_async_main", REFIT_ASYNC_MAIN, ACCEL_DEV_SOURCES)):
        exe = os.path.join(BIN_DIR, name)
        if force or not _newer(exe, [main_src, *more, *accel_deps]):
            run([cxx, *ACCEL_WALK_FLAGS, main_src, *more, "-o", exe])
        outs.append(exe)
    for name, deps, optional in HEADER_PROGRAMS:
        main_src, exe = os.path.join(TESTS_CPP, name + ".cpp"), os.path.join(BIN_DIR, name)
        if optional and not os.path.exists(main_src):
            continue
        if force or not _newer(exe, [main_src, *(os.path.join(CSRC, d) for d in deps)]):
            run([cxx, "-std=c++17", "-O2", "-Wall", main_src, "-o", exe])
        outs.append(exe)
    return outs


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 4))
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--host", action="store_true", help="also build the C++ host (liberay_host.so, bin/)")
    a = ap.parse_args()
    print(build(a.jobs, a.verbose, a.force))
    if a.host:
        print("\n".join(build_host(a.jobs, a.verbose, a.force)))


if __name__ == "__main__":
    main()
