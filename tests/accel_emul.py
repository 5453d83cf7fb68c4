"""What the tests of the ray-query hierarchy's CPU programs share (tests/test_accel_host.py,
test_accel_dev_host.py, test_accel_refit_host.py, test_accel_refit_async_host.py; the programs'
own shared part is tests/cpp/accel_emul.hpp): the mesh files, the parser of the figures, the run of
a program that build_host() built, and the sanitizer build and the check of its run."""
import os
import shutil
import subprocess

import numpy as np

from eray_amd import meshgen
from eray_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZER_FLAGS = [f for f in B.ACCEL_WALK_FLAGS if f != "-O2"]


def write_spheres(folder, sizes):
    """sphere{T}.bin in `folder` per T of `sizes`: the T x 9 float32 face positions of
    meshgen.displaced_sphere(T, 42).  Returns the paths."""
    out = []
    for T in sizes:
        v, _, _, F, _, _ = meshgen.displaced_sphere(T, 42)
        out.append(str(folder / f"sphere{T}.bin"))
        v[F].reshape(T, 9).astype(np.float32).tofile(out[-1])
    return out


def figures(stdout, key="suite"):
    """{name: {figure: value}} of the program's '<key>=<name> figure=value ...' lines."""
    out = {}
    for line in stdout.splitlines():
        if line.startswith(key + "="):
            kv = dict(item.split("=", 1) for item in line.split())
            name = kv.pop(key)
            out[name] = {k: float(v) for k, v in kv.items()}
    return out


def run_built(name, args, timeout):
    """eray_amd/bin/<name>, built by build_host(), run with `args`; its output is printed."""
    exe = os.path.join(ROOT, "eray_amd", "bin", name)
    assert exe in B.build_host() and os.access(exe, os.X_OK)
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)
    print(r.stdout)
    return r


def asan_build(sources, exe, flags):
    """A program of its own with -fsanitize=address,undefined, to be run directly."""
    cxx = shutil.which("g++") or "g++"
    subprocess.run([cxx, *flags, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *sources,
                    "-o", exe], check=True, capture_output=True, text=True)


def assert_clean_sanitizer_run(r):
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
