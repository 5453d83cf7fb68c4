"""Times the general tracer with and without the ray-query hierarchy (diagnostics, GPU only).

    python scripts/trace_accel_bench.py [--repeats 5] [--with-1m] [--only gain|c3] [--default-only] [--out FILE.jsonl]

Gain.  The 69,451-face displaced sphere with its TRUE bounding box (so that shadow and reflected
rays reach its face search) on a reflective two-face floor, two point lights and an ambient one,
1920x1080, for (anti_aliasing, bounces) in (4, 0), (0, 2), (4, 2); with --with-1m the 1M-face sphere
at (0, 1).  Two forms of the same call in one context that holds the hierarchy: the default (the
hierarchy) and ERAY_RENDER_NO_RAY_ACCEL (the per-lane scan, the tracer before it took the
hierarchy).  The two frames are compared byte for byte first.

No harm.  C3 (main.rs's scene around the 69,451-face mesh as the reference loads it: the (0,0,0)
box that rejects almost every shadow ray) at 1920x1080 with AA = 4 and a hierarchy built: the
default against the flag.  The library does not take the hierarchy form there (no covered object
has a box that lets such rays in; trace_ray_accel_objects() reports 0), so both run the same kernel;
for the parent commit's figure run the script again with ERAY_LIB=<its build> --only c3 in the
same sitting, alternating.

Every sample is eray_render_frames' mean_frame_ms (device events around `frames` back-to-back
frames, replayed from the call's cached graph; frames chosen from a warm-up frame so that a sample
lasts about a quarter of a second, at most 64).  After one untimed round the forms alternate
inside each of `repeats` rounds; medians and the min..max spread.  One JSON line per case.
No GPU: the context fails to open.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from eray_amd import capi, meshgen  # noqa: E402
from eray_amd.frame import MainScene  # noqa: E402

W, H = 1920, 1080
LIGHTS = ((4.0, 3.0, 2.0), (-4.5, 3.5, 0.5))
FLOOR_Y = -1.05
NO_RAY_ACCEL = capi.RENDER_NO_RAY_ACCEL  # (None: the default form alone, see main)


def summary(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "samples_ms": [round(v, 4) for v in ms]}


def generated_mesh(triangles: int, seed: int = 42):
    v, n, t, F, _, _ = meshgen.displaced_sphere(triangles, seed)
    return (v[F].reshape(triangles, 9).astype(np.float32), n[F].reshape(triangles, 9).astype(np.float32),
            t[F].reshape(triangles, 6).astype(np.float32))


def floor_mesh():
    y, r = FLOOR_Y, 5.0
    pos = np.float32([[-r, y, -r, -r, y, r, r, y, r], [-r, y, -r, r, y, r, r, y, -r]])
    return pos, np.float32([[0, 1, 0] * 3] * 2), np.float32([[0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 0]])


def timed_forms(ctx, forms: dict, repeats: int, budget_ms: float = 250.0) -> dict:
    """forms: name -> f(frames) -> mean ms per frame.  A warm-up frame per form picks its frame count."""
    frames = {}
    for k, fn in forms.items():
        fn(1)
        one = fn(1)
        frames[k] = int(min(64, max(1, budget_ms / max(one, 1e-3))))
        if frames[k] > 1:
            fn(frames[k])  # (captures the graph outside the timed rounds)
    times = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            times[k].append(fn(frames[k]))
    out = {k: summary(v) for k, v in times.items()}
    for k in out:
        out[k]["frames_per_sample"] = frames[k]
    return out


def render_forms(ctx, rgb, aa: int, bounces: int) -> dict:
    def form(flags):
        return lambda frames: ctx.render_frames(frames, W, H, out_rgb=rgb.ptr, flags=flags, bounces=bounces,
                                                anti_aliasing=aa, aa_seed=11, timed=True)
    forms = {"default": form(capi.RENDER_DEFAULT)}
    if NO_RAY_ACCEL is not None:
        forms["no_ray_accel"] = form(NO_RAY_ACCEL)
    return forms


def same_frames(ctx, rgb, aa: int, bounces: int) -> int:
    """Renders both forms once and compares the bytes; the objects the default form searched through
    the hierarchy."""
    ctx.render(W, H, out_rgb=rgb.ptr, bounces=bounces, anti_aliasing=aa, aa_seed=11)
    ctx.synchronize()
    objects = ctx.trace_ray_accel_objects() if hasattr(capi.lib(), "eray_debug_trace_ray_accel") else -1
    if NO_RAY_ACCEL is None:
        return objects
    want = rgb.numpy().tobytes()
    ctx.memset(rgb.ptr, 0, rgb.nbytes)
    ctx.render(W, H, out_rgb=rgb.ptr, bounces=bounces, anti_aliasing=aa, aa_seed=11, flags=NO_RAY_ACCEL)
    ctx.synchronize()
    if rgb.numpy().tobytes() != want:
        raise AssertionError(f"aa={aa} bounces={bounces}: the hierarchy form's frame differs from the scan's")
    return objects


def bench_gain(triangles: int, cases, repeats: int, emit) -> None:
    stream = torch.cuda.Stream()
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    bufs = []
    try:
        mesh = generated_mesh(triangles)
        lo, hi = mesh[0].reshape(-1, 3).min(0), mesh[0].reshape(-1, 3).max(0)
        refl = ctx.to_device(np.full((1, 1), 0.5, np.float32))
        bufs.append(refl)
        ctx.set_camera(capi.make_camera((0.0, 0.3, 3.0), (16.0, 9.0), W, 1.0))
        ctx.add_object(*mesh, tuple(lo), tuple(hi), reflection=refl.image())
        fl = floor_mesh()
        ctx.add_object(*fl, tuple(fl[0].reshape(-1, 3).min(0)), tuple(fl[0].reshape(-1, 3).max(0)), reflection=refl.image())
        for p in LIGHTS:
            ctx.add_light(capi.make_light(p, "point"))
        ctx.add_light(capi.make_light((0.0, 2.0, 0.0), "ambient", brightness=0.2))
        info = ctx.build_ray_accel()
        rgb = ctx.empty((H, W, 3), np.float32)
        bufs.append(rgb)
        for aa, bounces in cases:
            objects = same_frames(ctx, rgb, aa, bounces)
            out = {"case": "gain", "faces": triangles, "true_box": True, "width": W, "height": H, "aa": aa, "bounces": bounces,
                   "repeats": repeats, "accel_info": info, "trace_ray_accel_objects": objects,
                   "lib": os.path.basename(capi.LIB_PATH)}
            out.update(timed_forms(ctx, render_forms(ctx, rgb, aa, bounces), repeats))
            if "no_ray_accel" in out:
                out["scan_over_hierarchy"] = round(out["no_ray_accel"]["median_ms"] / out["default"]["median_ms"], 3)
            emit(out)
    finally:
        for a in bufs:
            a.free()
        ctx.close()


def bench_c3(repeats: int, emit) -> None:
    stream = torch.cuda.Stream()
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    mesh = generated_mesh(**meshgen.STANDIN_70K)
    scene = MainScene(ctx, *mesh, W, H, texture=1024, fov=(16.0, 9.0))
    rgb = ctx.empty((H, W, 3), np.float32)
    try:
        info = ctx.build_ray_accel()
        objects = same_frames(ctx, rgb, 4, 0)
        out = {"case": "c3 no-harm", "faces": int(mesh[0].shape[0]), "true_box": False, "width": W, "height": H, "aa": 4,
               "bounces": 0, "repeats": repeats, "accel_info": info, "trace_ray_accel_objects": objects,
               "lib": os.path.basename(capi.LIB_PATH)}
        out.update(timed_forms(ctx, render_forms(ctx, rgb, 4, 0), repeats))
        emit(out)
    finally:
        rgb.free()
        scene.close()
        ctx.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--with-1m", action="store_true", help="also the 1M-face sphere at (aa, bounces) = (0, 1)")
    ap.add_argument("--only", choices=("gain", "c3"), default="")
    ap.add_argument("--default-only", action="store_true",
                    help="time the default form alone (a variant build of the kernels: the scan is the product's)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    global NO_RAY_ACCEL
    if a.default_only or not hasattr(capi.lib(), "eray_debug_trace_ray_accel"):  # (or a library that predates the flag)
        NO_RAY_ACCEL = None

    def emit(rec: dict) -> None:
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.only != "gain":
        bench_c3(a.repeats, emit)
    if a.only != "c3":
        bench_gain(meshgen.STANDIN_70K["triangles"], ((4, 0), (0, 2), (4, 2)), a.repeats, emit)
        if a.with_1m:
            bench_gain(1_000_000, ((0, 1),), a.repeats, emit)


if __name__ == "__main__":
    main()
