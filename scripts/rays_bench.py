"""Times eray_cast_rays against the brute-force render of the same rays (diagnostics, GPU only).

    python scripts/rays_bench.py [--repeats 5] [--small-only] [--no-1m] [--out FILE.json]
    python scripts/rays_bench.py --accel-build both [--repeats 5] [--no-1m] [--out FILE.json]

Two cameras, main.rs's scene: C2 (1920x1080, cube.obj) and 3840x2160 over the 69,451-face
stand-in mesh (bench.py's north-star scene).  The rays are the camera's own pixel-corner rays
(camera.rs:57-76, restated here in np.float32 and checked against eray_render's faces), so
eray_render with ERAY_RENDER_BRUTE_FORCE runs the same intersection tests plus shading — the code
that existed before the ray queries — and is the yardstick of the hit-only query.

Per camera and per form (hit records through the LDS tiles, hit records with
ERAY_RAYS_BRUTE_FORCE, the brute-force render, hit records through the ray-query hierarchy),
`repeats` timings by device events around one call each, the forms alternating inside every
repeat, after one untimed warm-up round; medians and the min..max spread.  The hierarchy form
runs in a second context holding the same scene plus eray_scene_build_ray_accel's hierarchy (no
flag selects the tiles once a hierarchy exists), on the same stream; its records are checked
byte for byte against the tiled ones.

Then the incoherent workload the hierarchy is for: 2^22 rays from the radius-3 sphere toward
targets uniform in [-1, 1]^3 against the 69,451-face mesh with its true box (tiles against
hierarchy), and 2^20 such rays against the 1M-face mesh (--no-1m skips it), with each mesh's build
time and device bytes.  One JSON line per workload.  No GPU: the context fails to open.

--accel-build {host,device,both} measures the hierarchy's builders instead (eray_scene_build_ray_accel
and eray_scene_build_ray_accel_device): per scene — the 69,451-face mesh, the 1M-face mesh, 64
objects of 1,024 faces — `repeats` builds of each chosen builder in one process, alternating after
one untimed round (build_ms: host wall time of the whole call, final synchronisation included),
and the query workloads (2^22 incoherent rays / 69k, 2^20 / 1M, the 3840x2160 camera's rays / 69k)
timed by device events through each builder's tree, alternating likewise, the records compared
byte for byte between the trees.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from eray_amd import capi, meshgen  # noqa: E402
from eray_amd.frame import MainScene, fov_for  # noqa: E402
from eray_amd.objfile import load_obj_file  # noqa: E402


def camera_rays(center, fov, width: int, height: int, z_dist: float = 1.0) -> np.ndarray:
    """Camera::pixel_to_ray(x / W, y / H) for every pixel (camera.rs:57-76; Ray::new normalises),
    each operation in f32 in the reference's order: (H * W, 6) start | dir."""
    f = np.float32
    C = np.array(center, f)
    vw = f(f(fov[0]) / f(fov[1])) * f(2.0)
    horizontal, vertical = np.array([vw, 0, 0], f), np.array([0, 2, 0], f)
    botleft = ((C - horizontal / f(2.0)) - vertical / f(2.0)) - np.array([0, 0, z_dist], f)
    xf = (np.arange(width, dtype=f) / f(width))[None, :, None]
    yf = (np.arange(height, dtype=f) / f(height))[:, None, None]
    d = ((botleft + horizontal * xf) + vertical * yf) - C
    sq = f(0.0) + d[..., 0] * d[..., 0]
    sq = sq + d[..., 1] * d[..., 1]
    sq = sq + d[..., 2] * d[..., 2]
    d = d / np.sqrt(sq)[..., None]
    rays = np.empty((height, width, 6), f)
    rays[..., :3] = C
    rays[..., 3:] = d
    return rays.reshape(-1, 6)


def summary(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "samples_ms": [round(v, 4) for v in ms]}


def bench(name: str, mesh, width: int, height: int, repeats: int) -> dict:
    stream = torch.cuda.Stream()
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    fov = fov_for(width, height)
    scene = MainScene(ctx, *mesh, width, height, texture=1024, fov=fov)
    actx = capi.Context(0)  # the same scene with a hierarchy
    actx.set_stream(stream.cuda_stream)
    ascene = MainScene(actx, *mesh, width, height, texture=1024, fov=fov)
    info = actx.build_ray_accel()
    n = width * height
    rays = ctx.to_device(camera_rays((0.0, 0.0, 5.0), fov, width, height))
    hit = ctx.empty((n,), capi.HIT_DTYPE)
    with torch.cuda.stream(stream):
        rgb = torch.empty((height, width, 3), dtype=torch.float32, device="cuda")
        face = torch.empty((height, width), dtype=torch.int32, device="cuda")
    forms = {
        "cast_rays_tiled": lambda: ctx.cast_rays_device(rays.ptr, n, out_hit=hit.ptr),
        "cast_rays_brute": lambda: ctx.cast_rays_device(rays.ptr, n, out_hit=hit.ptr, flags=capi.RAYS_BRUTE_FORCE),
        "render_brute": lambda: ctx.render(width, height, out_rgb=rgb.data_ptr(), out_face=face.data_ptr(),
                                           flags=capi.RENDER_BRUTE_FORCE),
        "cast_rays_accel": lambda: actx.cast_rays_device(rays.ptr, n, out_hit=hit.ptr),
    }
    try:
        # the same work: the query's faces are the render's
        forms["render_brute"]()
        forms["cast_rays_tiled"]()
        ctx.synchronize()
        h = hit.numpy()
        got = np.where(h["object"] >= 0, h["face"], -1).reshape(height, width)
        want = face.cpu().numpy()
        if not np.array_equal(got, want):
            raise AssertionError(f"{name}: cast_rays faces differ from eray_render's at {int((got != want).sum())} pixels")
        forms["cast_rays_brute"]()
        ctx.synchronize()
        if hit.numpy().tobytes() != h.tobytes():
            raise AssertionError(f"{name}: ERAY_RAYS_BRUTE_FORCE records differ from the tiled ones")
        forms["cast_rays_accel"]()
        ctx.synchronize()
        if hit.numpy().tobytes() != h.tobytes():
            raise AssertionError(f"{name}: the hierarchy's records differ from the tiled ones")
        times = {k: [] for k in forms}
        for rep in range(repeats + 1):  # round 0: warm-up
            for k, fn in forms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                fn()
                t1.record(stream)
                t1.synchronize()
                if rep:
                    times[k].append(t0.elapsed_time(t1))
        out = {"camera": name, "width": width, "height": height, "faces": int(mesh[0].shape[0]), "rays": n,
               "hit_rays": int((h["object"] >= 0).sum()), "repeats": repeats}
        out.update({k: summary(v) for k, v in times.items()})
        med = {k: out[k]["median_ms"] for k in forms}
        out["tiled_over_render_brute"] = round(med["cast_rays_tiled"] / med["render_brute"], 4)
        out["tiled_over_cast_rays_brute"] = round(med["cast_rays_tiled"] / med["cast_rays_brute"], 4)
        out["accel_over_tiled"] = round(med["cast_rays_accel"] / med["cast_rays_tiled"], 4)
        out["accel_info"] = info
        return out
    finally:
        rays.free()
        hit.free()
        ascene.close()
        actx.close()
        scene.close()
        ctx.close()


def sphere_rays(n: int, seed: int = 7) -> np.ndarray:
    """n rays from the radius-3 sphere toward targets uniform in [-1, 1]^3 (dir not normalised)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    start = 3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    target = rng.uniform(-1, 1, (n, 3))
    return np.ascontiguousarray(np.concatenate([start, target - start], axis=1), np.float32)


def bench_incoherent(name: str, mesh, nrays: int, repeats: int) -> dict:
    """Incoherent rays against one mesh with its true box: the tiles (context without a hierarchy)
    against the hierarchy (a second context), alternating; records compared byte for byte."""
    stream = torch.cuda.Stream()
    lo, hi = mesh[0].reshape(-1, 3).min(0), mesh[0].reshape(-1, 3).max(0)
    ctxs = []
    for _ in range(2):
        c = capi.Context(0)
        c.set_stream(stream.cuda_stream)
        c.set_camera(capi.make_camera((0.0, 0.0, 5.0), (60.0, 60.0), 64, 1.0))
        c.add_object(*mesh, tuple(lo), tuple(hi))
        ctxs.append(c)
    ctx, actx = ctxs
    info = actx.build_ray_accel()
    rays = ctx.to_device(sphere_rays(nrays))
    hit = ctx.empty((nrays,), capi.HIT_DTYPE)
    forms = {
        "cast_rays_tiled": lambda: ctx.cast_rays_device(rays.ptr, nrays, out_hit=hit.ptr, flags=capi.RAYS_NORMALIZE),
        "cast_rays_accel": lambda: actx.cast_rays_device(rays.ptr, nrays, out_hit=hit.ptr, flags=capi.RAYS_NORMALIZE),
    }
    try:
        forms["cast_rays_tiled"]()
        ctx.synchronize()
        h = hit.numpy()
        forms["cast_rays_accel"]()
        ctx.synchronize()
        if hit.numpy().tobytes() != h.tobytes():
            raise AssertionError(f"{name}: the hierarchy's records differ from the tiled ones")
        times = {k: [] for k in forms}
        for rep in range(repeats + 1):  # round 0: warm-up
            for k, fn in forms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                fn()
                t1.record(stream)
                t1.synchronize()
                if rep:
                    times[k].append(t0.elapsed_time(t1))
        out = {"workload": name, "faces": int(mesh[0].shape[0]), "rays": nrays, "hit_rays": int((h["object"] >= 0).sum()),
               "repeats": repeats, "accel_info": info}
        out.update({k: summary(v) for k, v in times.items()})
        out["tiled_over_accel"] = round(out["cast_rays_tiled"]["median_ms"] / out["cast_rays_accel"]["median_ms"], 2)
        return out
    finally:
        rays.free()
        hit.free()
        for c in ctxs:
            c.close()


def bench_builders(name: str, objects: list, builders: list, workloads: dict, repeats: int) -> dict:
    """Per builder a context holding `objects` ((mesh, lo, hi) each) and its hierarchy: build_ms of
    `repeats` alternating builds, then each workload ({name: (n, 6) rays}) through each tree."""
    stream = torch.cuda.Stream()
    ctxs = {}
    for b in builders:
        c = capi.Context(0)
        c.set_stream(stream.cuda_stream)
        c.set_camera(capi.make_camera((0.0, 0.0, 5.0), (60.0, 60.0), 64, 1.0))
        for mesh, lo, hi in objects:
            c.add_object(*mesh, tuple(lo), tuple(hi))
        ctxs[b] = c
    out = {"scene": name, "objects": len(objects), "faces": int(sum(m[0].shape[0] for m, _, _ in objects)), "repeats": repeats}
    bufs = []
    try:
        build_ms = {b: [] for b in builders}
        info = {}
        for rep in range(repeats + 1):  # round 0: warm-up
            for b in builders:
                info[b] = ctxs[b].build_ray_accel(1, device=(b == "device"))
                if rep:
                    build_ms[b].append(info[b]["build_ms"])
        for b in builders:
            out[f"build_{b}"] = summary(build_ms[b])
            out[f"info_{b}"] = info[b]
        if len(builders) == 2:
            out["host_over_device_build"] = round(out["build_host"]["median_ms"] / out["build_device"]["median_ms"], 2)
        for wname, rays_h in workloads.items():
            n = rays_h.shape[0]
            rays = ctxs[builders[0]].to_device(rays_h)
            hit = ctxs[builders[0]].empty((n,), capi.HIT_DTYPE)
            bufs += [rays, hit]
            records = {}
            times = {b: [] for b in builders}
            for rep in range(repeats + 1):
                for b in builders:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    ctxs[b].cast_rays_device(rays.ptr, n, out_hit=hit.ptr, flags=capi.RAYS_NORMALIZE)
                    t1.record(stream)
                    t1.synchronize()
                    if rep:
                        times[b].append(t0.elapsed_time(t1))
                    else:
                        records[b] = hit.numpy().tobytes()
            if len(set(records.values())) != 1:
                raise AssertionError(f"{name}, {wname}: the two trees' records differ")
            w = {"rays": n, **{f"query_{b}_tree": summary(times[b]) for b in builders}}
            if len(builders) == 2:
                w["device_over_host_tree"] = round(w["query_device_tree"]["median_ms"] / w["query_host_tree"]["median_ms"], 3)
            out[wname] = w
        return out
    finally:
        for a in bufs:
            a.free()
        for c in ctxs.values():
            c.close()


def bench_accel_build(which: str, repeats: int, no_1m: bool) -> list:
    builders = ["host", "device"] if which == "both" else [which]
    lines = []

    def one(mesh):
        p = mesh[0].reshape(-1, 3)
        return (mesh, p.min(0), p.max(0))

    m70 = generated_mesh(**meshgen.STANDIN_70K)
    cam = camera_rays((0.0, 0.0, 5.0), fov_for(3840, 2160), 3840, 2160)
    lines.append(bench_builders("69451 faces", [one(m70)], builders,
                                {"incoherent_2^22": sphere_rays(1 << 22), "camera_3840x2160": cam}, repeats))
    print(json.dumps(lines[-1]), flush=True)
    many = []
    for k in range(64):  # 64 displaced spheres of 1,024 faces on a 4 x 4 x 4 lattice
        m = generated_mesh(1024, 100 + k)
        c = np.float32([(k % 4 - 1.5) * 0.5, (k // 4 % 4 - 1.5) * 0.5, (k // 16 - 1.5) * 0.5])
        pos = ((m[0].reshape(-1, 3, 3) * np.float32(0.2)) + c).reshape(-1, 9).astype(np.float32)
        many.append(one((pos, m[1], m[2])))
    lines.append(bench_builders("64 objects x 1024 faces", many, builders, {"incoherent_2^20": sphere_rays(1 << 20)}, repeats))
    print(json.dumps(lines[-1]), flush=True)
    if not no_1m:
        lines.append(bench_builders("1M faces", [one(generated_mesh(**meshgen.SYNTH_1M))], builders,
                                    {"incoherent_2^20": sphere_rays(1 << 20)}, repeats))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def generated_mesh(triangles: int, seed: int):
    v, n, t, F, _, _ = meshgen.displaced_sphere(triangles, seed)
    return (v[F].reshape(triangles, 9).astype(np.float32), n[F].reshape(triangles, 9).astype(np.float32),
            t[F].reshape(triangles, 6).astype(np.float32))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small-only", action="store_true", help="C2 only (skip the 69,451-face camera)")
    ap.add_argument("--no-1m", action="store_true", help="skip the 1M-face incoherent workload")
    ap.add_argument("--accel-build", choices=("host", "device", "both"), default="",
                    help="measure the hierarchy's builders and the queries through their trees instead")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.accel_build:
        lines = bench_accel_build(a.accel_build, a.repeats, a.no_1m)
        if a.out:
            with open(a.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")
        return
    lines = [bench("C2 1920x1080 cube", load_obj_file(os.path.join(ROOT, "objects", "cube.obj")), 1920, 1080, a.repeats)]
    print(json.dumps(lines[-1]), flush=True)
    if not a.small_only:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "standin_69451.obj")
            meshgen.generate(path, 69451, 42)
            mesh = load_obj_file(path)
        lines.append(bench("3840x2160 69451 faces", mesh, 3840, 2160, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
        lines.append(bench_incoherent("2^22 sphere rays, 69451 faces, true box", generated_mesh(**meshgen.STANDIN_70K), 1 << 22,
                                      a.repeats))
        print(json.dumps(lines[-1]), flush=True)
        if not a.no_1m:
            lines.append(bench_incoherent("2^20 sphere rays, 1M faces, true box", generated_mesh(**meshgen.SYNTH_1M), 1 << 20,
                                          a.repeats))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
