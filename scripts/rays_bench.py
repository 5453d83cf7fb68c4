"""Times eray_cast_rays against the brute-force render of the same rays (diagnostics, GPU only).

    python scripts/rays_bench.py [--repeats 5] [--small-only] [--no-1m] [--out FILE.json]
    python scripts/rays_bench.py --accel-build both [--repeats 5] [--no-1m] [--out FILE.json]
    python scripts/rays_bench.py --secondary [--repeats 5] [--out FILE.jsonl]

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

--secondary measures out_rgb's shadow and reflected rays instead: C2's cube scene (no hierarchy
object), then the 69,451-face mesh with its true box, two point lights and a reflective material
through the host-built hierarchy — 2^20 incoherent rays and the 3840x2160 camera's rays, bounces 0
and 2 — and eray_rays_reach_light for 2^20 shadow rays with the hierarchy and with the tiles.  For a
same-session comparison run it once per library (ERAY_LIB=<the parent commit's build>, then the
product), alternating; --out appends.  A library that predates eray_rays_reach_light skips that leg.
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


def timed_forms(stream, forms: dict, repeats: int) -> dict:
    """`repeats` device-event timings of each form, alternating, after one untimed round."""
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
    return {k: summary(v) for k, v in times.items()}


SECONDARY_LIGHTS = ((4.0, 3.0, 2.0), (-4.5, 3.5, 0.5))


def bench_secondary_large(repeats: int) -> dict:
    """out_rgb on the 69,451-face mesh with its true box, two point lights, one ambient light and a
    1 x 1 reflection image of 0.5 (so that bounces = 2 casts reflected rays), through the host-built
    hierarchy: 2^20 incoherent rays and the 3840x2160 camera's rays, bounces 0 and 2; the colours
    are checked byte for byte against the context without a hierarchy on the incoherent rays.  Then
    eray_rays_reach_light (where the library has it) for 2^20 shadow rays formed from those rays'
    hits, with the hierarchy and with the tiles."""
    stream = torch.cuda.Stream()
    mesh = generated_mesh(**meshgen.STANDIN_70K)
    lo, hi = mesh[0].reshape(-1, 3).min(0), mesh[0].reshape(-1, 3).max(0)
    ctxs, bufs = [], []
    try:
        for _ in range(2):
            c = capi.Context(0)
            ctxs.append(c)
            c.set_stream(stream.cuda_stream)
            c.set_camera(capi.make_camera((0.0, 0.0, 5.0), (60.0, 60.0), 64, 1.0))
            refl = c.to_device(np.full((1, 1), 0.5, np.float32))
            bufs.append(refl)
            c.add_object(*mesh, tuple(lo), tuple(hi), reflection=refl.image())
            for p in SECONDARY_LIGHTS:
                c.add_light(capi.make_light(p, "point"))
            c.add_light(capi.make_light((0.0, 2.0, 0.0), "ambient", brightness=0.2))
        ctx, actx = ctxs
        info = actx.build_ray_accel()
        out = {"workload": "secondary, 69451 faces, true box, 2 point lights", "repeats": repeats, "accel_info": info,
               "lib": os.path.basename(capi.LIB_PATH)}
        n = 1 << 20
        inco_h = sphere_rays(n)
        inco = ctx.to_device(inco_h)
        cam_h = camera_rays((0.0, 0.0, 5.0), fov_for(3840, 2160), 3840, 2160)
        cam = ctx.to_device(cam_h)
        ncam = cam_h.shape[0]
        rgb, hit = ctx.empty((ncam, 3), np.float32), ctx.empty((n,), capi.HIT_DTYPE)
        bufs += [inco, cam, rgb, hit]
        # the same colours with and without the hierarchy (the incoherent rays, bounces 2)
        ctx.cast_rays_device(inco.ptr, n, out_hit=hit.ptr, out_rgb=rgb.ptr, bounces=2, flags=capi.RAYS_NORMALIZE)
        ctx.synchronize()
        want, hits = rgb.numpy()[:n].tobytes(), hit.numpy()
        actx.cast_rays_device(inco.ptr, n, out_rgb=rgb.ptr, bounces=2, flags=capi.RAYS_NORMALIZE)
        ctx.synchronize()
        if rgb.numpy()[:n].tobytes() != want:
            raise AssertionError("secondary: the hierarchy's out_rgb differs from the tiles'")
        out["hit_rays_incoherent"] = int((hits["object"] >= 0).sum())
        forms = {}
        for b in (0, 2):
            forms[f"rgb_incoherent_2^20_bounces{b}"] = lambda b=b: actx.cast_rays_device(
                inco.ptr, n, out_rgb=rgb.ptr, bounces=b, flags=capi.RAYS_NORMALIZE)
            forms[f"rgb_camera_3840x2160_bounces{b}"] = lambda b=b: actx.cast_rays_device(
                cam.ptr, ncam, out_rgb=rgb.ptr, bounces=b)
        if hasattr(capi.lib(), "eray_rays_reach_light"):
            ok = hits["object"] >= 0
            P, N = hits["position"][ok], hits["normal"][ok]
            S = (P + N * np.float32(0.1)).astype(np.float32)
            sh, tg = [], []
            for L in SECONDARY_LIGHTS:
                d = np.float32(L) - P
                sq = np.float32(0.0) + d[:, 0] * d[:, 0]
                sq = sq + d[:, 1] * d[:, 1]
                sq = sq + d[:, 2] * d[:, 2]
                sh.append(np.concatenate([S, d / np.sqrt(sq)[:, None]], axis=1))
                tg.append(np.tile(np.float32(L), (P.shape[0], 1)))
            sh, tg = np.concatenate(sh), np.concatenate(tg)
            idx = np.resize(np.arange(sh.shape[0]), n)  # (repeated from the start when fewer than 2^20)
            d_sh, d_tg = ctx.to_device(np.ascontiguousarray(sh[idx], np.float32)), ctx.to_device(np.ascontiguousarray(tg[idx], np.float32))
            words = ctx.empty((n,), np.uint32)
            bufs += [d_sh, d_tg, words]
            ctx.rays_reach_light_device(d_sh.ptr, d_tg.ptr, n, words.ptr)
            ctx.synchronize()
            w = words.numpy()
            actx.rays_reach_light_device(d_sh.ptr, d_tg.ptr, n, words.ptr)
            ctx.synchronize()
            if words.numpy().tobytes() != w.tobytes():
                raise AssertionError("secondary: the hierarchy's reach words differ from the tiles'")
            out["reach_blocked"] = int((w == 0).sum())
            forms["reach_2^20_accel"] = lambda: actx.rays_reach_light_device(d_sh.ptr, d_tg.ptr, n, words.ptr)
            forms["reach_2^20_tiled"] = lambda: ctx.rays_reach_light_device(d_sh.ptr, d_tg.ptr, n, words.ptr)
        out.update(timed_forms(stream, forms, repeats))
        return out
    finally:
        for a in bufs:
            a.free()
        for c in ctxs:
            c.close()


def bench_secondary_small(repeats: int) -> dict:
    """C2's cube scene (main.rs's, 1920x1080), out_rgb of the camera's rays: no object gets a
    hierarchy, so the context without one runs rays_kernel, which the secondary-ray change leaves
    alone; after a default build the same rays go through rays_accel_kernel with every object
    scanned."""
    stream = torch.cuda.Stream()
    width, height = 1920, 1080
    fov = fov_for(width, height)
    mesh = load_obj_file(os.path.join(ROOT, "objects", "cube.obj"))
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    scene = MainScene(ctx, *mesh, width, height, texture=1024, fov=fov)
    actx = capi.Context(0)
    actx.set_stream(stream.cuda_stream)
    ascene = MainScene(actx, *mesh, width, height, texture=1024, fov=fov)
    info = actx.build_ray_accel()
    n = width * height
    rays = ctx.to_device(camera_rays((0.0, 0.0, 5.0), fov, width, height))
    rgb = ctx.empty((n, 3), np.float32)
    try:
        forms = {"rgb_cube_1920x1080": lambda: ctx.cast_rays_device(rays.ptr, n, out_rgb=rgb.ptr),
                 "rgb_cube_1920x1080_after_build": lambda: actx.cast_rays_device(rays.ptr, n, out_rgb=rgb.ptr)}
        forms["rgb_cube_1920x1080"]()
        ctx.synchronize()
        want = rgb.numpy().tobytes()
        forms["rgb_cube_1920x1080_after_build"]()
        ctx.synchronize()
        if rgb.numpy().tobytes() != want:
            raise AssertionError("secondary: the cube's out_rgb differs after the build")
        out = {"workload": "secondary, C2 cube scene", "repeats": repeats, "accel_info": info,
               "lib": os.path.basename(capi.LIB_PATH)}
        out.update(timed_forms(stream, forms, repeats))
        return out
    finally:
        rays.free()
        rgb.free()
        ascene.close()
        actx.close()
        scene.close()
        ctx.close()


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
    ap.add_argument("--secondary", action="store_true",
                    help="measure out_rgb's secondary rays through the hierarchy and the reach query instead")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.secondary:
        lines = []
        for fn in (bench_secondary_small, bench_secondary_large):
            lines.append(fn(a.repeats))
            print(json.dumps(lines[-1]), flush=True)
        if a.out:
            with open(a.out, "a") as f:  # (appended: one file collects the libraries of an A/B)
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")
        return
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
