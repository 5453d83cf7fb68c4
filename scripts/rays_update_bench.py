"""What moving geometry costs through the ray-query stack (one GPU, one process; needs an MI355X).

    python scripts/rays_update_bench.py [--repeats 15] [--no-1m] [--out profiles/rays/rays_update_bench.json]

Per mesh (the 69,451-face stand-in and the 1M-face sphere, each with its true box, two point lights
and one ambient light) the wall time, stream-synchronised, of getting from "the vertices moved" to
"a valid hierarchy for them":

  (a) reset_add_build    eray_scene_reset + eray_scene_add_object (host arrays) + the lights +
                         eray_scene_build_ray_accel_device: the only route before the update call
  (b) update_refit       eray_scene_update_object (device pointers) + eray_scene_refit_ray_accel
  (c) update_build       eray_scene_update_object (device pointers) + eray_scene_build_ray_accel_device

and, separately, the refit and the build alone (their own build_ms and the wall time).  The moved
positions are resident before the clock starts in (b) and (c); in (a) the host arrays cross the bus
inside the clock, as they must.  Then (d) the query cost: 2^20 incoherent rays (radius-3 sphere
toward [-1, 1]^3) through the tree refitted from the undisplaced mesh's split and through a fresh
device build, after a smooth displacement of 1 %, 5 % and 20 % of the mesh radius; records compared
byte for byte.  Two untimed warm-up rounds, then `repeats` rounds alternating the forms; medians and
the min..max spread; what a form returns is looked at after its clock has stopped.  Query times
are device-event times of the one kernel."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from eray_amd import capi, meshgen  # noqa: E402

LIGHTS = (((4.0, 3.0, 2.0), "point", 1.0), ((-4.5, 3.5, 0.5), "point", 1.0), ((0.0, 2.0, 0.0), "ambient", 0.2))
NRAYS = 1 << 20


def summary(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "samples_ms": [round(v, 4) for v in ms]}


def generated_mesh(triangles: int, seed: int):
    v, n, t, F, _, _ = meshgen.displaced_sphere(triangles, seed)
    return (v[F].reshape(triangles, 9).astype(np.float32), n[F].reshape(triangles, 9).astype(np.float32),
            t[F].reshape(triangles, 6).astype(np.float32))


def displaced(pos: np.ndarray, frac: float) -> np.ndarray:
    """A smooth displacement of `frac` of the mesh radius, per vertex position."""
    p = pos.astype(np.float64).reshape(-1, 3)
    radius = np.linalg.norm(p - p.mean(0), axis=1).max()
    return (p + frac * radius * np.sin(2.5 * p[:, [1, 2, 0]] / radius + 0.3)).reshape(-1, 9).astype(np.float32)


def box(pos):
    p = pos.reshape(-1, 3)
    return tuple(float(x) for x in p.min(0)), tuple(float(x) for x in p.max(0))


def sphere_rays(n: int, seed: int = 7) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    start = 3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    target = rng.uniform(-1, 1, (n, 3))
    return np.ascontiguousarray(np.concatenate([start, target - start], axis=1), np.float32)


def load(ctx, mesh, pos):
    ctx.scene_reset()
    ctx.set_camera(capi.make_camera((0.0, 0.0, 5.0), (60.0, 60.0), 64, 1.0))
    ctx.add_object(pos, mesh[1], mesh[2], *box(pos))
    for position, variant, brightness in LIGHTS:
        ctx.add_light(capi.make_light(position, variant, brightness=brightness))


WARMUP = 2


def wall(ctx, fn):
    """(ms, what fn returned): wall time between two stream synchronisations."""
    ctx.synchronize()
    t0 = time.perf_counter()
    res = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def bench_mesh(name: str, mesh, repeats: int) -> dict:
    stream = torch.cuda.Stream()
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    T = mesh[0].shape[0]
    moves = [displaced(mesh[0], 0.01 * (1 + k % 2)) for k in range(2)]  # the mesh alternates between two poses
    d_moves = [ctx.to_device(m) for m in moves]
    rays = ctx.to_device(sphere_rays(NRAYS))
    hit = ctx.empty((NRAYS,), capi.HIT_DTYPE)
    out = {"workload": name, "faces": int(T), "repeats": repeats}
    try:
        load(ctx, mesh, mesh[0])
        out["accel_info"] = ctx.build_ray_accel(device=True)
        lo, hi = box(np.concatenate([mesh[0]] + moves))  # one box for every pose (no descriptor upload in (b), (c))
        ctx.update_object(0, bbox=(lo, hi))
        ctx.cast_rays_device(rays.ptr, 1024, out_hit=hit.ptr)
        ctx.synchronize()
        step = [0]

        def reset_add_build():
            k = step[0] % 2
            ctx.scene_reset()
            ctx.set_camera(capi.make_camera((0.0, 0.0, 5.0), (60.0, 60.0), 64, 1.0))
            ctx.add_object(moves[k], mesh[1], mesh[2], lo, hi)
            for position, variant, brightness in LIGHTS:
                ctx.add_light(capi.make_light(position, variant, brightness=brightness))
            ctx.build_ray_accel(device=True)

        def update(k):
            ctx.update_object_device(0, d_moves[k].ptr, None, None, T)

        def update_refit():
            update(step[0] % 2)
            return ctx.refit_ray_accel()

        def update_build():
            update(step[0] % 2)
            return ctx.build_ray_accel(device=True)

        def update_only():
            update(step[0] % 2)

        forms = {"a_reset_add_build": reset_add_build, "b_update_refit": update_refit, "c_update_build": update_build,
                 "update_only": update_only}
        times = {k: [] for k in forms}
        stats = {"refit_ms": [], "build_ms": []}
        for rep in range(repeats + WARMUP):
            for k, fn in forms.items():  # ((b) follows (a): the refit finds a device-built tree of the same object)
                step[0] += 1
                ms, info = wall(ctx, fn)
                if k == "b_update_refit" and not (info["rebuilt"] == 0 and info["refitted"] == 1):
                    raise AssertionError(f"{name}: the refit did not keep the topology: {info}")
                if rep < WARMUP:
                    continue
                times[k].append(ms)
                if k == "b_update_refit":
                    stats["refit_ms"].append(info["build_ms"])
                elif k == "c_update_build":
                    stats["build_ms"].append(info["build_ms"])
        out.update({k: summary(v) for k, v in times.items()})
        out["refit_call_ms"] = summary(stats["refit_ms"])  # the calls' own build_ms (entry to the final synchronisation)
        out["build_call_ms"] = summary(stats["build_ms"])
        out["c_over_b"] = round(out["c_update_build"]["median_ms"] / out["b_update_refit"]["median_ms"], 3)
        out["a_over_b"] = round(out["a_reset_add_build"]["median_ms"] / out["b_update_refit"]["median_ms"], 3)
        out["build_over_refit_call"] = round(out["build_call_ms"]["median_ms"] / out["refit_call_ms"]["median_ms"], 3)

        # (d) query cost after a displacement: the old split refitted against a fresh build
        out["query"] = {}
        for frac in (0.01, 0.05, 0.20):
            pos = displaced(mesh[0], frac)
            d_pos = ctx.to_device(pos)
            try:
                load(ctx, mesh, mesh[0])
                ctx.build_ray_accel(device=True)
                ctx.update_object(0, positions=d_pos, bbox=box(pos))
                info = ctx.refit_ray_accel()
                kept = info["rebuilt"] == 0
                q = {"refit_kept_topology": bool(kept), "unculled_faces": int(info["unculled_faces"])}
                records = {}
                for form in ("refitted", "rebuilt"):
                    if form == "rebuilt":
                        ctx.build_ray_accel(device=True)
                    ms = []
                    for rep in range(repeats + WARMUP):
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record(stream)
                        ctx.cast_rays_device(rays.ptr, NRAYS, out_hit=hit.ptr, flags=capi.RAYS_NORMALIZE)
                        t1.record(stream)
                        t1.synchronize()
                        if rep >= WARMUP:
                            ms.append(t0.elapsed_time(t1))
                    q[form] = summary(ms)
                    records[form] = hit.numpy().tobytes()
                if records["refitted"] != records["rebuilt"]:
                    raise AssertionError(f"{name}, {frac}: the refitted tree's records differ from the rebuilt tree's")
                q["refitted_over_rebuilt"] = round(q["refitted"]["median_ms"] / q["rebuilt"]["median_ms"], 3)
                out["query"][f"{frac:.2f}"] = q
            finally:
                d_pos.free()
        return out
    finally:
        for a in (*d_moves, rays, hit):
            a.free()
        ctx.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--no-1m", action="store_true", help="skip the 1M-face mesh")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays", "rays_update_bench.json"))
    a = ap.parse_args()
    lines = [bench_mesh("69451 faces", generated_mesh(**meshgen.STANDIN_70K), a.repeats)]
    print(json.dumps(lines[-1]), flush=True)
    if not a.no_1m:
        lines.append(bench_mesh("1M faces", generated_mesh(**meshgen.SYNTH_1M), a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rays": NRAYS, "results": lines}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
