"""The frame loop "move the mesh, refit the hierarchy, ask 2^20 rays" by direct calls and as one graph
replay (one GPU, one process; needs an MI355X).

    python scripts/rays_refit_graph_bench.py [--repeats 20] [--no-1m] [--out profiles/rays/rays_refit_graph_bench.json]

Per mesh (the 69,451-face stand-in and the 1M-face sphere, one box for every pose, two point lights
and one ambient light), with the moved positions resident and the hierarchy device-built, the wall
time between two stream synchronisations of one frame, the mesh alternating between two poses:

  (a) direct              eray_scene_update_object (device pointers) + eray_scene_refit_ray_accel +
                          eray_cast_rays of 2^20 incoherent rays, by direct calls
  (b) graph               update + eray_scene_refit_ray_accel_async + the same rays, one graph replay
  (c) graph_per_level     (b) captured with the upper levels NOT in one launch
                          (eray_debug_set_refit_top_levels(0)): what refit_top_levels_kernel buys
  (d) update + refit alone, without the rays: direct with the synchronous refit, direct with the
      async refit, and as a graph replay (with and without the one-launch kernel)

All in the same process, alternating the forms round by round: 3 untimed warm-up rounds, then
`repeats` rounds (at least 20); medians and the min..max spread.  After the clocks: per pose the hit
records of (a), (b) and (c) are compared byte for byte, and the hierarchy's four arrays after (b) and
(c) against those after (a)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from eray_amd import capi, meshgen  # noqa: E402
from rays_update_bench import NRAYS, box, displaced, generated_mesh, load, sphere_rays, summary  # noqa: E402

WARMUP = 3


def bench_mesh(name: str, mesh, repeats: int) -> dict:
    stream = torch.cuda.Stream()
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    T = mesh[0].shape[0]
    moves = [displaced(mesh[0], 0.01 * (1 + k)) for k in range(2)]
    d_moves = [ctx.to_device(m) for m in moves]
    rays = ctx.to_device(sphere_rays(NRAYS))
    hit = ctx.empty((NRAYS,), capi.HIT_DTYPE)
    out = {"workload": name, "faces": int(T), "rays": NRAYS, "repeats": repeats, "warmup": WARMUP}
    try:
        load(ctx, mesh, mesh[0])
        out["accel_info"] = ctx.build_ray_accel(device=True)
        ctx.update_object(0, bbox=box(np.concatenate([mesh[0]] + moves)))  # one box for every pose
        ctx.cast_rays_device(rays.ptr, 1024, out_hit=hit.ptr)
        ctx.synchronize()

        def update(k):
            ctx.update_object_device(0, d_moves[k].ptr, None, None, T)

        def cast():
            ctx.cast_rays_device(rays.ptr, NRAYS, out_hit=hit.ptr, flags=capi.RAYS_NORMALIZE)

        def captured(k, top, with_rays):
            ctx.set_refit_top_levels(top)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                update(k)
                ctx.refit_ray_accel_async()
                if with_rays:
                    cast()
            ctx.set_refit_top_levels(True)
            return g

        update(0)
        ctx.refit_ray_accel_async()  # (outside a capture: the workspace)
        ctx.synchronize()
        out["workspace_bytes"] = ctx.refit_status()["workspace_bytes"]
        graphs = {(top, with_rays): [captured(k, top, with_rays) for k in range(2)]
                  for top in (True, False) for with_rays in (True, False)}

        def replay(top, with_rays):
            def run(k):
                with torch.cuda.stream(stream):
                    graphs[(top, with_rays)][k].replay()
            return run

        def direct(k):
            update(k)
            info = ctx.refit_ray_accel()
            cast()
            return info

        def direct_refit(k):
            update(k)
            return ctx.refit_ray_accel()

        def direct_async(k):
            update(k)
            ctx.refit_ray_accel_async()

        forms = {"a_direct": direct, "b_graph": replay(True, True), "c_graph_per_level": replay(False, True),
                 "d_direct_update_refit": direct_refit, "d_direct_update_refit_async": direct_async,
                 "d_graph_update_refit": replay(True, False), "d_graph_update_refit_per_level": replay(False, False)}
        times = {k: [] for k in forms}
        for rep in range(repeats + WARMUP):
            for name_, fn in forms.items():
                ctx.synchronize()
                t0 = time.perf_counter()
                info = fn(rep % 2)
                ctx.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                if info is not None and not (info["rebuilt"] == 0 and info["refitted"] == 1):
                    raise AssertionError(f"{name}: the synchronous refit did not keep the topology: {info}")
                if rep >= WARMUP:
                    times[name_].append(ms)
        out.update({k: summary(v) for k, v in times.items()})
        st = ctx.refit_status()
        if st["fell_back"] or st["kept"] != st["covered"]:
            raise AssertionError(f"{name}: an object fell back: {st}")
        out["refit_status"] = st
        a, b, c = (out[k]["median_ms"] for k in ("a_direct", "b_graph", "c_graph_per_level"))
        out["a_over_b"] = round(a / b, 3)
        out["c_over_b"] = round(c / b, 3)
        out["d_direct_over_graph"] = round(out["d_direct_update_refit"]["median_ms"] / out["d_graph_update_refit"]["median_ms"], 3)

        # every form yields the same bytes
        for k in range(2):
            seen = {}
            for name_ in ("a_direct", "b_graph", "c_graph_per_level"):
                ctx.memset(hit.ptr, 0xFF, hit.nbytes)
                forms[name_](k)
                ctx.synchronize()
                seen[name_] = (hit.numpy().tobytes(), ctx.ray_accel_arrays())
            for name_ in ("b_graph", "c_graph_per_level"):
                if seen[name_] != seen["a_direct"]:
                    raise AssertionError(f"{name}, pose {k}: {name_} differs from the direct sequence")
        out["same_bytes"] = True
        return out
    finally:
        for x in (*d_moves, rays, hit):
            x.free()
        ctx.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-1m", action="store_true", help="skip the 1M-face mesh")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays", "rays_refit_graph_bench.json"))
    a = ap.parse_args()
    repeats = max(a.repeats, 20)
    lines = [bench_mesh("69451 faces", generated_mesh(**meshgen.STANDIN_70K), repeats)]
    print(json.dumps(lines[-1]), flush=True)
    if not a.no_1m:
        lines.append(bench_mesh("1M faces", generated_mesh(**meshgen.SYNTH_1M), repeats))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rays": NRAYS, "results": lines}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
