"""What a refit of a HOST-built ray-query hierarchy costs and keeps, beside the device-built one (one
GPU, one process; needs an MI355X).

    python scripts/rays_refit_host_bench.py [--repeats 15] [--no-1m] [--out profiles/rays/rays_refit_host_bench.json]

Per mesh (the 69,451-face stand-in and the 1M-face sphere, one box for every pose, two point lights
and one ambient light) two contexts hold the same scene, one with the hierarchy of
eray_scene_build_ray_accel_refittable (the host's widest-axis median split, nodes in recursion
order), one with that of eray_scene_build_ray_accel_device (the middle of the Morton order, nodes
level by level).  The moved positions are resident; the mesh alternates between two poses.

  (a) refit cost: the wall time between two stream synchronisations of
        sync_host / sync_device     eray_scene_update_object (device pointers) + eray_scene_refit_ray_accel
        graph_host / graph_device   update + eray_scene_refit_ray_accel_async as one graph replay
        graph_host_per_level / graph_device_per_level   the same captured with a launch per level
      and the ratios host / device.  In recursion order a level's node and bounds stores scatter.
  (b) query cost: 2^20 incoherent rays (radius-3 sphere toward [-1, 1]^3) after a smooth displacement
      of 1 %, 5 % and 20 % of the mesh radius through the refitted host tree, a fresh host build of the
      displaced mesh, the refitted device tree and a fresh device build; device-event times of the one
      kernel; the records compared byte for byte outside the clock.

Two untimed warm-up rounds, then `repeats` rounds alternating the forms; medians and the min..max
spread; what a form returns is looked at after its clock has stopped."""
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
from rays_update_bench import NRAYS, WARMUP, box, displaced, generated_mesh, load, sphere_rays, summary  # noqa: E402

BUILDERS = {"host": {"refittable": True}, "device": {"device": True}}


class Side:
    """One context on its own stream with the scene and one builder's hierarchy."""

    def __init__(self, which, mesh, moves):
        self.which = which
        self.stream = torch.cuda.Stream()
        self.ctx = ctx = capi.Context(0)
        ctx.set_stream(self.stream.cuda_stream)
        self.T = mesh[0].shape[0]
        self.d_moves = [ctx.to_device(m) for m in moves]
        self.rays = ctx.to_device(sphere_rays(NRAYS))
        self.hit = ctx.empty((NRAYS,), capi.HIT_DTYPE)
        self.held = [*self.d_moves, self.rays, self.hit]

    def build(self):
        return self.ctx.build_ray_accel(**BUILDERS[self.which])

    def update(self, k):
        self.ctx.update_object_device(0, self.d_moves[k].ptr, None, None, self.T)

    def captured(self, k, top):
        self.ctx.set_refit_top_levels(top)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.stream):
            self.update(k)
            self.ctx.refit_ray_accel_async()
        self.ctx.set_refit_top_levels(True)
        return g

    def query_ms(self, repeats):
        ms = []
        for rep in range(repeats + WARMUP):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(self.stream)
            self.ctx.cast_rays_device(self.rays.ptr, NRAYS, out_hit=self.hit.ptr, flags=capi.RAYS_NORMALIZE)
            t1.record(self.stream)
            t1.synchronize()
            if rep >= WARMUP:
                ms.append(t0.elapsed_time(t1))
        return summary(ms), self.hit.numpy().tobytes()

    def close(self):
        for a in self.held:
            a.free()
        self.ctx.close()


def bench_mesh(name: str, mesh, repeats: int) -> dict:
    moves = [displaced(mesh[0], 0.01 * (1 + k)) for k in range(2)]
    sides = {w: Side(w, mesh, moves) for w in BUILDERS}
    out = {"workload": name, "faces": int(mesh[0].shape[0]), "rays": NRAYS, "repeats": repeats, "warmup": WARMUP}
    try:
        # ---- (a) refit cost
        graphs = {}
        for w, s in sides.items():
            load(s.ctx, mesh, mesh[0])
            out[f"accel_info_{w}"] = s.build()
            s.ctx.update_object(0, bbox=box(np.concatenate([mesh[0]] + moves)))  # one box for every pose
            s.ctx.cast_rays_device(s.rays.ptr, 1024, out_hit=s.hit.ptr)
            s.update(0)
            s.ctx.refit_ray_accel_async()  # (outside a capture: the workspace)
            s.ctx.synchronize()
            for top in (True, False):
                graphs[(w, top)] = [s.captured(k, top) for k in range(2)]

        def sync_refit(s):
            def run(k):
                s.update(k)
                return s.ctx.refit_ray_accel()
            return run

        def replay(s, gs):
            def run(k):
                with torch.cuda.stream(s.stream):
                    gs[k].replay()
            return run

        forms = {}
        for w, s in sides.items():
            forms[f"sync_{w}"] = (s, sync_refit(s))
            forms[f"graph_{w}"] = (s, replay(s, graphs[(w, True)]))
            forms[f"graph_{w}_per_level"] = (s, replay(s, graphs[(w, False)]))
        times = {k: [] for k in forms}
        for rep in range(repeats + WARMUP):
            for k, (s, fn) in forms.items():
                s.ctx.synchronize()
                t0 = time.perf_counter()
                info = fn(rep % 2)
                s.ctx.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                if info is not None and not (info["rebuilt"] == 0 and info["refitted"] == 1):
                    raise AssertionError(f"{name}, {k}: the refit did not keep the topology: {info}")
                if rep >= WARMUP:
                    times[k].append(ms)
        out["refit"] = {k: summary(v) for k, v in times.items()}
        for form in ("sync", "graph"):
            out["refit"][f"{form}_host_over_device"] = round(
                out["refit"][f"{form}_host"]["median_ms"] / out["refit"][f"{form}_device"]["median_ms"], 3)
        out["refit"]["graph_per_level_host_over_device"] = round(
            out["refit"]["graph_host_per_level"]["median_ms"] / out["refit"]["graph_device_per_level"]["median_ms"], 3)
        for w, s in sides.items():
            st = s.ctx.refit_status()
            if st["fell_back"] or st["kept"] != st["covered"]:
                raise AssertionError(f"{name}, {w}: an object fell back: {st}")
            out[f"refit_status_{w}"] = st
        # the graph's refit leaves the bytes of the synchronous one (outside the clock)
        for w, s in sides.items():
            for k in range(2):
                forms[f"sync_{w}"][1](k)
                want = s.ctx.ray_accel_arrays()
                for form in (f"graph_{w}", f"graph_{w}_per_level"):
                    forms[form][1](k)
                    s.ctx.synchronize()
                    if s.ctx.ray_accel_arrays() != want:
                        raise AssertionError(f"{name}, pose {k}: {form} leaves other bytes than the synchronous refit")
        out["same_bytes"] = True
        del graphs, forms  # (the builds below release the workspaces the graphs captured)

        # ---- (b) query cost after a displacement
        out["query"] = {}
        for frac in (0.01, 0.05, 0.20):
            pos = displaced(mesh[0], frac)
            q, records = {}, {}
            for w, s in sides.items():
                d_pos = s.ctx.to_device(pos)
                try:
                    load(s.ctx, mesh, mesh[0])
                    s.build()
                    s.ctx.update_object(0, positions=d_pos, bbox=box(pos))
                    info = s.ctx.refit_ray_accel()
                    q[f"{w}_refit_kept_topology"] = bool(info["rebuilt"] == 0)
                    q[f"refitted_{w}"], records[f"refitted_{w}"] = s.query_ms(repeats)
                    if w == "host":
                        s.ctx.build_ray_accel()
                    else:
                        s.ctx.build_ray_accel(device=True)
                    q[f"fresh_{w}"], records[f"fresh_{w}"] = s.query_ms(repeats)
                finally:
                    d_pos.free()
            if len(set(records.values())) != 1:
                raise AssertionError(f"{name}, {frac}: the four trees' records differ")
            m = {k: q[k]["median_ms"] for k in records}
            q["refitted_host_over_fresh_host"] = round(m["refitted_host"] / m["fresh_host"], 3)
            q["refitted_device_over_fresh_device"] = round(m["refitted_device"] / m["fresh_device"], 3)
            q["refitted_device_over_refitted_host"] = round(m["refitted_device"] / m["refitted_host"], 3)
            q["fresh_device_over_fresh_host"] = round(m["fresh_device"] / m["fresh_host"], 3)
            out["query"][f"{frac:.2f}"] = q
        return out
    finally:
        for s in sides.values():
            s.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--no-1m", action="store_true", help="skip the 1M-face mesh")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays", "rays_refit_host_bench.json"))
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
