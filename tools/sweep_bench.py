"""Throughput of the batched swept-sphere queries (tyr_query_sweep) on C3's scene, next to tyr_query_closest as a yardstick.

C3's scene (scenes.mesh_scene(), 996,882 triangles) and 2 Mi sweeps: the origins are tools/nearest_bench.py's "surface" batch
(within 0.5 of the surface, drawn from the same seed), each with a seeded displacement of up to 3 units per axis -- particles
near a mesh moved by one step.  Radii 0, 0.1 and 1 (one radius per launch), and the batch in two orders: shuffled (as drawn) and
sorted by the Morton code of the origins.  The yardstick, tyr_query_closest on the same origins and directions in the same
process, is context, not a gate: a ray does binary32 work on fewer boxes.  The launches run in turn, REPS rounds after two
warm-up rounds, each timed with device events around its launch on a stream of their own: median and p10-p90 per launch, sweeps
per second, and the share of the sweeps that touch the mesh (and of those, that start in overlap).

    python tools/sweep_bench.py [--reps 10] [--out profiles/sweep_bench_c3.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime in the process, see tests/conftest.py)

import numpy as np  # noqa: E402

from query_bench_common import c3_points, morton_order, stats, timed_rounds  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402

N = 1 << 21
RADII = (0.0, 0.1, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    nodes, prims, _ = g.build_upload(sc.triangles)
    surface = c3_points(nodes, prims, N)["surface"]
    disp = np.random.default_rng(2026).uniform(-3.0, 3.0, (N, 3)).astype(np.float32)
    lo, hi = nodes[0]["bounds"][0].astype(np.float32), nodes[0]["bounds"][1].astype(np.float32)
    order = morton_order(np.clip((surface - lo) / (hi - lo) * 1023.0, 0, 1023))

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    batches = {"shuffled": (on(surface), on(disp)), "morton": (on(surface[order]), on(disp[order]))}
    radius = {r: torch.full((N,), r, dtype=torch.float32, device=dev) for r in RADII}
    t, prim, region = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
    point, center, normal = (torch.empty((N, 3), dtype=torch.float32, device=dev) for _ in range(3))
    rt, rprim, rgeom = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    out = binding.SweepOut(t.data_ptr(), prim.data_ptr(), region.data_ptr(), point.data_ptr(), center.data_ptr(), normal.data_ptr())
    L = g.L

    launches = {}
    for name, (o, d) in batches.items():
        for r in RADII:
            launches[f"sweep_{name}_r{r:g}"] = lambda o=o, d=d, r=r: L.tyr_query_sweep(g.h, N, o.data_ptr(), d.data_ptr(), radius[r].data_ptr(), None, 0, C.byref(out), h)
        launches[f"closest_{name}"] = lambda o=o, d=d: L.tyr_query_closest(g.h, N, o.data_ptr(), d.data_ptr(), None, 0, rt.data_ptr(), rprim.data_ptr(), rgeom.data_ptr(), None, h)
    found = {}

    def read_found(name, rep):
        if rep == 0 and name.startswith("sweep_"):
            found[name] = {"hit_share": float((prim >= 0).float().mean().item()), "overlap_share_of_hits": float(((prim >= 0) & (t == 0)).sum().item() / max(int((prim >= 0).sum().item()), 1))}

    samples = timed_rounds(g, launches, stream, args.reps, after=read_found)
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "items": N,
              "displacement": "uniform in [-3, 3] per axis", "batches": {k: stats(v, N) for k, v in samples.items()}, "found": found,
              "kernel_time": "not measured here: event times around each launch"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["mitems_s"], 1) for k, v in result["batches"].items()}))
    print(json.dumps(found))


if __name__ == "__main__":
    main()
