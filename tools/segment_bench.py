"""Throughput of the batched closest-segment queries (tyr_query_segment) on C3's scene, next to tyr_query_nearest as context.

C3's scene (scenes.mesh_scene(), 996,882 triangles, mean triangle edge 0.35) and 1 Mi segments: p is the first Mi points of
tools/nearest_bench.py's "surface" batch (within 0.5 of the surface, drawn from the same seed), q = p + a seeded direction times
the length -- 1, 4 and 16 mean triangle edges without a bound, and 4 edges with max_dist = 0.1 (a capsule of that radius).  Each
in two orders: shuffled (as drawn) and sorted by the Morton code of p.  Context, in the same rounds, not a gate (the query has no
predecessor): tyr_query_nearest on p and on the 4-edge q, and the workaround the query replaces -- tyr_query_nearest on 8 evenly
spaced samples of every 4-edge segment (8 Mi points), with the share of segments where the best of the 8 answers lies above the
query's dist2 (what sampling misses).  The sorted batch is the slower one; two more orders of the 4-edge batch show at which
scale: the Morton order cut into blocks of 64 and of 1024 consecutive segments, the blocks shuffled.  The launches run in turn,
REPS rounds after two warm-up rounds, each timed with device events around its launch on a stream of their own: median and
p10-p90 per launch, segments per second, and the share of the segments that touch the mesh (dist2 = 0) and that answer "none".

    python tools/segment_bench.py [--reps 10] [--out profiles/segment_bench_c3.json]
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

N = 1 << 20
EDGE = 0.35
CASES = (("short", 1, None), ("medium", 4, None), ("long", 16, None), ("medium_r0.1", 4, 0.1))
SAMPLES = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    nodes, prims, _ = g.build_upload(sc.triangles)
    surface = c3_points(nodes, prims, 1 << 21)["surface"][:N]
    unit = np.random.default_rng(2027).normal(size=(N, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    lo, hi = nodes[0]["bounds"][0].astype(np.float32), nodes[0]["bounds"][1].astype(np.float32)
    orders = {"shuffled": np.arange(N), "morton": morton_order(np.clip((surface - lo) / (hi - lo) * 1023.0, 0, 1023))}

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    ends = {edges: (surface + unit * (edges * EDGE)).astype(np.float32) for edges in (1, 4, 16)}
    p = {name: on(surface[order]) for name, order in orders.items()}
    q = {(name, edges): on(ends[edges][order]) for name, order in orders.items() for edges in ends}
    bound = torch.full((N,), 0.1, dtype=torch.float32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    dist2, prim = f32(N), torch.empty(N, dtype=torch.int32, device=dev)
    s, feature, region = f32(N), torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
    on_segment, on_triangle = f32(N, 3), f32(N, 3)
    out = binding.SegmentOut(*(a.data_ptr() for a in (dist2, prim, s, feature, region, on_segment, on_triangle)))
    nd2, nprim = f32(SAMPLES * N), torch.empty(SAMPLES * N, dtype=torch.int32, device=dev)
    nout = binding.NearestOut(nd2.data_ptr(), nprim.data_ptr(), None, None, None)
    w = torch.linspace(0.0, 1.0, SAMPLES, device=dev)[None, :, None]
    samples = (p["shuffled"][:, None, :] * (1 - w) + q[("shuffled", 4)][:, None, :] * w).reshape(-1, 3).contiguous()
    L = g.L

    launches = {}
    for name in orders:
        for case, edges, r in CASES:
            launches[f"segment_{name}_{case}"] = lambda a=p[name], b=q[(name, edges)], r=r: L.tyr_query_segment(
                g.h, N, a.data_ptr(), b.data_ptr(), bound.data_ptr() if r is not None else None, 0, C.byref(out), h)
        launches[f"nearest_{name}_p"] = lambda a=p[name]: L.tyr_query_nearest(g.h, N, a.data_ptr(), None, 0, C.byref(nout), h)
        launches[f"nearest_{name}_q_medium"] = lambda b=q[(name, 4)]: L.tyr_query_nearest(g.h, N, b.data_ptr(), None, 0, C.byref(nout), h)
    rng = np.random.default_rng(2028)
    for block in (64, 1024):  # coherent within a block of consecutive segments, the blocks in random order
        order = orders["morton"].reshape(-1, block)[rng.permutation(N // block)].reshape(-1)
        launches[f"segment_morton_blocks{block}_medium"] = lambda a=on(surface[order]), b=on(ends[4][order]): L.tyr_query_segment(
            g.h, N, a.data_ptr(), b.data_ptr(), None, 0, C.byref(out), h)
    launches["nearest_shuffled_8_samples_medium"] = lambda: L.tyr_query_nearest(g.h, SAMPLES * N, samples.data_ptr(), None, 0, C.byref(nout), h)
    found, kept = {}, {}

    def read_found(name, rep):
        if rep != 0:
            return
        if name.startswith("segment_"):
            found[name] = {"touching_share": float(((prim >= 0) & (dist2 == 0)).float().mean().item()), "none_share": float((prim < 0).float().mean().item())}
            if name == "segment_shuffled_medium":
                kept["dist2"] = dist2.clone()
        elif name == "nearest_shuffled_8_samples_medium":
            best = nd2.reshape(N, SAMPLES).min(dim=1).values
            found[name] = {"share_of_segments_where_the_samples_best_dist2_exceeds_the_querys": float((best > kept["dist2"]).float().mean().item()),
                           "share_where_it_exceeds_it_by_more_than_1e-4": float((best > kept["dist2"] + 1e-4).float().mean().item())}

    times = timed_rounds(g, launches, stream, args.reps, after=read_found)
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "items": N,
              "lengths": {case: f"{edges} x {EDGE}" + ("" if r is None else f", max_dist {r}") for case, edges, r in CASES},
              "batches": {k: stats(v, SAMPLES * N if "8_samples" in k else N) for k, v in times.items()}, "found": found,
              "kernel_time": "not measured here: event times around each launch", "tuned": "nothing: launch bounds and slack as first written"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["median_ms"], 3) for k, v in result["batches"].items()}))
    print(json.dumps(found))


if __name__ == "__main__":
    main()
