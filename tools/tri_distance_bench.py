"""Throughput of the batched closest-triangle distance queries (tyr_query_tri_distance) on C3's scene, next to the three-call
workaround it replaces.

C3's scene (scenes.mesh_scene(), 996,882 triangles, mean triangle edge 0.35) and 1 Mi query triangles: a is the first Mi points
of tools/nearest_bench.py's "surface" batch (within 0.5 of the surface, drawn from the same seed), b and c = a + a seeded
direction each times the size -- 1, 4 and 16 mean triangle edges.  Each size without a bound and with max_dist = 0.1, in two
orders: shuffled (as drawn) and sorted by the Morton code of a.  Beside them the self-proximity pass: the mesh's own triangles as
queries with TYR_QUERY_TRI_SKIP_SHARED and max_dist = 0.1.  Context, in the same rounds, not a gate (the query has no
predecessor): the workaround -- three tyr_query_segment calls on the edges of the 4-edge triangles, unbounded, and a min over
their dist2 on the device -- with its summed time and the share of queries whose best dist2 of the three lies above the new
call's by more than 1e-4 (what the edges miss: a mesh vertex facing the interior, a mesh edge through it).  The launches run in
turn, REPS rounds after two warm-up rounds, each timed with device events around its launch on a stream of their own: median and
p10-p90 per launch, queries per second, and the share of the queries that touch the mesh (dist2 = 0) and that answer "none".

    python tools/tri_distance_bench.py [--reps 10] [--out profiles/tri_distance_bench_c3.json]
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
SIZES = (("small", 1), ("medium", 4), ("large", 16))
RADIUS = 0.1
SKIP_SHARED = binding.TYR_QUERY_TRI_SKIP_SHARED


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_distance_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    nodes, prims, _ = g.build_upload(sc.triangles)
    surface = c3_points(nodes, prims, 1 << 21)["surface"][:N]
    rng = np.random.default_rng(2029)
    units = []
    for _ in range(2):
        u = rng.normal(size=(N, 3))
        units.append(u / np.linalg.norm(u, axis=1, keepdims=True))
    lo, hi = nodes[0]["bounds"][0].astype(np.float32), nodes[0]["bounds"][1].astype(np.float32)
    orders = {"shuffled": np.arange(N), "morton": morton_order(np.clip((surface - lo) / (hi - lo) * 1023.0, 0, 1023))}

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)  # noqa: E731
    corners = {edges: tuple((surface + u * (edges * EDGE)).astype(np.float32) for u in units) for _, edges in SIZES}
    a = {name: on(surface[order]) for name, order in orders.items()}
    bc = {(name, edges): tuple(on(x[order]) for x in corners[edges]) for name, order in orders.items() for _, edges in SIZES}
    vert, e1, e2 = (np.ascontiguousarray(prims[k], np.float32).reshape(-1, 3) for k in ("vert", "e1", "e2"))
    own = (on(vert), on((vert + e1).astype(np.float32)), on((vert + e2).astype(np.float32)))
    M = len(vert)
    big = max(N, M)
    bound = torch.full((big,), RADIUS, dtype=torch.float32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)  # noqa: E731
    dist2, prim = f32(big), torch.empty(big, dtype=torch.int32, device=dev)
    feature, region, on_query, on_triangle = u8(big), u8(big), f32(big, 3), f32(big, 3)
    out = binding.TriDistanceOut(*(x.data_ptr() for x in (dist2, prim, feature, region, on_query, on_triangle)))
    sd2 = [f32(N) for _ in range(3)]
    sprim = torch.empty(N, dtype=torch.int32, device=dev)
    souts = [binding.SegmentOut(d.data_ptr(), sprim.data_ptr(), None, None, None, None, None) for d in sd2]
    L = g.L

    launches = {}
    for name in orders:
        for case, edges in SIZES:
            for r in (None, RADIUS):
                launches[f"tri_distance_{name}_{case}" + ("" if r is None else f"_r{r}")] = lambda p0=a[name], p12=bc[(name, edges)], r=r: L.tyr_query_tri_distance(
                    g.h, N, p0.data_ptr(), p12[0].data_ptr(), p12[1].data_ptr(), bound.data_ptr() if r is not None else None, 0, C.byref(out), h)
    launches[f"tri_distance_self_skip_shared_r{RADIUS}"] = lambda: L.tyr_query_tri_distance(
        g.h, M, own[0].data_ptr(), own[1].data_ptr(), own[2].data_ptr(), bound.data_ptr(), SKIP_SHARED, C.byref(out), h)
    p0, (p1, p2) = a["shuffled"], bc[("shuffled", 4)]
    for k, (x, y) in enumerate(((p0, p1), (p1, p2), (p2, p0))):
        launches[f"segment_shuffled_medium_edge{k}"] = lambda x=x, y=y, k=k: L.tyr_query_segment(g.h, N, x.data_ptr(), y.data_ptr(), None, 0, C.byref(souts[k]), h)
    best3 = f32(N)

    def host_min():
        torch.minimum(torch.minimum(sd2[0], sd2[1]), sd2[2], out=best3)
        return 0

    launches["segment_shuffled_medium_min_of_three"] = host_min
    found, kept = {}, {}

    def read_found(name, rep):
        if rep != 0:
            return
        if name.startswith("tri_distance_"):
            n = M if "self" in name else N
            found[name] = {"touching_share": float(((prim[:n] >= 0) & (dist2[:n] == 0)).float().mean().item()), "none_share": float((prim[:n] < 0).float().mean().item())}
            if name == "tri_distance_shuffled_medium":
                kept["dist2"] = dist2[:N].clone()
        elif name == "segment_shuffled_medium_min_of_three":
            found[name] = {"share_of_queries_where_the_edges_best_dist2_exceeds_the_querys": float((best3 > kept["dist2"]).float().mean().item()),
                           "share_where_it_exceeds_it_by_more_than_1e-4": float((best3 > kept["dist2"] + 1e-4).float().mean().item())}

    with torch.cuda.stream(stream):
        times = timed_rounds(g, launches, stream, args.reps, after=read_found)
    items = lambda k: M if "self" in k else N  # noqa: E731
    batches = {k: stats(v, items(k)) for k, v in times.items()}
    three = [batches[f"segment_shuffled_medium_edge{k}"]["median_ms"] for k in range(3)] + [batches["segment_shuffled_medium_min_of_three"]["median_ms"]]
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "items": N, "self_items": M,
              "sizes": {case: f"{edges} x {EDGE}" for case, edges in SIZES}, "max_dist": RADIUS, "batches": batches,
              "workaround_three_segment_calls_and_min_median_ms": float(sum(three)), "found": found,
              "kernel_time": "not measured here: event times around each launch", "tuned": "nothing: launch bounds and slack as first written"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["median_ms"], 3) for k, v in result["batches"].items()}))
    print(json.dumps({"workaround_ms": result["workaround_three_segment_calls_and_min_median_ms"]}))
    print(json.dumps(found))


if __name__ == "__main__":
    main()
