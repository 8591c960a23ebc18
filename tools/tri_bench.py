"""Throughput of the batched triangle-overlap queries (tyr_query_tri) on C3's scene, next to the broadphase a caller would
otherwise run before filtering on the host: tyr_query_box on the query triangles' bounding boxes.

C3's scene (scenes.mesh_scene(), 996,882 triangles) and 1 Mi seeded query triangles whose centres are tools/nearest_bench.py's
"surface" batch (within 0.5 of the surface, drawn from the same seed), every corner uniform in a cube round the centre sized so
that the triangle's edges average 1 and 4 mean edges of the mesh; the batch in two orders, shuffled (as drawn) and sorted by the
Morton code of the centres; three variants per size and order: `any` (TYR_QUERY_TRI_ANY), a count alone (max_prims 0) and
max_prims 16.  Then the mesh's own triangles, in build order, with TYR_QUERY_TRI_SKIP_SHARED -- the self-intersection check --
as `any` and as a count, and as a count without the flag (every triangle then finds itself and its neighbours).  Beside them
tyr_query_box with a count on the bounding boxes of the same query triangles: it over-reports, its time is a floor and not a
target.  The launches run in turn, REPS rounds after two warm-up rounds, each timed with device events around its launch on a
stream of their own: median and p10-p90 per launch, queries per second, the members per query, the share of queries that touch
anything, and tri over box as a ratio of medians.

    python tools/tri_bench.py [--reps 10] [--out profiles/tri_bench_c3.json]
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
EDGES = (1, 4)  # the query triangles' mean edge, in mean triangle edges of the mesh
K = 16
F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    nodes, prims, _ = g.build_upload(sc.triangles)
    centres = c3_points(nodes, prims, N)["surface"]
    mean_edge = float(np.linalg.norm(np.concatenate([prims["e1"], prims["e2"], prims["e2"] - prims["e1"]]).astype(np.float64), axis=1).mean())
    lo, hi = nodes[0]["bounds"][0].astype(F), nodes[0]["bounds"][1].astype(F)
    order = morton_order(np.clip((centres - lo) / (hi - lo) * 1023.0, 0, 1023))
    rng = np.random.default_rng(2026)
    unit = [rng.uniform(-1, 1, (N, 3)) for _ in range(3)]  # two uniform points of a cube of side L are 0.66 L apart on average

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    M = max(N, len(prims))
    count = torch.empty(M, dtype=torch.int32, device=dev)
    prim = torch.empty((N, K), dtype=torch.int32, device=dev)
    out = binding.TriOut(count.data_ptr(), prim.data_ptr())
    bout = binding.BoxOut(count.data_ptr(), prim.data_ptr())
    L = g.L
    ANY, SKIP = binding.TYR_QUERY_TRI_ANY, binding.TYR_QUERY_TRI_SKIP_SHARED

    def tri(n, a, b, c, k, flags):
        return lambda: L.tyr_query_tri(g.h, n, a.data_ptr(), b.data_ptr(), c.data_ptr(), k, flags, C.byref(out), h)

    launches, keep, sizes, query_edges = {}, [], {}, {}
    for m in EDGES:
        half = 0.5 * m * mean_edge / 0.66
        abc = [(centres + u * half).astype(F) for u in unit]
        query_edges[f"edge{m}"] = float(np.mean([np.linalg.norm((abc[i] - abc[(i + 1) % 3]).astype(np.float64), axis=1).mean() for i in range(3)]))
        for name, idx in (("shuffled", slice(None)), ("morton", order)):
            a, b, c = (on(x[idx]) for x in abc)
            blo, bhi = on(np.minimum(np.minimum(abc[0], abc[1]), abc[2])[idx]), on(np.maximum(np.maximum(abc[0], abc[1]), abc[2])[idx])
            keep += [a, b, c, blo, bhi]
            tag = f"{name}_edge{m}"
            launches[f"tri_any_{tag}"] = tri(N, a, b, c, 0, ANY)
            launches[f"tri_count_{tag}"] = tri(N, a, b, c, 0, 0)
            launches[f"tri_k{K}_{tag}"] = tri(N, a, b, c, K, 0)
            launches[f"box_count_{tag}"] = lambda blo=blo, bhi=bhi: L.tyr_query_box(g.h, N, blo.data_ptr(), bhi.data_ptr(), 0, 0, C.byref(bout), h)
            sizes.update({k: N for k in launches if k.endswith(tag)})
    vert, e1, e2 = (np.ascontiguousarray(prims[k], F) for k in ("vert", "e1", "e2"))
    own = [on(vert), on((vert + e1).astype(F)), on((vert + e2).astype(F))]  # the corners the library gives the scene's triangles
    keep += own
    n_own = len(prims)
    launches["tri_any_own_skip_shared"] = tri(n_own, *own, 0, ANY | SKIP)
    launches["tri_count_own_skip_shared"] = tri(n_own, *own, 0, SKIP)
    launches["tri_count_own"] = tri(n_own, *own, 0, 0)
    sizes.update({k: n_own for k in launches if "_own" in k})
    found = {}

    def read_found(name, rep):
        if rep != 0 or "_count_" not in name:
            return
        cnt = count[: sizes[name]]
        found[name] = {"members_per_query": float(cnt.float().mean().item()), "touching_share": float((cnt > 0).float().mean().item()), f"share_above_{K}": float((cnt > K).float().mean().item())}

    samples = timed_rounds(g, launches, stream, args.reps, after=read_found)
    batches = {k: stats(v, sizes[k], unit="queries", count=True) for k, v in samples.items()}
    ratio = {k: batches[k]["median_ms"] / batches["box_count_" + k.split("_", 2)[2]]["median_ms"] for k in batches if k.startswith("tri_") and "_own" not in k}
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "mean_triangle_edge": mean_edge,
              "query_mean_edge": query_edges, "batches": batches, "found": found, "tri_over_box_count": ratio, "kernel_time": "not measured here: event times around each launch"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["mqueries_s"], 1) for k, v in batches.items()}))
    print(json.dumps({k: round(v, 2) for k, v in ratio.items()}))
    print(json.dumps(found))


if __name__ == "__main__":
    main()
