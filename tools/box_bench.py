"""Throughput of the batched box-overlap queries (tyr_query_box) on C3's scene, next to the workaround that existed before it:
tyr_query_nearest_k with a count at the radius of the box's circumscribed sphere.

C3's scene (scenes.mesh_scene(), 996,882 triangles) and 1 Mi cubic boxes whose centres are tools/nearest_bench.py's "surface"
batch (within 0.5 of the surface, drawn from the same seed) -- the voxels a surface voxelisation asks about.  Three edge lengths:
the mesh's mean triangle edge, 4 and 16 times it; the batch in two orders, shuffled (as drawn) and sorted by the Morton code of
the centres; three variants per size and order: `any` (TYR_QUERY_BOX_ANY), a count alone (max_prims 0) and max_prims 16.  Beside
them tyr_query_nearest_k with k = 1 and a count on the same centres at max_dist = edge * sqrt(3) / 2: it counts every triangle
within the sphere round the box, so it over-reports, and it is context, not a gate.  The launches run in turn, REPS rounds after
two warm-up rounds, each timed with device events around its launch on a stream of their own: median and p10-p90 per launch,
boxes per second, the members per box, the share of boxes that touch anything, and box over nearest_k as a ratio of medians.

    python tools/box_bench.py [--reps 10] [--out profiles/box_bench_c3.json]
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
EDGES = (1, 4, 16)  # in mean triangle edges
K = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    nodes, prims, _ = g.build_upload(sc.triangles)
    centres = c3_points(nodes, prims, N)["surface"]
    mean_edge = float(np.linalg.norm(np.concatenate([prims["e1"], prims["e2"], prims["e2"] - prims["e1"]]).astype(np.float64), axis=1).mean())
    lo, hi = nodes[0]["bounds"][0].astype(np.float32), nodes[0]["bounds"][1].astype(np.float32)
    order = morton_order(np.clip((centres - lo) / (hi - lo) * 1023.0, 0, 1023))

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    count = torch.empty(N, dtype=torch.int32, device=dev)
    prim = torch.empty((N, K), dtype=torch.int32, device=dev)
    kd2, kprim, kcount = torch.empty((N, 1), dtype=torch.float32, device=dev), torch.empty((N, 1), dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    out = binding.BoxOut(count.data_ptr(), prim.data_ptr())
    kout = binding.NearestKOut(kd2.data_ptr(), kprim.data_ptr(), kcount.data_ptr(), None, None, None)
    L = g.L

    launches, keep = {}, []
    for name, c in (("shuffled", centres), ("morton", centres[order])):
        pts = on(c)
        for m in EDGES:
            half = np.float32(0.5 * m * mean_edge)
            blo, bhi = on(c - half), on(c + half)
            radius = torch.full((N,), float(half) * 3.0 ** 0.5, dtype=torch.float32, device=dev)
            keep += [pts, blo, bhi, radius]
            tag = f"{name}_edge{m}"
            launches[f"box_any_{tag}"] = lambda blo=blo, bhi=bhi: L.tyr_query_box(g.h, N, blo.data_ptr(), bhi.data_ptr(), 0, binding.TYR_QUERY_BOX_ANY, C.byref(out), h)
            launches[f"box_count_{tag}"] = lambda blo=blo, bhi=bhi: L.tyr_query_box(g.h, N, blo.data_ptr(), bhi.data_ptr(), 0, 0, C.byref(out), h)
            launches[f"box_k{K}_{tag}"] = lambda blo=blo, bhi=bhi: L.tyr_query_box(g.h, N, blo.data_ptr(), bhi.data_ptr(), K, 0, C.byref(out), h)
            launches[f"nearest_k_count_{tag}"] = lambda pts=pts, radius=radius: L.tyr_query_nearest_k(g.h, N, pts.data_ptr(), radius.data_ptr(), 1, 0, C.byref(kout), h)
    found = {}

    def read_found(name, rep):
        if rep != 0:
            return
        if name.startswith("box_count_"):
            found[name] = {"members_per_box": float(count.float().mean().item()), "touching_share": float((count > 0).float().mean().item()),
                           f"share_above_{K}": float((count > K).float().mean().item())}
        elif name.startswith("nearest_k_count_"):
            found[name] = {"triangles_per_sphere": float(kcount.float().mean().item())}

    samples = timed_rounds(g, launches, stream, args.reps, after=read_found)
    batches = {k: stats(v, N, unit="boxes") for k, v in samples.items()}
    ratio = {k: batches[k]["median_ms"] / batches["nearest_k_count_" + k.split("_", 2)[2]]["median_ms"] for k in batches if k.startswith("box_")}
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "boxes": N,
              "mean_triangle_edge": mean_edge, "edges_in_mean_triangle_edges": list(EDGES), "batches": batches, "found": found, "box_over_nearest_k_count": ratio,
              "kernel_time": "not measured here: event times around each launch"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["mboxes_s"], 1) for k, v in batches.items()}))
    print(json.dumps({k: round(v, 2) for k, v in ratio.items()}))
    print(json.dumps(found))


if __name__ == "__main__":
    main()
