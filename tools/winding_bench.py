"""Throughput of the batched winding-number queries (tyr_query_winding) on C3's mesh.

C3's scene (scenes.mesh_scene(), 996,882 triangles) uploaded with TYR_FLAG_WINDING; 1 Mi points uniform in the mesh's root box,
asked in two orders -- as drawn (random) and sorted along a Morton curve (30-bit keys) -- at accuracy 2, 3 and 4, and the exact
mode (accuracy inf) on 4 Ki points for scale.  Each launch is timed with device events around it on a stream of its own, REPS
rounds after two warm-up rounds: median and p10-p90, points per second, the mean dipoles and triangles per point, and the lane
efficiency computed on the host from `terms`: per 64 consecutive points, the sum of their terms over 64 times the largest, averaged
over the batch's waves.  The moment build: the bytes it adds to device_bytes, and the median wall time of tyr_scene_upload of the
same arrays on a ctx with the flag and on one without (their difference is the build, its scratch and its drain).  No time is a
gate.

    python tools/winding_bench.py [--reps 10] [--out profiles/winding_bench_c3.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime in the process, see tests/conftest.py)

import numpy as np  # noqa: E402

from query_bench_common import morton_order, stats, timed_rounds  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402


def lane_efficiency(terms):
    t = terms.astype(np.int64).sum(axis=1)
    t = t[: t.size // 64 * 64].reshape(-1, 64)
    return float((t.sum(axis=1) / (64.0 * np.maximum(t.max(axis=1), 1))).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--exact-points", type=int, default=1 << 12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_bench_c3.json"))
    args = ap.parse_args()
    n = args.points

    sc = scenes.mesh_scene()
    nodes, prims = binding.bvh_build(sc.triangles)
    g = binding.Renderer(64, 64, 4096, flags=binding.TYR_FLAG_WINDING)
    g0 = binding.Renderer(64, 64, 4096)
    wall = {"with_flag": [], "without_flag": []}
    for rep in range(6):
        for key, r in (("with_flag", g), ("without_flag", g0)):
            t0 = time.perf_counter()
            r.upload(nodes, prims)
            if rep:
                wall[key].append((time.perf_counter() - t0) * 1e3)
    build = {"upload_ms_with_flag": float(np.median(wall["with_flag"])), "upload_ms_without_flag": float(np.median(wall["without_flag"])),
             "bytes": int(g.scene_info()["device_bytes"] - g0.scene_info()["device_bytes"]), "nodes": int(nodes.shape[0])}
    build["build_ms"] = build["upload_ms_with_flag"] - build["upload_ms_without_flag"]
    g0.close()

    lo, hi = nodes[0]["bounds"][0].astype(np.float64), nodes[0]["bounds"][1].astype(np.float64)
    rng = np.random.default_rng(91)
    pts = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    cells = np.clip(((pts.astype(np.float64) - lo) / (hi - lo) * 1024.0).astype(np.int64), 0, 1023)
    orders = {"random": pts, "morton": pts[morton_order(cells)]}

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    L = g.L
    w = torch.empty(n, dtype=torch.float32, device=dev)
    terms = torch.empty((n, 2), dtype=torch.int32, device=dev)
    launches, walk = {}, {}
    for order, p in orders.items():
        tp = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
        for acc in (2.0, 3.0, 4.0):
            _, t = g.query_winding(tp, accuracy=acc, terms=True)
            t = t.cpu().numpy()
            walk[f"{order}/accuracy_{acc:g}"] = {"dipoles_per_point": float(t[:, 0].mean()), "triangles_per_point": float(t[:, 1].mean()), "lane_efficiency": lane_efficiency(t)}
            launches[f"{order}/accuracy_{acc:g}"] = (n, lambda tp=tp, acc=acc: L.tyr_query_winding(g.h, n, tp.data_ptr(), acc, w.data_ptr(), None, h))
        m = args.exact_points
        launches[f"{order}/exact"] = (m, lambda tp=tp, m=m: L.tyr_query_winding(g.h, m, tp.data_ptr(), math.inf, w.data_ptr(), terms.data_ptr(), h))
    # (the exact launches take seconds each: two timed rounds are enough for a scale)
    samples = timed_rounds(g, {k: launch for k, (_, launch) in launches.items()}, stream, args.reps, rounds={k: 4 for k in launches if k.endswith("exact")})
    res = {k: dict(stats(v, launches[k][0], unit="points", count=True), **walk.get(k, {})) for k, v in samples.items()}
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "points": n,
              "moment_build": build, "launches": res, "kernel_time": "not measured here: event times around each launch"}
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"mpoints_s": {k: round(v["mpoints_s"], 2) for k, v in res.items()}, "lane_efficiency": {k: round(v["lane_efficiency"], 3) for k, v in walk.items()},
                      "build_ms": round(build["build_ms"], 2), "build_bytes": build["bytes"]}))


if __name__ == "__main__":
    main()
