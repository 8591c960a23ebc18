"""Throughput of the batched k-nearest queries (tyr_query_nearest_k) on C3's scene, next to tyr_query_nearest in the same run.

C3's scene (scenes.mesh_scene(), 996,882 triangles) and the two batches of 2 Mi points of tools/nearest_bench.py (same seed):
  uniform  uniform in the root box inflated by 10 %
  surface  within 0.5 of the surface: a seeded triangle's point plus a uniform offset of at most 0.5 per axis
On each: tyr_query_nearest (the yardstick: its kernel is shared code and its time must lie within the spread committed in
profiles/nearest_bench_c3.json), tyr_query_nearest_k at k = 1, 8 and 32 without a count and without a bound, and k = 8 with
the count inside --radius.  All outputs are asked for.  The launches run in turn, REPS rounds after a warm-up, each timed
with device events around its launch on a stream of their own: median and p10-p90 per launch, k = 1 against the yardstick,
and the cost per added entry from k = 1 to 8 and from 8 to 32.  A round starts with the two yardstick launches, one behind
the other as tools/nearest_bench.py has them, after an untimed tyr_query_nearest: behind the k = 32 launches, which write
1.9 GB of rows past the 83 MB scene in the 256 MB Infinity Cache, the surface yardstick measured 3.23 ms instead of 3.14.

    python tools/nearest_k_bench.py [--reps 20] [--radius 0.4] [--out profiles/nearest_k_bench_c3.json]
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

from query_bench_common import c3_points, stats, timed_rounds  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402

N = 1 << 21
KS = (1, 8, 32)
K_COUNT = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_k_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    nodes, prims, _ = g.build_upload(sc.triangles)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    sets = {name: torch.from_numpy(p).to(dev) for name, p in c3_points(nodes, prims, N).items()}
    radius = torch.full((N,), args.radius, dtype=torch.float32, device=dev)
    kmax = max(KS)
    d2, prim, uv = torch.empty((N, kmax), dtype=torch.float32, device=dev), torch.empty((N, kmax), dtype=torch.int32, device=dev), torch.empty((N, kmax, 2), dtype=torch.float32, device=dev)
    region, point = torch.empty((N, kmax), dtype=torch.uint8, device=dev), torch.empty((N, kmax, 3), dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    one = binding.NearestOut(d2.data_ptr(), prim.data_ptr(), uv.data_ptr(), region.data_ptr(), point.data_ptr())
    rows = binding.NearestKOut(d2.data_ptr(), prim.data_ptr(), None, uv.data_ptr(), region.data_ptr(), point.data_ptr())
    counted = binding.NearestKOut(d2.data_ptr(), prim.data_ptr(), count.data_ptr(), uv.data_ptr(), region.data_ptr(), point.data_ptr())
    L = g.L

    launches = {"untimed_nearest": lambda p=sets["surface"]: L.tyr_query_nearest(g.h, N, p.data_ptr(), None, 0, C.byref(one), h)}
    for name, p in sets.items():
        launches[f"nearest_{name}"] = lambda p=p: L.tyr_query_nearest(g.h, N, p.data_ptr(), None, 0, C.byref(one), h)
    for name, p in sets.items():
        for k in KS:
            launches[f"nearest_k{k}_{name}"] = lambda p=p, k=k: L.tyr_query_nearest_k(g.h, N, p.data_ptr(), None, k, 0, C.byref(rows), h)
        launches[f"nearest_k{K_COUNT}_count_{name}"] = lambda p=p: L.tyr_query_nearest_k(g.h, N, p.data_ptr(), radius.data_ptr(), K_COUNT, 0, C.byref(counted), h)
    mean_count = {}

    def read_count(name, rep):
        if rep < 2 and "_count_" in name:
            mean_count[name] = float(count.double().mean().item())

    samples = timed_rounds(g, launches, stream, args.reps, after=read_count)
    batches = {k: stats(v, N) for k, v in samples.items() if not k.startswith("untimed")}
    derived = {}
    for name in sets:
        t = {k: batches[f"nearest_k{k}_{name}"]["median_ms"] for k in KS}
        derived[name] = {"k1_over_nearest": t[1] / batches[f"nearest_{name}"]["median_ms"],
                         "ns_per_point_per_added_entry_1_to_8": (t[8] - t[1]) * 1e6 / N / 7, "ns_per_point_per_added_entry_8_to_32": (t[32] - t[8]) * 1e6 / N / 24}
    # the yardstick against the spread committed by tools/nearest_bench.py
    committed = os.path.join(ROOT, "profiles", "nearest_bench_c3.json")
    yardstick = {}
    if os.path.exists(committed):
        old = json.load(open(committed))["batches"]
        for name in sets:
            o, med = old[f"nearest_{name}"], batches[f"nearest_{name}"]["median_ms"]
            yardstick[name] = {"median_ms": med, "committed_p10_p90_ms": [o["p10_ms"], o["p90_ms"]], "inside": bool(o["p10_ms"] <= med <= o["p90_ms"])}
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "items": N, "radius": args.radius,
              "batches": batches, "mean_count_inside_radius": mean_count, "derived": derived, "yardstick_tyr_query_nearest": yardstick,
              "kernel_time": "not measured: event times around the launches only"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"median_ms": {k: round(v["median_ms"], 3) for k, v in batches.items()}, "mean_count": mean_count, "yardstick": yardstick}))


if __name__ == "__main__":
    main()
