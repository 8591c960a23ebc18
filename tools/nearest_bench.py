"""Throughput of the batched closest-point queries (tyr_query_nearest) on C3's scene, next to tyr_query_closest as a yardstick.

C3's scene (scenes.mesh_scene(), 996,882 triangles) and two batches of 2 Mi points:
  uniform  uniform in the root box inflated by 10 %
  surface  within 0.5 of the surface: a seeded triangle's point plus a uniform offset of at most 0.5 per axis
and the yardstick, tyr_query_closest on 2 Mi camera-like rays (a 2048 x 1024 grid from the scene's camera) in the same process.
The three are launched in turn, REPS rounds after a warm-up, each timed with device events around its launch on a stream of
their own: median and p10-p90 per batch.  The yardstick is context, not a gate: the two queries do different work.  Kernel
time comes from a separate run under rocprofv3 --kernel-trace --stats (this file reports event times only).

    python tools/nearest_bench.py [--reps 20] [--out profiles/nearest_bench_c3.json]
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

from query_bench_common import c3_points, camera_rays, stats, timed_rounds  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402

N = 1 << 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    nodes, prims, _ = g.build_upload(sc.triangles)
    points = c3_points(nodes, prims, N)
    origins, dirs = camera_rays(sc.camera)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    pu, ps, ro, rd = on(points["uniform"]), on(points["surface"]), on(origins), on(dirs)
    d2, prim, uv = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty((N, 2), dtype=torch.float32, device=dev)
    region, point = torch.empty(N, dtype=torch.uint8, device=dev), torch.empty((N, 3), dtype=torch.float32, device=dev)
    rt, rprim, rgeom = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    out = binding.NearestOut(d2.data_ptr(), prim.data_ptr(), uv.data_ptr(), region.data_ptr(), point.data_ptr())
    L = g.L

    def nearest(p):
        return lambda: L.tyr_query_nearest(g.h, N, p.data_ptr(), None, 0, C.byref(out), h)

    launches = {
        "nearest_uniform": nearest(pu),
        "nearest_surface": nearest(ps),
        "closest_camera_rays": lambda: L.tyr_query_closest(g.h, N, ro.data_ptr(), rd.data_ptr(), None, 0, rt.data_ptr(), rprim.data_ptr(), rgeom.data_ptr(), None, h),
    }
    samples = timed_rounds(g, launches, stream, args.reps)
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "items": N,
              "batches": {k: stats(v, N) for k, v in samples.items()}, "kernel_time": "not measured here: rocprofv3 --kernel-trace --stats in a run of its own"}
    # what the last nearest launch (the surface batch) found
    torch.cuda.synchronize()
    result["surface_batch"] = {"hits": int((prim >= 0).sum().item()), "median_distance": float(d2.sqrt().median().item())}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["mitems_s"], 1) for k, v in result["batches"].items()}))


if __name__ == "__main__":
    main()
