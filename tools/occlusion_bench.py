"""Throughput of the batched ambient-occlusion queries (tyr_query_occlusion) on C3's scene, next to tyr_query_any on the
identical rays.

C3's scene (scenes.mesh_scene(), 996,882 triangles), 64 Ki points on seeded triangles of the mesh (vert + 0.3 e1 + 0.3 e2) with
their face normals, 64 samples each (4 Mi rays), without max_dist and with max_dist = 10:
  a  tyr_query_occlusion, `visible` only
  b  the same with `mask` and `bent`
  c  tyr_query_any on the identical rays -- a's `origin` / `direction` outputs, written once outside the timed region
  d  c plus the torch reduction to a count per point: what a caller pays today, without making the rays
and, for scale, tyr_query_any on the 2 Mi camera rays of tools/hits_bench.py.  c is the yardstick: existing code on the same
rays.  The launches are made in turn, REPS rounds after a warm-up, each timed with device events around its launch on a stream
of their own: median and p10-p90 per variant, and a / c as a ratio of medians with the two spreads beside it.  No time is a gate.

    python tools/occlusion_bench.py [--reps 20] [--out profiles/occlusion_bench_c3.json]
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

from query_bench_common import camera_rays, stats, timed_rounds  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion_bench_c3.json"))
    args = ap.parse_args()
    n, S = args.points, args.samples

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    g.build_upload(sc.triangles)
    rng = np.random.default_rng(81)
    t = sc.triangles[rng.integers(0, sc.triangles.shape[0], n)]
    e1, e2 = t["e1"].astype(np.float32), t["e2"].astype(np.float32)
    points = (t["vert"] + np.float32(0.3) * e1 + np.float32(0.3) * e2).astype(np.float32)
    normals = np.cross(e1, e2).astype(np.float32)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    tp, tn = torch.from_numpy(points).to(dev), torch.from_numpy(normals).to(dev)
    dist = {"far": None, "10": torch.full((n,), 10.0, dtype=torch.float32, device=dev)}
    # the rays of variant a, once: what c and d trace
    visible0, _, _, origin, direction = g.query_occlusion(tp, tn, samples=S, seed=1, rays=True)
    ro, rd = origin.repeat_interleave(S, dim=0).contiguous(), direction.reshape(-1, 3).contiguous()
    rt = {"far": None, "10": torch.full((n * S,), 10.0, dtype=torch.float32, device=dev)}
    check = {}
    for k in dist:  # the fused call and the sibling agree, by count
        vis = g.query_occlusion(tp, tn, samples=S, max_dist=dist[k], seed=1)[0]
        occ = g.query_any(ro, rd, rt[k]).view(n, S)
        assert torch.equal(vis, (S - occ.sum(dim=1)).to(torch.int32)), k
        check[k] = {"mean_visibility": float(vis.float().mean().item()) / S, "fraction_partly_visible": float(((vis > 0) & (vis < S)).float().mean().item())}
    co, cd = (torch.from_numpy(a).to(dev) for a in camera_rays(sc.camera))

    L = g.L
    W = (S + 31) // 32
    vis = torch.empty(n, dtype=torch.int32, device=dev)
    msk, bnt = torch.empty((n, W), dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
    out_a = binding.OcclusionOut(vis.data_ptr(), None, None, None, None)
    out_b = binding.OcclusionOut(vis.data_ptr(), msk.data_ptr(), bnt.data_ptr(), None, None)
    occ = torch.empty(n * S, dtype=torch.bool, device=dev)
    occ_cam = torch.empty(co.shape[0], dtype=torch.bool, device=dev)

    def ptr(a):
        return None if a is None else a.data_ptr()

    def fused(k, out):
        return lambda: L.tyr_query_occlusion(g.h, n, tp.data_ptr(), tn.data_ptr(), ptr(dist[k]), S, 1e-3, 1, 0, C.byref(out), h)

    def any_(k):
        return lambda: L.tyr_query_any(g.h, n * S, ro.data_ptr(), rd.data_ptr(), ptr(rt[k]), 0, occ.data_ptr(), h)

    def any_reduced(k):
        def launch():
            rc = any_(k)()
            with torch.cuda.stream(stream):
                vis.copy_(S - occ.view(n, S).sum(dim=1))
            return rc
        return launch

    launches = {}
    for k in dist:
        launches[f"{k}/a_occlusion"] = (n * S, fused(k, out_a))
        launches[f"{k}/b_occlusion_mask_bent"] = (n * S, fused(k, out_b))
        launches[f"{k}/c_any_same_rays"] = (n * S, any_(k))
        launches[f"{k}/d_any_same_rays_reduced"] = (n * S, any_reduced(k))
    launches["camera/any"] = (co.shape[0], lambda: L.tyr_query_any(g.h, co.shape[0], co.data_ptr(), cd.data_ptr(), None, 0, occ_cam.data_ptr(), h))
    samples = timed_rounds(g, {k: launch for k, (_, launch) in launches.items()}, stream, args.reps)
    res = {k: stats(v, launches[k][0], count=True) for k, v in samples.items()}
    ratio = {}
    for k in dist:
        a, c = res[f"{k}/a_occlusion"], res[f"{k}/c_any_same_rays"]
        ratio[k] = {"a_over_c": a["median_ms"] / c["median_ms"], "b_over_c": res[f"{k}/b_occlusion_mask_bent"]["median_ms"] / c["median_ms"],
                    "a_over_d": a["median_ms"] / res[f"{k}/d_any_same_rays_reduced"]["median_ms"],
                    "a_p10_p90_over_c_median": [a["p10_ms"] / c["median_ms"], a["p90_ms"] / c["median_ms"]], "c_p10_p90_over_c_median": [c["p10_ms"] / c["median_ms"], c["p90_ms"] / c["median_ms"]]}
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "points": n, "samples": S, "rays": n * S,
              "visibility": check, "launches": res, "ratios_of_medians": ratio, "kernel_time": "not measured here: event times around each launch"}
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"mrays_s": {k: round(v["mitems_s"], 1) for k, v in res.items()}, "a_over_c": {k: round(v["a_over_c"], 3) for k, v in ratio.items()}}))


if __name__ == "__main__":
    main()
