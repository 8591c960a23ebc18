"""Throughput of the batched ray queries (tyr_query_closest / tyr_query_any) next to the render's extend stage on the same rays.

C3's scene (scenes.mesh_scene(), 996,882 triangles) and three ray sets:
  (a) camera  the 1080p camera rays, exported after stage("primary")
  (b) bounce  the survivors of the first bounce, exported after one stage("shade"): incoherent rays
  (c) random  uniform random origins in the scene box, uniform directions
For each set: query_closest (without and with the spheres), query_any (tmax = VERY_FAR), timed with device events on a
stream of their own after a warm-up, REPS repetitions, median and spread in Mrays/s; and the yardstick -- stage("extend")
on the same records (imported as the work queue, budget 0) under TYR_FLAG_PROFILE: the extend launches' hipEvent time
(sphere pre-pass + k_trace_flat).  Every query answer is also checked against the extend stage's (distance, identifier).

    python tools/query_bench.py [--reps 20] [--out profiles/query_bench_c3.json]
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

from query_bench_common import stats  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402

W, H = 1920, 1080


def time_query(g, kind, o, d, outs, flags, reps, stream):
    L, n = g.L, o.shape[0]
    h = stream.cuda_stream

    def launch():
        if kind == "closest":
            t, p, ge, uv = outs
            rc = L.tyr_query_closest(g.h, n, o.data_ptr(), d.data_ptr(), None, flags, t.data_ptr(), p.data_ptr(), ge.data_ptr(), uv.data_ptr(), h)
        else:
            rc = L.tyr_query_any(g.h, n, o.data_ptr(), d.data_ptr(), None, flags, outs[0].data_ptr(), h)
        if rc:
            raise binding.TyrError(rc, "tyr_query")

    for _ in range(3):
        launch()
    stream.synchronize()
    samples = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        launch()
        b.record(stream)
        b.synchronize()
        samples.append(a.elapsed_time(b))
    assert g.query_error() == 0
    return stats(samples, n, unit="rays", spread="min_max")


def time_extend(g, rays, reps):
    """stage("extend") on `rays` imported as the work queue (budget 0: stage("primary") adds none): its hipEvent time"""
    n = rays.shape[0]
    samples, q = [], None
    for i in range(reps + 1):
        g.stage("begin")
        g.import_work_queue(rays, n)
        g.set_budget(0)
        g.stage("primary")
        g.timings(reset=True)
        g.stage("extend")
        ms = g.timings()["extend"]["ms"]
        if i == 0:
            q = g.ray_queue(0, n)  # (the warm-up's answers: for the cross-check)
        else:
            samples.append(ms)
        g.stage("end")
    return stats(samples, n, unit="rays", spread="min_max"), q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    N = W * H
    g = binding.Renderer(W, H, N, flags=binding.TYR_FLAG_TRIANGLE_MATERIALS | binding.TYR_FLAG_PROFILE)
    nodes, prims, _ = g.build_upload(sc.triangles)
    g.set_spheres(sc.spheres)
    g.set_camera(sc.camera)
    # (a) camera rays, (b) first-bounce survivors
    g.set_budget(N)
    g.stage("begin")
    g.stage("primary")
    n_cam = g.counters()["n_live"]
    cam = g.ray_queue(0, n_cam)
    g.stage("extend")
    g.stage("shade")
    n_surv = g.counters()["primary_ray_cnt"]
    bounce = g.ray_queue(1, n_surv)
    g.stage("connect")
    g.stage("end")
    # (c) random rays in the scene box
    rng = np.random.default_rng(2024)
    lo, hi = nodes[0]["bounds"][0].astype(np.float32), nodes[0]["bounds"][1].astype(np.float32)
    rnd = np.zeros(N, dtype=scenes.RAY_DTYPE)
    rnd["origin"] = lo + (hi - lo) * rng.random((N, 3)).astype(np.float32)
    dd = rng.normal(size=(N, 3)).astype(np.float32)
    rnd["direction"] = dd / np.linalg.norm(dd, axis=1, keepdims=True)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "sets": {}}
    for name, rays in (("a_camera", cam), ("b_bounce", bounce), ("c_random", rnd)):
        rays = np.ascontiguousarray(rays).copy()
        rays["direct"] = 1.0
        rays["distance"] = np.float32(1e20)
        n = rays.shape[0]
        o = torch.from_numpy(np.ascontiguousarray(rays["origin"])).to(dev)
        d = torch.from_numpy(np.ascontiguousarray(rays["direction"])).to(dev)
        outs = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty((n, 2), dtype=torch.float32, device=dev))
        occ = (torch.empty(n, dtype=torch.bool, device=dev),)
        r = {"rays": n}
        r["extend_stage"], q = time_extend(g, rays, args.reps)
        r["query_closest"] = time_query(g, "closest", o, d, outs, 0, args.reps, stream)
        r["query_any"] = time_query(g, "any", o, d, occ, 0, args.reps, stream)
        r["query_closest_spheres"] = time_query(g, "closest", o, d, outs, binding.TYR_QUERY_SPHERES, args.reps, stream)
        stream.synchronize()
        # the spheres query answers what the extend stage answered
        t, p, ge = (x.cpu().numpy() for x in outs[:3])
        hit = q["distance"] < np.float32(1e20)
        same = np.array_equal(t.view(np.uint32), q["distance"].view(np.uint32)) and np.array_equal(p[hit], q["identifier"][hit]) and np.array_equal(ge[hit], q["geometry_type"][hit])
        r["matches_extend"] = bool(same)
        ext = r["extend_stage"]["mrays_s"]
        r["ratio_closest_spheres_vs_extend"] = r["query_closest_spheres"]["mrays_s"] / ext
        r["ratio_closest_vs_extend"] = r["query_closest"]["mrays_s"] / ext
        result["sets"][name] = r
        print(f"{name:9s} n={n:8d}  extend {ext:8.1f}  closest {r['query_closest']['mrays_s']:8.1f}  closest+spheres {r['query_closest_spheres']['mrays_s']:8.1f}  "
              f"any {r['query_any']['mrays_s']:8.1f} Mrays/s   ratio(closest+spheres / extend) {r['ratio_closest_spheres_vs_extend']:.2f}  matches extend: {same}", flush=True)
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {kk: (vv["mrays_s"] if isinstance(vv, dict) and "mrays_s" in vv else vv) for kk, vv in v.items()} for k, v in result["sets"].items()}))


if __name__ == "__main__":
    main()
