"""Throughput of the batched multi-hit queries (tyr_query_hits) on C3's scene, next to tyr_query_any and tyr_query_closest on
the same rays.

C3's scene (scenes.mesh_scene(), 996,882 triangles) and 2 Mi camera rays (a 2048 x 1024 grid from the scene's camera), asked
with max_hits 1, 4 and 32, one- and two-sided, beside the two sibling queries.  Then the expectation this kernel is held to: on
rays whose hit set is empty it does tyr_query_any's traversal -- the same boxes, every leaf to its end, nothing kept -- so on
such rays its time is measured against tyr_query_any's.  Two such batches are cut from the camera rays:
  empty_miss   the rays that go through nothing at all (count == 0 with tmax = VERY_FAR): most of them miss the root box
  empty_short  the rays that hit something, stopped at 0.9 of their first hit's distance: they descend and find nothing in range
The launches are made in turn, REPS rounds after a warm-up, each timed with device events around its launch on a stream of
their own: median and p10-p90 per batch, and hits / any as a ratio of medians.  No time is a gate.

    python tools/hits_bench.py [--reps 20] [--out profiles/hits_bench_c3.json]
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

from query_bench_common import camera_rays, stats, timed_rounds  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402

N = 1 << 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    g.build_upload(sc.triangles)
    origins, dirs = camera_rays(sc.camera)  # (2048 x 1024 = N)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    ro, rd = torch.from_numpy(origins).to(dev), torch.from_numpy(dirs).to(dev)
    # what the rays go through, for the report and for the two batches with an empty hit set
    count, _, _, _, _, back = g.query_hits(ro, rd, max_hits=1, two_sided=True)
    t_first = g.query_closest(ro, rd)[0]
    front = g.query_hits(ro, rd, max_hits=1)[0]
    miss = front == 0
    short = ~miss
    batches = {"camera": (ro, rd, None), "empty_miss": (ro[miss].contiguous(), rd[miss].contiguous(), None),
               "empty_short": (ro[short].contiguous(), rd[short].contiguous(), (t_first[short] * 0.9).contiguous())}
    for name in ("empty_miss", "empty_short"):  # keep the rays whose hit set is empty by both kernels' word
        o, d, tm = batches[name]
        keep = (g.query_hits(o, d, tm, max_hits=1)[0] == 0) & ~g.query_any(o, d, tm)
        batches[name] = (o[keep].contiguous(), d[keep].contiguous(), None if tm is None else tm[keep].contiguous())
        assert batches[name][0].shape[0] > N // 16, name

    L = g.L
    cnt, bcnt = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    ht, hp = torch.empty((N, 32), dtype=torch.float32, device=dev), torch.empty((N, 32), dtype=torch.int32, device=dev)
    huv, hs = torch.empty((N, 32, 2), dtype=torch.float32, device=dev), torch.empty((N, 32), dtype=torch.uint8, device=dev)
    out = binding.HitsOut(cnt.data_ptr(), ht.data_ptr(), hp.data_ptr(), huv.data_ptr(), hs.data_ptr(), bcnt.data_ptr())
    occ = torch.empty(N, dtype=torch.uint8, device=dev)
    ct, cp = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    cuv = torch.empty((N, 2), dtype=torch.float32, device=dev)

    def ptr(a):
        return None if a is None else a.data_ptr()

    def hits(batch, k, flags):
        o, d, tm = batches[batch]
        return o.shape[0], lambda: L.tyr_query_hits(g.h, o.shape[0], o.data_ptr(), d.data_ptr(), ptr(tm), k, flags, C.byref(out), h)

    def any_(batch):
        o, d, tm = batches[batch]
        return o.shape[0], lambda: L.tyr_query_any(g.h, o.shape[0], o.data_ptr(), d.data_ptr(), ptr(tm), 0, occ.data_ptr(), h)

    def closest(batch):
        o, d, tm = batches[batch]
        return o.shape[0], lambda: L.tyr_query_closest(g.h, o.shape[0], o.data_ptr(), d.data_ptr(), ptr(tm), 0, ct.data_ptr(), cp.data_ptr(), None, cuv.data_ptr(), h)

    launches = {"camera/any": any_("camera"), "camera/closest": closest("camera")}
    for k in (1, 4, 32):
        launches[f"camera/hits_{k}"] = hits("camera", k, 0)
        launches[f"camera/hits_{k}_two_sided"] = hits("camera", k, binding.TYR_QUERY_TWO_SIDED)
    for b in ("empty_miss", "empty_short"):
        launches[f"{b}/any"] = any_(b)
        launches[f"{b}/hits_4"] = hits(b, 4, 0)
    samples = timed_rounds(g, {k: launch for k, (_, launch) in launches.items()}, stream, args.reps)
    res = {k: stats(v, launches[k][0], count=True) for k, v in samples.items()}
    ratio = {b: res[f"{b}/hits_4"]["median_ms"] / res[f"{b}/any"]["median_ms"] for b in ("empty_miss", "empty_short")}
    c = count.to(torch.int64)
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "rays": N,
              "camera_rays": {"mean_count_two_sided": float(c.float().mean().item()), "max_count_two_sided": int(c.max().item()), "mean_back_count": float(back.float().mean().item()),
                              "fraction_count_over_4": float((c > 4).float().mean().item()), "fraction_empty_one_sided": float(miss.float().mean().item())},
              "launches": res, "hits_over_any_on_empty_hit_sets": ratio,
              "kernel_time": "not measured here: event times around each launch"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"mrays_s": {k: round(v["mitems_s"], 1) for k, v in res.items()}, "hits_over_any_on_empty_hit_sets": {k: round(v, 3) for k, v in ratio.items()}}))


if __name__ == "__main__":
    main()
