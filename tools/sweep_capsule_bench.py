"""Throughput of the batched swept-capsule queries (tyr_query_sweep_capsule) on C3's scene, next to tyr_query_sweep on the same
p, d and r and next to the workaround it replaces: eight sphere sweeps at samples along the axis, and a minimum.

C3's scene (scenes.mesh_scene(), 996,882 triangles) and 1 Mi capsules: p is tools/nearest_bench.py's "surface" batch (within 0.5
of the surface, drawn from the same seed), the displacement tools/sweep_bench.py's (up to 3 units per axis), the axis a seeded
direction of 1, 4 or 16 mean triangle edges, the radius 0 or 0.1 (one length and one radius per launch).  The launches run in
turn, REPS rounds after two warm-up rounds, each timed with device events around it on a stream of their own: median and p10-p90
per launch and capsules per second; the share of the capsules that touch the mesh (and of those, that start in overlap); and the
share for which the workaround's t is later than the capsule's by more than 1e-4 -- contacts between the samples.  The sphere
sweep at p is context, not a gate: it answers another question.

    python tools/sweep_capsule_bench.py [--reps 5] [--out profiles/sweep_capsule_bench_c3.json]
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

from query_bench_common import c3_points, stats, timed_rounds  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402

N = 1 << 20
LENGTHS = (1.0, 4.0, 16.0)  # in mean triangle edges
RADII = (0.0, 0.1)
SAMPLES = 8
LATE = 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_capsule_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096)
    nodes, prims, _ = g.build_upload(sc.triangles)
    e1, e2 = prims["e1"].astype(np.float64), prims["e2"].astype(np.float64)
    mean_edge = float(np.mean([np.linalg.norm(e, axis=1).mean() for e in (e1, e2, e2 - e1)]))
    surface = c3_points(nodes, prims, 1 << 21)["surface"][:N]
    rng = np.random.default_rng(2026)
    disp = rng.uniform(-3.0, 3.0, (1 << 21, 3)).astype(np.float32)[:N]  # tools/sweep_bench.py's displacements
    axis = np.random.default_rng(2027).normal(size=(N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    p, d = on(surface), on(disp)
    ends = {ln: on(surface + axis * (ln * mean_edge)) for ln in LENGTHS}
    along = {ln: [(p + (ends[ln] - p) * (k / (SAMPLES - 1))).contiguous() for k in range(SAMPLES)] for ln in LENGTHS}
    radius = {r: torch.full((N,), r, dtype=torch.float32, device=dev) for r in RADII}
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    u8 = lambda: torch.empty(N, dtype=torch.uint8, device=dev)  # noqa: E731
    t, prim, s, feature, region, point, center, normal = f32(N), torch.empty(N, dtype=torch.int32, device=dev), f32(N), u8(), u8(), f32(N, 3), f32(N, 3), f32(N, 3)
    cout = binding.SweepCapsuleOut(*(x.data_ptr() for x in (t, prim, s, feature, region, point, center, normal)))
    st, sprim = f32(N), torch.empty(N, dtype=torch.int32, device=dev)
    sout = binding.SweepOut(st.data_ptr(), sprim.data_ptr(), None, None, None, None)
    wt, wbest = f32(N), f32(N)
    wout = binding.SweepOut(wt.data_ptr(), sprim.data_ptr(), None, None, None, None)
    L = g.L

    def workaround(ln, r):
        with torch.cuda.stream(stream):
            wbest.fill_(float("inf"))
            for o in along[ln]:
                rc = L.tyr_query_sweep(g.h, N, o.data_ptr(), d.data_ptr(), radius[r].data_ptr(), None, 0, C.byref(wout), h)
                if rc:
                    return rc
                torch.minimum(wbest, torch.where(sprim >= 0, wt, torch.full_like(wt, float("inf"))), out=wbest)
        return 0

    launches = {}
    for r in RADII:
        launches[f"sweep_r{r:g}"] = lambda r=r: L.tyr_query_sweep(g.h, N, p.data_ptr(), d.data_ptr(), radius[r].data_ptr(), None, 0, C.byref(sout), h)
        for ln in LENGTHS:
            launches[f"capsule_len{ln:g}_r{r:g}"] = lambda r=r, ln=ln: L.tyr_query_sweep_capsule(g.h, N, p.data_ptr(), ends[ln].data_ptr(), d.data_ptr(), radius[r].data_ptr(), None, 0, C.byref(cout), h)
            launches[f"spheres{SAMPLES}_len{ln:g}_r{r:g}"] = lambda r=r, ln=ln: workaround(ln, r)
    found, truth = {}, {}

    def read_found(name, rep):
        if rep != 0:
            return
        if name.startswith("capsule_"):
            hit = prim >= 0
            truth[name[len("capsule_"):]] = torch.where(hit, t, torch.full_like(t, float("inf")))
            found[name] = {"hit_share": float(hit.float().mean().item()), "overlap_share_of_hits": float((hit & (t == 0)).sum().item() / max(int(hit.sum().item()), 1))}
        elif name.startswith("spheres"):
            true_t = truth[name.split("_", 1)[1]]  # (the capsule of the same length and radius runs just before)
            late = (wbest - true_t > LATE) | (torch.isinf(wbest) & ~torch.isinf(true_t))
            found[name] = {"late_share": float(late.float().mean().item()), "late_share_of_hits": float(late.sum().item() / max(int((~torch.isinf(true_t)).sum().item()), 1)),
                           "earlier_than_the_capsule": int((true_t - wbest > LATE).sum().item())}

    samples = timed_rounds(g, launches, stream, args.reps, after=read_found)
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "items": N,
              "mean_edge": mean_edge, "axis_lengths_in_mean_edges": LENGTHS, "displacement": "uniform in [-3, 3] per axis", "late_threshold": LATE,
              "batches": {k: stats(v, N) for k, v in samples.items()}, "found": found, "kernel_time": "not measured here: event times around each launch"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["median_ms"], 3) for k, v in result["batches"].items()}))
    print(json.dumps(found))


if __name__ == "__main__":
    main()
