"""Time of the signed-distance queries (tyr_query_signed) and the SDF grid bake (tyr_bake_sdf) on C3's scene, next to what they
replace: tyr_query_nearest plus tyr_query_winding on the same points, joined in torch.

C3's scene (scenes.mesh_scene(), 996,882 triangles, mean triangle edge 0.35).  Points: the first Mi points of
tools/nearest_bench.py's "surface" batch (within 0.5 of the surface), shuffled (as drawn) and sorted by their Morton code, without
a bound and with max_dist = 0.5; the baseline is tyr_query_nearest with the same bound and tyr_query_winding, one after the other
on the same stream, timed as one span.  Grids: the scene's bounding box at 128^3 and 256^3 cubic cells (cell = the box's largest
extent / n), with a band of 3 cells and with a band of the box's diagonal, which no brick is farther than; the baseline is the
same two calls on the voxel centres handed over as an (N, 3) array in brick-major order (the order the bake works in), with
max_dist = band, plus the elementwise join (where / sqrt on the stream), timed as one span.  The launches run in turn, REPS rounds
after two warm-up rounds, each span timed with device events on a stream of their own: median and p10-p90 per case, the near and
far brick counts, and the ratios new / baseline of the medians.  On the first warm-up round the new call's sd is compared with
the baseline's join, so that the two are known to time the same answer.

    python tools/signed_bench.py [--reps 10] [--grid-reps 5] [--out profiles/signed_bench_c3.json]
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
ACCURACY = 2.0
GRIDS = (128, 256)
BAND_CELLS = 3.0


def brick_major_centres(origin, cell, n):
    """the n^3 voxel centres by the header's rule, (N, 3) float32, brick by brick (4 x 4 x 4, x fastest inside a brick and among
    bricks); and each one's index in the (nz, ny, nx) grid"""
    f = np.float32
    axis = [(f(origin[k]) + (f(cell) * (np.arange(n).astype(f) + f(0.5))).astype(f)).astype(f) for k in range(3)]
    b = n // 4
    i = np.arange(n ** 3, dtype=np.int64)
    lane, brick = i % 64, i // 64
    x = 4 * (brick % b) + (lane & 3)
    y = 4 * ((brick // b) % b) + ((lane >> 2) & 3)
    z = 4 * (brick // (b * b)) + (lane >> 4)
    return np.stack([axis[0][x], axis[1][y], axis[2][z]], axis=1), (z * n + y) * n + x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--grid-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_bench_c3.json"))
    args = ap.parse_args()

    sc = scenes.mesh_scene()
    g = binding.Renderer(64, 64, 4096, flags=binding.TYR_FLAG_WINDING)
    nodes, prims, _ = g.build_upload(sc.triangles)
    surface = c3_points(nodes, prims, 1 << 21)["surface"][:N]
    lo, hi = nodes[0]["bounds"][0].astype(np.float32), nodes[0]["bounds"][1].astype(np.float32)
    orders = {"shuffled": np.arange(N), "morton": morton_order(np.clip((surface - lo) / (hi - lo) * 1023.0, 0, 1023))}

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    L = g.L
    launches, rounds, checks = {}, {}, {}

    def pair(name, reps, new, base, sd_new, sd_base):
        """a new call and its baseline, and the comparison of their answers behind the first warm-up round"""
        launches[f"{name}_new"], launches[f"{name}_baseline"] = new, base
        rounds[f"{name}_new"] = rounds[f"{name}_baseline"] = reps + 2
        checks[f"{name}_baseline"] = (name, sd_new, sd_base)

    def baseline(pts, md, n, d2, prim, w, sd, band):
        nout = binding.NearestOut(d2.data_ptr(), prim.data_ptr(), None, None, None)

        def run():
            rc = L.tyr_query_nearest(g.h, n, pts.data_ptr(), None if md is None else md.data_ptr(), 0, C.byref(nout), h)
            rc = rc or L.tyr_query_winding(g.h, n, pts.data_ptr(), ACCURACY, w.data_ptr(), None, h)
            with torch.cuda.stream(stream):
                m = torch.where(prim >= 0, d2.sqrt(), torch.full_like(d2, band))
                torch.where(w > 0.5, -m, m, out=sd)
            return rc

        return run

    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    # ---- points ----
    sd, prim, bd2, bprim, bw, bsd = f32(N), i32(N), f32(N), i32(N), f32(N), f32(N)
    sout = binding.SignedOut(sd.data_ptr(), prim.data_ptr(), None, None, None)
    bound = torch.full((N,), 0.5, dtype=torch.float32, device=dev)
    for name, order in orders.items():
        p = on(surface[order])
        for case, md, band in (("unbounded", None, float("inf")), ("max_dist_0.5", bound, 0.5)):
            pair(f"points_{name}_{case}", args.reps,
                 lambda p=p, md=md: L.tyr_query_signed(g.h, N, p.data_ptr(), None if md is None else md.data_ptr(), ACCURACY, 0, C.byref(sout), h),
                 baseline(p, md, N, bd2, bprim, bw, bsd, band), sd, bsd)
    # ---- grids ----
    extent = float((hi - lo).max())
    diagonal = float(np.linalg.norm((hi - lo).astype(np.float64)))
    grid_info, stat_words = {}, {}
    big = max(GRIDS) ** 3
    gsd, gd2, gprim, gw, gbsd = f32(big), f32(big), i32(big), f32(big), f32(big)
    for n in GRIDS:
        cell = extent / n
        centres, index = brick_major_centres(lo, cell, n)
        pts, idx = on(centres), torch.from_numpy(index).to(dev)
        for case, band in (("band_3_cells", BAND_CELLS * cell), ("band_diagonal", diagonal)):
            name = f"grid_{n}_{case}"
            grid = binding.SdfGrid((C.c_float * 3)(*map(float, lo)), cell, (C.c_uint32 * 3)(n, n, n), band, ACCURACY)
            st = torch.zeros(2, dtype=torch.int32, device=dev)
            stat_words[name] = st
            gout = binding.SdfOut(gsd.data_ptr(), None, st.data_ptr())
            md = torch.full((n ** 3,), band, dtype=torch.float32, device=dev)
            grid_info[name] = {"dims": [n, n, n], "cell": cell, "band": band, "voxels": n ** 3}
            # (the bake's sd is in grid order, the baseline's in brick-major order: compared through idx)
            pair(name, args.grid_reps, lambda grid=grid, gout=gout: L.tyr_bake_sdf(g.h, C.byref(grid), 0, C.byref(gout), h),
                 baseline(pts, md, n ** 3, gd2[:n ** 3], gprim[:n ** 3], gw[:n ** 3], gbsd[:n ** 3], band), (gsd, idx), gbsd[:n ** 3])
    agree = {}

    def compare(name, rep):
        if rep != 0 or name not in checks:
            return
        case, new, base = checks[name]
        if isinstance(new, tuple):
            new = new[0][new[1]]
        a, b = new[:base.numel()].view(torch.int32), base.view(torch.int32)
        agree[case] = {"values": int(base.numel()), "differing_words": int((a != b).sum().item())}

    times = timed_rounds(g, launches, stream, max(args.reps, args.grid_reps), after=compare, rounds=rounds)
    batches = {}
    for k, v in times.items():
        case = k.rsplit("_", 1)[0]
        batches[k] = stats(v, grid_info[case]["voxels"] if case in grid_info else N)
    ratios = {k[:-4]: batches[k]["median_ms"] / batches[k[:-4] + "_baseline"]["median_ms"] for k in batches if k.endswith("_new")}
    for name, st in stat_words.items():
        near, far = (int(x) for x in st.cpu().numpy().view(np.uint32))
        grid_info[name].update({"near_bricks": near, "far_bricks": far, "far_share": far / (near + far)})
    result = {"scene": sc.name, "triangles": int(sc.triangles.shape[0]), "device": torch.cuda.get_device_name(0), "reps": args.reps, "grid_reps": args.grid_reps, "points": N,
              "accuracy": ACCURACY, "grids": grid_info, "batches": batches, "ratio_new_over_baseline": ratios, "new_against_baseline_answers": agree,
              "kernel_time": "not measured here: event times around each span", "tuned": "the form of the points loop (DESIGN.md \"Signed distance\"); launch bounds and brick size as first tried"}
    g.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["median_ms"], 3) for k, v in batches.items()}))
    print(json.dumps({k: round(v, 3) for k, v in ratios.items()}))
    print(json.dumps(agree))
    print(json.dumps(grid_info))


if __name__ == "__main__":
    main()
