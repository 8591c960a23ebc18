"""Records tests/golden/signed_c3.npz: on C3's mesh (scenes.mesh_scene(), 996,882 triangles) the answers of the numpy restatement
of tyr_query_signed and tyr_bake_sdf (tests/signed_ref.py) for 256 seeded points near the surface and for one 16^3 window of a
bake that holds near and far bricks.  A one-off CPU run of a few minutes of numpy (--jobs spreads the points over processes).  No
GPU is needed.

The points lie within 0.05 of the surface (a seeded triangle's point plus a uniform offset), on both sides of it; every fourth has
a max_dist of 0.01, the others none.  Their closest triangles are brute force over all triangles.  (C3's mesh is a room seen from
inside with a terrain in it: w runs from -1.5 to 0.15, so no point counts as inside and every sd is positive; the sign rule is
the small scenes' business in tests/test_signed_query.py.)  The window has cells of 0.25
and a band of two cells, and sits on a seeded surface point so that the sheet passes through its lower bricks and its upper
bricks are far; the closest-point half of its restatement runs on the triangles whose boxes come within 2 * reach + 1 of the
window (every triangle that can be within reach of a brick centre, with room), the winding half on the whole tree.  The file
holds the inputs, the answers and a digest of the triangle array they belong to; tests/test_signed_query.py::test_c3_tree checks
the digest, checks the recorded answers against the join's rules and recomputes one point by brute force on every run.

    python tools/signed_c3_golden.py [--jobs 8] [--out tests/golden/signed_c3.npz]
"""
from __future__ import annotations

import argparse
import hashlib
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from query_bench_common import surface_points  # noqa: E402

N = 256
F = np.float32
CELL, DIMS, BAND_CELLS = 0.25, (16, 16, 16), 2.0


def c3_points(prims):
    rng = np.random.default_rng(35)
    md = np.full(N, np.inf, F)
    md[::4] = 0.01
    return surface_points(rng, prims, N, 0.05), md


def c3_window(prims):
    """(origin, cell, dims, band) of the window: a seeded surface point lies in its third layer of voxels from below"""
    s = surface_points(np.random.default_rng(36), prims, 1, 0.0)[0]
    origin = (s - np.array([8, 8, 3], F) * F(CELL)).astype(F)
    return tuple(float(x) for x in origin), CELL, DIMS, BAND_CELLS * CELL


def digest_of(prims):
    return hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest()


def _job(args):
    import nearest_ref

    pts, md, prims = args
    return nearest_ref.nearest(pts, prims, md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "signed_c3.npz"))
    args = ap.parse_args()

    import nearest_ref
    import signed_ref as ref
    import winding_ref
    from tyrant_amd import binding, scenes

    sc = scenes.mesh_scene()
    nodes, prims = binding.bvh_build(sc.triangles)
    tree = ref.tree_of(nodes, prims)
    pts, md = c3_points(prims)
    parts = [slice(k, min(k + 8, N)) for k in range(0, N, 8)]
    with multiprocessing.Pool(args.jobs) as pool:
        res = pool.map(_job, [(pts[s], md[s], prims) for s in parts])
    dist2, prim, _, _, point = (np.concatenate([r[k] for r in res]) for k in range(5))
    w, _ = winding_ref.winding(tree, pts, 2.0)
    answers = dict(zip(ref.NAMES, ref.join(pts, md, dist2, prim, point, w, prims)))

    origin, cell, dims, band = c3_window(prims)
    vert, e1, e2 = (a.astype(np.float64) for a in nearest_ref.records(prims))
    corners = np.stack([vert, vert + e1, vert + e2])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    wlo, whi = np.array(origin, np.float64), np.array(origin, np.float64) + cell * np.array(dims)
    gap = np.maximum(np.maximum(wlo - hi, lo - whi), 0.0)
    near = np.nonzero(np.sqrt((gap * gap).sum(axis=1)) <= 2.0 * float(ref.reach(band, cell)) + 1.0)[0]
    gsd, gprim, gstats, _ = ref.bake(nodes, prims, origin, cell, dims, band, 2.0, tree=tree, prims_near=near)
    assert gstats[0] > 0 and gstats[1] > 0, gstats
    np.savez_compressed(args.out, digest=np.array(digest_of(prims)), points=pts, max_dist=md, origin=np.array(origin, F), cell=np.array(cell, F), dims=np.array(dims, np.uint32),
                        band=np.array(band, F), grid_sd=gsd, grid_prim=gprim, grid_stats=gstats, **answers)
    sd, prim = answers["sd"], answers["prim"]
    print(f"{args.out}: {int((prim >= 0).sum())} of {N} points have a triangle within their bound, {int((sd < 0).sum())} are inside; the window has {int(gstats[0])} near and "
          f"{int(gstats[1])} far bricks, {int((gsd < 0).sum())} voxels inside, {len(near)} triangles near it")


if __name__ == "__main__":
    main()
