"""Records tests/golden/tri_distance_c3.npz: 256 seeded triangles on C3's mesh (scenes.mesh_scene(), 996,882 triangles) and their
six answers by the numpy restatement of tyr_query_tri_distance (tests/tri_distance_ref.py), brute force over every triangle its
triangle-inequality shortlist keeps.  A one-off CPU run of a few minutes of numpy (--jobs spreads the queries over processes).
No GPU is needed.

The triangles' corners lie around points within 1.5 of the surface (a seeded triangle's point plus a uniform offset), at seeded
normal offsets scaled by a size class: 0 (a == b == c), 0.035, 0.35 (a mean triangle edge), 1.4, 5.6 and 40; every fourth query has
a max_dist of 0.25.  The file holds the queries, the answers and a digest of the triangle array they belong to;
tests/test_tri_distance_query.py::test_c3_tree checks the digest and evaluates the winners' pairs from the restatement on every
run.

    python tools/tri_distance_c3_golden.py [--jobs 8] [--out tests/golden/tri_distance_c3.npz]
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


def c3_triangles(prims):
    rng = np.random.default_rng(34)
    centre = surface_points(rng, prims, N, 1.5)
    size = rng.choice([0.0, 0.035, 0.35, 1.4, 5.6, 40.0], (N, 1))
    a, b, c = ((centre + rng.normal(size=(N, 3)) * size * 0.5).astype(F) for _ in range(3))
    md = np.full(N, np.inf, F)
    md[::4] = 0.25
    return a, b, c, md


def digest_of(prims):
    return hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest()


def _job(args):
    import tri_distance_ref as ref

    a, b, c, md, prims = args
    return ref.tri_distance(a, b, c, prims, md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tri_distance_c3.npz"))
    args = ap.parse_args()

    import tri_distance_ref as ref
    from tyrant_amd import binding, scenes

    sc = scenes.mesh_scene()
    _, prims = binding.bvh_build(sc.triangles)
    a, b, c, md = c3_triangles(prims)
    parts = [slice(k, min(k + 8, N)) for k in range(0, N, 8)]
    with multiprocessing.Pool(args.jobs) as pool:
        res = pool.map(_job, [(a[s], b[s], c[s], md[s], prims) for s in parts])
    answers = {name: np.concatenate([r[k] for r in res]) for k, name in enumerate(ref.NAMES)}
    np.savez_compressed(args.out, digest=np.array(digest_of(prims)), a=a, b=b, c=c, max_dist=md, **answers)
    prim, dist2 = answers["prim"], answers["dist2"]
    print(f"{args.out}: {int((prim >= 0).sum())} of {N} queries have a triangle within their bound, {int(((prim >= 0) & (dist2 == 0)).sum())} of them touch it,"
          f" codes {sorted(set(answers['feature'][prim >= 0].tolist()))}")


if __name__ == "__main__":
    main()
