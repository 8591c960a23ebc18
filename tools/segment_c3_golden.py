"""Records tests/golden/segment_c3.npz: 256 seeded segments on C3's mesh (scenes.mesh_scene(), 996,882 triangles) and their seven
answers by the numpy restatement of tyr_query_segment (tests/segment_ref.py), brute force over every triangle its
triangle-inequality shortlist keeps.  A one-off CPU run of a few minutes of numpy (--jobs spreads the segments over processes).
No GPU is needed.

p lies within 1.5 of the surface (a seeded triangle's point plus a uniform offset); q = p + a seeded displacement whose length
class is one of 0 (p == q), 0.35 (a mean triangle edge), 1.4, 5.6 and 40; every fourth segment has a max_dist of 0.25.  The file
holds the segments, the answers and a digest of the triangle array they belong to; tests/test_segment_query.py::test_c3_tree
checks the digest, evaluates the winners' pairs from the restatement and recomputes one segment by brute force on every run.

    python tools/segment_c3_golden.py [--jobs 8] [--out tests/golden/segment_c3.npz]
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


def c3_segments(prims):
    rng = np.random.default_rng(33)
    p = surface_points(rng, prims, N, 1.5)
    d = rng.normal(size=(N, 3))
    d *= rng.choice([0.0, 0.35, 1.4, 5.6, 40.0], (N, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    md = np.full(N, np.inf, F)
    md[::4] = 0.25
    return p, (p + d).astype(F), md


def digest_of(prims):
    return hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest()


def _job(args):
    import segment_ref as ref

    p, q, md, prims = args
    return ref.segment(p, q, prims, md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "segment_c3.npz"))
    args = ap.parse_args()

    import segment_ref as ref
    from tyrant_amd import binding, scenes

    sc = scenes.mesh_scene()
    _, prims = binding.bvh_build(sc.triangles)
    p, q, md = c3_segments(prims)
    parts = [slice(k, min(k + 8, N)) for k in range(0, N, 8)]
    with multiprocessing.Pool(args.jobs) as pool:
        res = pool.map(_job, [(p[s], q[s], md[s], prims) for s in parts])
    answers = {name: np.concatenate([r[k] for r in res]) for k, name in enumerate(ref.NAMES)}
    np.savez_compressed(args.out, digest=np.array(digest_of(prims)), p=p, q=q, max_dist=md, **answers)
    prim, dist2 = answers["prim"], answers["dist2"]
    print(f"{args.out}: {int((prim >= 0).sum())} of {N} segments have a triangle within their bound, {int(((prim >= 0) & (dist2 == 0)).sum())} of them touch it")


if __name__ == "__main__":
    main()
