"""Records tests/golden/box_c3.npz: 256 seeded boxes on C3's mesh (scenes.mesh_scene(), 996,882 triangles) and their answers by
the numpy restatement of tyr_query_box (tests/box_ref.py), brute force over every triangle: the box axes for all 255 M pairs, the
binary64 axes for the pairs they leave.  A one-off CPU run of a few seconds; no GPU is needed, and nothing comes from the code
under test.

Three quarters of the boxes lie round points within 0.5 of the surface, a quarter anywhere in the root box inflated by 10 %; the
half extents run from 0.01 to 3 units per axis (the mesh's triangles have edges of about 0.14), and every sixteenth box is flat
on one axis.  The file holds the boxes, their counts and first 32 indices and a digest of the triangle array they belong to;
tests/test_box_query.py::test_c3_tree checks the digest and recomputes one box by brute force on every run.

    python tools/box_c3_golden.py [--out tests/golden/box_c3.npz]
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from query_bench_common import c3_points  # noqa: E402

N = 256
K = 32
F = np.float32


def c3_boxes(nodes, prims):
    pts = c3_points(nodes, prims, N)
    c = np.where((np.arange(N) % 4 == 3)[:, None], pts["uniform"], pts["surface"])
    rng = np.random.default_rng(32)
    half = (10.0 ** rng.uniform(-2.0, 0.5, (N, 3))).astype(F)
    half[np.arange(0, N, 16), rng.integers(0, 3, N // 16)] = 0
    return (c - half).astype(F), (c + half).astype(F)


def digest_of(prims):
    return hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "box_c3.npz"))
    args = ap.parse_args()

    import box_ref as ref
    from tyrant_amd import binding, scenes

    sc = scenes.mesh_scene()
    nodes, prims = binding.bvh_build(sc.triangles)
    lo, hi = c3_boxes(nodes, prims)
    count, prim = ref.box(lo, hi, prims, K)
    np.savez_compressed(args.out, digest=np.array(digest_of(prims)), lo=lo, hi=hi, count=count, prim=prim)
    print(f"{args.out}: {int((count == 0).sum())} of {N} boxes touch nothing, {int((count > K).sum())} more than {K} triangles, the largest {int(count.max())}")


if __name__ == "__main__":
    main()
