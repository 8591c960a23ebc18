"""Records tests/golden/tri_c3.npz: 256 seeded query triangles on C3's mesh (scenes.mesh_scene(), 996,882 triangles) and their
answers by the numpy restatement of tyr_query_tri (tests/tri_ref.py), brute force over every triangle: the coordinate axes for all
255 M pairs, the binary64 axes for the pairs they leave.  A one-off CPU run of a few seconds; no GPU is needed, and nothing comes
from the code under test.

Three quarters of the triangles lie round points within 0.5 of the surface, a quarter anywhere in the root box inflated by 10 %;
every corner lies within 0.03 to 12.6 units of its point, one size per triangle (the mesh's triangles have edges of about 0.35), and
every sixteenth query is a triangle of the mesh itself.  The file holds the queries, their counts and first 32 indices and a
digest of the triangle array they belong to; tests/test_tri_query.py::test_c3_tree checks the digest and recomputes one query by
brute force on every run.

    python tools/tri_c3_golden.py [--out tests/golden/tri_c3.npz]
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


def c3_triangles(nodes, prims, corners):
    pts = c3_points(nodes, prims, N)
    centre = np.where((np.arange(N) % 4 == 3)[:, None], pts["uniform"], pts["surface"])
    rng = np.random.default_rng(33)
    size = (10.0 ** rng.uniform(-1.5, 1.1, (N, 1))).astype(F)
    a, b, c = ((centre + rng.uniform(-1, 1, (N, 3)) * size).astype(F) for _ in range(3))
    own = rng.integers(0, len(prims), N // 16)
    a[::16], b[::16], c[::16] = (x[own].astype(F) for x in corners)
    return a, b, c


def digest_of(prims):
    return hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tri_c3.npz"))
    args = ap.parse_args()

    import tri_ref as ref
    from tyrant_amd import binding, scenes

    sc = scenes.mesh_scene()
    nodes, prims = binding.bvh_build(sc.triangles)
    a, b, c = c3_triangles(nodes, prims, ref.corners(*ref.records(prims)))
    count, prim = ref.tri(a, b, c, prims, K)
    np.savez_compressed(args.out, digest=np.array(digest_of(prims)), a=a, b=b, c=c, count=count, prim=prim)
    fits = int(((count > 0) & (count <= K)).sum())
    print(f"{args.out}: {int((count == 0).sum())} of {N} triangles touch nothing, {fits} at most {K} triangles, {int((count > K).sum())} more, the largest {int(count.max())}")


if __name__ == "__main__":
    main()
