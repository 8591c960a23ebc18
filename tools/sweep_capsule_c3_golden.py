"""Records tests/golden/sweep_capsule_c3.npz: 256 seeded capsules on C3's mesh (scenes.mesh_scene(), 996,882 triangles) and
their answers by the numpy restatement of tyr_query_sweep_capsule (tests/sweep_capsule_ref.py), brute force over every triangle
whose box the capsule's swept box meets.  A one-off CPU run of about a minute of numpy.  No GPU is needed.

p lies within 1.5 of the surface (a seeded triangle's point plus a uniform offset); q = p + a seeded axis whose length is one of
0 (p == q), 1, 4 and 16 mean triangle edges (0.35); the displacement is up to 3 units per axis, the radius one of 0, 0.1, 0.5
and 1, tmax one of 0.5, 1 and 2.  The file holds the capsules, the answers and a digest of the triangle array they belong to;
tests/test_sweep_capsule_query.py::test_c3_tree checks the digest, evaluates the winners' pairs from the restatement and
recomputes one capsule by brute force on every run.

    python tools/sweep_capsule_c3_golden.py [--out tests/golden/sweep_capsule_c3.npz]
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

from query_bench_common import surface_points  # noqa: E402

N = 256
F = np.float32
MEAN_EDGE = 0.35


def c3_capsules(prims):
    rng = np.random.default_rng(34)
    p = surface_points(rng, prims, N, 1.5)
    axis = rng.normal(size=(N, 3))
    axis *= rng.choice([0.0, 1.0, 4.0, 16.0], (N, 1)) * MEAN_EDGE / np.linalg.norm(axis, axis=1, keepdims=True)
    d = rng.uniform(-3.0, 3.0, (N, 3)).astype(F)
    r = rng.choice(np.array([0.0, 0.0, 0.1, 0.1, 0.5, 1.0], F), N).astype(F)
    tmax = rng.choice(np.array([0.5, 1.0, 1.0, 2.0], F), N).astype(F)
    return p, (p + axis).astype(F), d, r, tmax


def digest_of(prims):
    return hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sweep_capsule_c3.npz"))
    args = ap.parse_args()

    import sweep_capsule_ref as ref
    from tyrant_amd import binding, scenes

    sc = scenes.mesh_scene()
    _, prims = binding.bvh_build(sc.triangles)
    p, q, d, r, tmax = c3_capsules(prims)
    answers = dict(zip(ref.NAMES, ref.sweep_capsule(p, q, d, r, prims, tmax)))
    np.savez_compressed(args.out, digest=np.array(digest_of(prims)), p=p, q=q, directions=d, radius=r, tmax=tmax, **answers)
    prim, t = answers["prim"], answers["t"]
    print(f"{args.out}: {int((prim >= 0).sum())} of {N} capsules touch the mesh, {int(((prim >= 0) & (t == 0)).sum())} of them at the start; "
          f"features {sorted(set(answers['feature'][(prim >= 0) & (t > 0)].tolist()))}")


if __name__ == "__main__":
    main()
