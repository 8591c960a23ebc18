"""Records tests/golden/sweep_c3.npz: 256 seeded sweeps on C3's mesh (scenes.mesh_scene(), 996,882 triangles) and their answers
by the numpy restatement of tyr_query_sweep (tests/sweep_ref.py), brute force over every triangle.  A one-off CPU run: 268 M pair
evaluations in binary64, about ten minutes of numpy on one core (--jobs spreads the sweeps over processes).  No GPU is needed.

The sweeps start within 1.5 of the surface (a seeded triangle's point plus a uniform offset), move by a seeded displacement of
up to 3 units per axis and have radii from 0 to 1; every eighth has a tmax of its own.  The file holds the sweeps, the winners
(t, prim) and a digest of the triangle array they belong to; tests/test_sweep_query.py::test_c3_tree checks the digest, evaluates
the winners' other outputs from the restatement and recomputes one sweep by brute force on every run.

    python tools/sweep_c3_golden.py [--jobs 8] [--out tests/golden/sweep_c3.npz]
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


def c3_sweeps(prims):
    rng = np.random.default_rng(31)
    o = surface_points(rng, prims, N, 1.5)
    d = rng.uniform(-3.0, 3.0, (N, 3)).astype(F)
    r = rng.uniform(0.0, 1.0, N).astype(F)
    r[::16] = 0
    tmax = np.ones(N, F)
    tmax[::8] = rng.uniform(0.0, 2.0, N // 8).astype(F)
    return o, d, r, tmax


def digest_of(prims):
    return hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest()


def _job(args):
    import sweep_ref as ref

    o, d, r, tmax, prims = args
    best, arg, _ = ref.brute_values(o, d, r, tmax, prims)
    return best, arg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sweep_c3.npz"))
    args = ap.parse_args()

    from tyrant_amd import binding, scenes

    sc = scenes.mesh_scene()
    _, prims = binding.bvh_build(sc.triangles)
    o, d, r, tmax = c3_sweeps(prims)
    parts = [slice(k, min(k + 8, N)) for k in range(0, N, 8)]
    with multiprocessing.Pool(args.jobs) as pool:
        res = pool.map(_job, [(o[p], d[p], r[p], tmax[p], prims) for p in parts])
    best = np.concatenate([b for b, _ in res])
    arg = np.concatenate([a for _, a in res]).astype(np.int32)
    t = np.where(arg >= 0, best, tmax).astype(F)
    np.savez_compressed(args.out, digest=np.array(digest_of(prims)), origins=o, directions=d, radius=r, tmax=tmax, t=t, prim=arg)
    print(f"{args.out}: {int((arg >= 0).sum())} of {N} sweeps touch the mesh, {int((t == 0).sum())} of them at the start")


if __name__ == "__main__":
    main()
