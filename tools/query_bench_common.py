"""What the query benchmarks (tools/{query,nearest,nearest_k,hits,occlusion,sweep,winding,box,tri,segment}_bench.py) share: the
summary of a launch's samples, the seeded point batches on C3's scene, a camera-like ray grid, the Morton order of a batch and the
loop that times the launches in turn.  tools/sweep_c3_golden.py, tools/box_c3_golden.py, tools/tri_c3_golden.py and
tools/segment_c3_golden.py take their starting points from here too, so nothing at module level needs a GPU or torch."""
from __future__ import annotations

import numpy as np


def stats(samples_ms, n, unit="items", count=False, spread="p10_p90"):
    """median and spread of a launch's event times and its rate in M<unit>/s; count: the report also carries n, under `unit`;
    spread: "p10_p90", or "min_max" (tools/query_bench.py's committed keys)"""
    s = np.asarray(samples_ms, dtype=np.float64)
    med = float(np.median(s))
    head = {unit: int(n)} if count else {}
    if spread == "min_max":
        lo, hi = float(s.min()), float(s.max())
        return {**head, "median_ms": med, "min_ms": lo, "max_ms": hi, f"m{unit}_s": n / med / 1e3, f"m{unit}_s_spread": [n / hi / 1e3, n / lo / 1e3]}
    p10, p90 = float(np.percentile(s, 10)), float(np.percentile(s, 90))
    return {**head, "median_ms": med, "p10_ms": p10, "p90_ms": p90, f"m{unit}_s": n / med / 1e3, f"m{unit}_s_p10_p90": [n / p90 / 1e3, n / p10 / 1e3]}


def surface_points(rng, prims, n, offset):
    """n points near the surface: a seeded triangle's point plus a uniform offset of at most `offset` per axis"""
    i = rng.integers(0, prims.shape[0], n)
    u = rng.random(n)
    v = rng.random(n) * (1 - u)
    return (prims["vert"][i] + u[:, None] * prims["e1"][i] + v[:, None] * prims["e2"][i] + rng.uniform(-offset, offset, (n, 3))).astype(np.float32)


def c3_points(nodes, prims, n=1 << 21):
    """the two seeded point batches on an uploaded scene (nodes, prims as build_upload returns them), always drawn in this order:
    "uniform" in the root box inflated by 10 %, "surface" within 0.5 of the surface"""
    rng = np.random.default_rng(2025)
    lo, hi = nodes[0]["bounds"][0].astype(np.float32), nodes[0]["bounds"][1].astype(np.float32)
    pad = (hi - lo) * np.float32(0.1)
    uniform = ((lo - pad) + (hi - lo + 2 * pad) * rng.random((n, 3))).astype(np.float32)
    return {"uniform": uniform, "surface": surface_points(rng, prims, n, 0.5)}


def camera_rays(cam, n_x=2048, n_y=1024):
    """(origins, directions) of an n_x x n_y grid of camera-like rays from the scene's camera"""
    ys, xs = np.meshgrid(np.linspace(-0.6, 0.6, n_y, dtype=np.float32), np.linspace(-0.9, 0.9, n_x, dtype=np.float32), indexing="ij")
    fwd, up = np.asarray(cam.direction, np.float32), np.asarray(cam.up, np.float32)
    right = np.cross(fwd, up).astype(np.float32)
    dirs = fwd[None, :] + xs.reshape(-1, 1) * right[None, :] + ys.reshape(-1, 1) * up[None, :]
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    return np.tile(np.asarray(cam.position, np.float32), (n_x * n_y, 1)), dirs


def morton_order(cells):
    """the permutation that sorts points along a 30-bit Morton curve; cells: (n, 3) integers in 0 .. 1023, each tool's own
    quantisation of its points"""
    q = np.asarray(cells).astype(np.uint64)

    def spread(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249

    return np.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2), kind="stable")


def timed_rounds(g, launches, stream, reps, after=None, rounds=None):
    """The launches (name -> a call that returns the C status) in turn, `reps` rounds behind two warm-up rounds, each launch timed with
    device events around it on `stream` and waited for: {name: [ms, ...]}.  after(name, rep): called behind each finished launch
    (the tools that read results on a warm-up round); rounds: {name: the number of rounds, warm-up included, that launch takes
    part in}.  Ends with the ctx's query error bits, which must be zero."""
    import torch

    from tyrant_amd import binding

    torch.cuda.synchronize()
    samples = {k: [] for k in launches}
    for rep in range(reps + 2):
        for name, launch in launches.items():
            if rounds is not None and rep >= rounds.get(name, reps + 2):
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            rc = launch()
            b.record(stream)
            if rc:
                raise binding.TyrError(rc, name)
            b.synchronize()
            if rep >= 2:
                samples[name].append(a.elapsed_time(b))
            if after is not None:
                after(name, rep)
    assert g.query_error() == 0
    return samples
