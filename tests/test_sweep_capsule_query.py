"""Batched swept-capsule queries on the uploaded scene (tyr_query_sweep_capsule, hip/sweep_capsule.hip;
Renderer.query_sweep_capsule): the first contact of include/tyr_c.h "Swept-capsule queries" as an argmin over all triangles,
bit for bit against its numpy restatement (tests/sweep_capsule_ref.py) by brute force -- the definition has no traversal order
in it, so nothing else is needed as an oracle.

CPU: the restatement by hand, the restatement against a sampled-and-bisected binary64 truth and against the swept sphere's for
p == q, the pruning key against the value, what the fixtures are for, what the compiler made of the kernel, the ABI.  GPU:
lattices with shared edges and vertices, exact ties by index, over-long leaves, offset scenes and slivers, radii and tmax,
hostile input, batch sizes, optional outputs, isolation from the render, refit, streams, argument checks, and one pass on C3's
1 M-triangle tree."""
import ctypes as C
import functools
import hashlib
import os
import re

import numpy as np
import pytest

import sweep_capsule_ref as ref
import sweep_ref
from conftest import GOLDEN, ROOT, bits, built_scene
from query_support import (OFFSET, assert_kernel_budget, assert_query_abi, assert_render_undisturbed, box_points, build, deformed, duplicated, lattice, launch_bounds_blocks,
                           no_triangles, offset_soup, on_side_stream, query_exists, renderer, stack40, surface_points, tri)
from query_support import same as same_outputs

F = np.float32
D = np.float64
C3_ANSWERS = os.path.join(GOLDEN, "sweep_capsule_c3.npz")
NAMES = ref.NAMES
# |t - truth| of the restatement on the committed seeds (test_restatement_against_truth prints it; DESIGN.md "Swept-capsule
# queries" has the table): the worst family's value, asserted with 4x room for other seeds
WORST_T_ERROR = 3.7e-12
SWEEP_T_ERROR = 4e-12  # what include/tyr_c.h "Swept-sphere queries" states for the swept sphere's own value
CELL = 100.0 / 32  # heightfield(32)'s grid step

_the_query_exists = query_exists("tyr_query_sweep_capsule")


# ---- fixtures (numpy only) --------------------------------------------------------------------------------------------
def aimed(rng, prims, n, radii=(0.0, 0.05, 0.5, 4.0), lengths=(0.0, 0.5, 1.0, 2.0, 4.0, 16.0), unit_len=CELL):
    """seeded capsules whose p starts in the inflated root box and moves towards points near the surface, some stopping short,
    some passing through; the axis has a seeded direction and one of `lengths` (in units of unit_len)"""
    p = box_points(rng, prims, n)
    target = surface_points(rng, prims, n, 0.5)
    d = ((target - p) * rng.uniform(0.3, 1.7, (n, 1))).astype(F)
    axis = rng.normal(size=(n, 3))
    axis *= (rng.choice(np.array(lengths), (n, 1)) * unit_len) / np.linalg.norm(axis, axis=1, keepdims=True)
    q = (p + axis).astype(F)
    r = rng.choice(np.array(radii, F), n).astype(F)
    return p, q, d, r


@functools.lru_cache(maxsize=None)
def lattice_case():
    """heightfield(32): a capsule dropped onto every grid vertex with its axis along a grid line (one, two or no cells long, in
    +-x or +-y), and seeded capsules -- (nodes, prims, capsules, answers)"""
    nodes, prims, grid, _ = lattice(32, 21)
    rng = np.random.default_rng(51)
    g = len(grid)
    drop = np.tile(np.array([0, 0, -60], F), (g, 1))
    step = np.zeros((g, 3), F)
    step[np.arange(g), rng.integers(0, 2, g)] = (rng.choice(np.array([-2.0, -1.0, 0.0, 1.0, 2.0]), g) * CELL).astype(F)
    sp, sq, sd, sr = aimed(rng, prims, 448)
    p, q, d = np.concatenate([grid, sp]), np.concatenate([(grid + step).astype(F), sq]), np.concatenate([drop, sd])
    r = np.concatenate([rng.choice(np.array([0.0, 0.25, 2.0, 5.0], F), g).astype(F), sr])
    tmax = np.concatenate([np.ones(g, F), rng.choice(np.array([0.0, 0.5, 1.0, 1.0, 2.0], F), len(sp)).astype(F)])
    caps = tuple(np.ascontiguousarray(a) for a in (p, q, d, r, tmax))
    return nodes, prims, caps, ref.sweep_capsule(p, q, d, r, prims, tmax)


@functools.lru_cache(maxsize=None)
def duplicated_case():
    nodes, prims, pts, _ = duplicated(22, 2048)
    rng = np.random.default_rng(52)
    n = 640
    p = pts[:n].copy()
    target = surface_points(rng, prims, n, 0.5)
    d = ((target - p) * rng.uniform(0.5, 1.5, (n, 1))).astype(F)
    axis = rng.normal(size=(n, 3)) * rng.choice([0.0, 2.0, 10.0], (n, 1))
    q = (p + axis).astype(F)
    r = rng.choice(np.array([0.0, 0.3, 3.0], F), n).astype(F)
    return nodes, prims, (p, q, d, r), ref.sweep_capsule(p, q, d, r, prims)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
S2 = float(np.sqrt(2.0))
T1, T2, T3, T4 = 0.75, 1 - 0.25 * S2, 0.75 - 0.125 * S2, 1 - 0.125 * S2
HAND = [  # vert (0,0,0), e1 (1,0,0), e2 (0,1,0), r = 0.5: p, q, d, t, s, feature, region, point -- one capsule per feature code
    ((0.25, 0.25, 2), (0.25, 0.25, 3), (0, 0, -2), T1, 0, 0, 0, (0.25, 0.25, 0)),
    ((0.25, 0.25, 3), (0.25, 0.25, 2), (0, 0, -2), T1, 1, 1, 0, (0.25, 0.25, 0)),
    ((0.5, -2, -1), (0.5, -2, 1), (0, 2, 0), T1, 0.5, 2, 4, (0.5, 0, 0)),
    ((-2, 0.5, -1), (-2, 0.5, 1), (2, 0, 0), T1, 0.5, 3, 5, (0, 0.5, 0)),
    ((2, 2, -1), (2, 2, 1), (-2, -2, 0), T3, 0.5, 4, 6, (0.5, 0.5, 0)),
    ((-1, -1, 0), (-2, -2, 0), (1, 1, 0), T2, 0, 5, 1, (0, 0, 0)),  # (the lateral edge from A begins there at the same t: the lower code)
    ((2, -1, 0), (3, -2, 0), (-1, 1, 0), T2, 0, 6, 2, (1, 0, 0)),
    ((-1, 2, 0), (-2, 3, 0), (1, -1, 0), T2, 0, 7, 3, (0, 1, 0)),
    ((-2, -2, 0), (-1, -1, 0), (1, 1, 0), T2, 1, 8, 1, (0, 0, 0)),
    ((3, -2, 0), (2, -1, 0), (-1, 1, 0), T2, 1, 9, 2, (1, 0, 0)),
    ((-2, 3, 0), (-1, 2, 0), (1, -1, 0), T2, 1, 10, 3, (0, 1, 0)),
    ((0.5, -2, 0), (0.5, -3, 0), (0, 2, 0), T1, 0, 11, 4, (0.5, 0, 0)),  # a in the triangle's plane
    ((-2, 0.5, 0), (-3, 0.5, 0), (2, 0, 0), T1, 0, 12, 5, (0, 0.5, 0)),
    ((2, 2, 0), (3, 3, 0), (-2, -2, 0), T3, 0, 13, 6, (0.5, 0.5, 0)),
    ((0.5, -3, 0), (0.5, -2, 0), (0, 2, 0), T1, 1, 14, 4, (0.5, 0, 0)),
    ((-3, 0.5, 0), (-2, 0.5, 0), (2, 0, 0), T1, 1, 15, 5, (0, 0.5, 0)),
    ((3, 3, 0), (2, 2, 0), (-2, -2, 0), T3, 1, 16, 6, (0.5, 0.5, 0)),
    ((-2, -2, -1), (-2, -2, 1), (2, 2, 0), T4, 0.5, 17, 1, (0, 0, 0)),
    ((3, -2, -1), (3, -2, 1), (-2, 2, 0), T4, 0.5, 18, 2, (1, 0, 0)),
    ((-2, 3, -1), (-2, 3, 1), (2, -2, 0), T4, 0.5, 19, 3, (0, 1, 0)),
]


def test_hand_cases():
    """exactly representable numbers on the unit right triangle: one capsule per feature code, an initial overlap by the axis's
    middle, an equal-t tie, grazing at exactly r and one binary32 step beyond, moving away, p == q, a needle, d == 0, a in the
    plane and along an edge, the zero triangle, tmax inclusive, the argmin, every invalid input"""
    unit = tri((0, 0, 0), (1, 0, 0), (0, 1, 0))

    def one(p, q, d, r, tmax=None, prims=unit):
        res = ref.sweep_capsule(np.array([p], F), np.array([q], F), np.array([d], F), F(r), prims, None if tmax is None else np.array([tmax], F))
        return tuple(a[0] for a in res)

    for p, q, d, t, s, feature, region, point in HAND:
        gt, prim, gs, fe, reg, pt, cen, nrm = one(p, q, d, 0.5)
        assert prim == 0 and (int(fe), int(reg), float(gs)) == (feature, region, s) and abs(float(gt) - t) <= 6e-8 * t, (p, float(gt), int(fe))
        axis_point = np.array(p) + s * (np.array(q) - np.array(p)) + float(gt) * np.array(d)
        assert np.allclose(pt, point, atol=1e-7) and np.allclose(cen, axis_point, atol=1e-6), p
        assert abs(float(np.linalg.norm(nrm.astype(D))) - 1) < 1e-6 and np.allclose(cen - pt, 0.5 * nrm, atol=1e-6), p
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.25, 0.25, 3), (0.25, 0.25, 2), (0, 0, -2), 0.5)
    assert (float(gt), pt.tolist(), cen.tolist(), nrm.tolist()) == (0.75, [0.25, 0.25, 0], [0.25, 0.25, 0.5], [0, 0, 1])
    # an initial overlap by the axis's middle: the axis crosses the face, both ends farther than r from the triangle
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.25, 0.25, -1), (0.25, 0.25, 1), (0, 0, -2), 0.5)
    assert (float(gt), prim, float(gs), int(fe), int(reg), pt.tolist(), cen.tolist(), nrm.tolist()) == (0.0, 0, 0.5, 0, 0, [0.25, 0.25, 0], [0.25, 0.25, 0], [0, 0, 0])
    # an initial overlap by an end: the closest-segment value's s, point and region; the normal's length is distance / r
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.25, 0.25, 0.25), (0.25, 0.25, 3), (0, 0, -2), 0.5)
    assert (float(gt), prim, float(gs), int(fe), int(reg), pt.tolist(), cen.tolist(), nrm.tolist()) == (0.0, 0, 0.0, 0, 0, [0.25, 0.25, 0], [0.25, 0.25, 0.25], [0, 0, 0.5])
    # an equal-t tie keeps the lower code: the cap edge A -> B (11) and its copy moved by -a (14), a parallel to the edge
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.25, -2, 0), (0.75, -2, 0), (0, 2, 0), 0.5)
    assert (float(gt), prim, float(gs), int(fe), int(reg), pt.tolist()) == (0.75, 0, 0.0, 11, 4, [0.25, 0, 0])
    # past the edge A -> B at exactly r: touched; one binary32 step farther out: a miss
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.5, -0.5, -2), (0.5, -1.5, -2), (0, 0, 4), 0.5)
    assert (float(gt), prim, float(gs), int(fe), int(reg), pt.tolist()) == (0.5, 0, 0.0, 11, 4, [0.5, 0, 0])
    out = float(np.nextafter(F(-0.5), F(-1)))
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.5, out, -2), (0.5, -1.5, -2), (0, 0, 4), 0.5)
    assert (float(gt), prim, float(gs), int(fe), int(reg)) == (1.0, -1, 0.0, 0, 0) and cen.tolist() == pt.tolist() == [0.5, out, 2.0] and not nrm.any()
    # moving away
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.25, 0.25, 2), (0.25, 0.25, 3), (0, 0, 2), 0.5)
    assert (float(gt), prim, cen.tolist()) == (1.0, -1, [0.25, 0.25, 4])
    # p == q: the sphere's own candidates, the moved copies tie and lose
    for (p, q, d, t, s, feature, region, point), code in ((HAND[0], 0), (HAND[5], 5), (HAND[11], 11)):
        gt, prim, gs, fe, reg, pt, cen, nrm = one(p, p, d, 0.5)
        assert (prim, float(gs), int(fe), int(reg)) == (0, 0.0, code, region) and abs(float(gt) - t) <= 6e-8
    # r == 0: a needle across the edge A -> B is a side face's; a point (p == q, r == 0) from either side
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.5, -1, -1), (0.5, -1, 1), (0, 2, 0), 0.0)
    assert (float(gt), prim, float(gs), int(fe), int(reg), pt.tolist(), cen.tolist()) == (0.5, 0, 0.5, 2, 4, [0.5, 0, 0], [0.5, 0, 0]) and not nrm.any()
    for z in (2.0, -2.0):
        gt, prim, gs, fe, reg, pt, cen, nrm = one((0.25, 0.25, z), (0.25, 0.25, z), (0, 0, -2 * z), 0.0)
        assert (float(gt), prim, int(fe), int(reg), pt.tolist(), cen.tolist()) == (0.5, 0, 0, 0, [0.25, 0.25, 0], [0.25, 0.25, 0]) and not nrm.any()
    # d == 0: only the overlap rule
    assert [int(x) for x in one((0.25, 0.25, 0.25), (0.25, 0.25, 3), (0, 0, 0), 0.5)[:2]] == [0, 0]
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.25, 0.25, 0.25), (0.25, 0.25, 3), (0, 0, 0), 0.125)
    assert (float(gt), prim, cen.tolist(), pt.tolist()) == (1.0, -1, [0.25, 0.25, 0.25], [0.25, 0.25, 0.25])
    # the zero triangle: its one point, as its first vertex (5; 6, 7 and the cap edges tie or fail)
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0, 0, 2), (0, 0, 3), (0, 0, -2), 0.5, prims=tri((0, 0, 0), (0, 0, 0), (0, 0, 0)))
    assert (float(gt), prim, float(gs), int(fe), int(reg), pt.tolist()) == (0.75, 0, 0.0, 5, 1, [0, 0, 0])
    # tmax is inclusive; one step below the contact: none, with the end of p's shortened path
    below = float(np.nextafter(F(0.75), F(0)))
    assert [int(one((0.25, 0.25, 2), (0.25, 0.25, 3), (0, 0, -2), 0.5, tm)[1]) for tm in (0.75, below, 0.0)] == [0, -1, -1]
    gt, prim, gs, fe, reg, pt, cen, nrm = one((0.25, 0.25, 2), (0.25, 0.25, 3), (0, 0, -2), 0.5, below)
    assert float(gt) == below and cen.tolist() == pt.tolist() == [0.25, 0.25, float(F(2.0 - 2.0 * below))]
    # the argmin: the lowest index of equal t32; every invalid input
    three = np.concatenate([tri((0, 0, 5), (1, 0, 0), (0, 1, 0)), unit, unit])
    nan, inf = np.nan, np.inf
    n = 14
    p = np.array([[0.25, 0.25, 2]] * n, F)
    q = np.array([[0.25, 0.25, 3]] * n, F)
    d = np.array([[0, 0, -2]] * n, F)
    r = np.full(n, 0.5, F)
    tm = np.ones(n, F)
    p[1, 0], p[2, 2], q[3, 1], q[4, 0], d[5, 1], d[6, 0] = nan, -inf, nan, inf, nan, -inf
    r[7], r[8], r[9] = nan, -1.0, inf
    tm[10], tm[11], tm[12] = nan, -1.0, inf
    r[13] = -0.0  # (a negative zero is zero: valid)
    gt, prim, gs, fe, reg, pt, cen, nrm = ref.sweep_capsule(p, q, d, r, three, tm)
    assert prim.tolist() == [1] + [-1] * 12 + [1] and float(gt[0]) == 0.75 and np.isposinf(gt[1:13]).all()
    assert np.array_equal(bits(cen[1:13]), bits(p[1:13])) and np.array_equal(bits(pt[1:13]), bits(p[1:13]))
    assert not nrm[1:13].any() and not reg.any() and not fe.any() and not gs.any()
    assert ref.sweep_capsule(p[:1], q[:1], d[:1], r[:1], three[:0])[1].tolist() == [-1]  # no triangles: none


MEAN_EDGE = 0.35  # of C3's mesh, the scale of the bench's axis lengths


def _families(rng, n):
    """(name, p, q, d, r, tmax, vert, e1, e2) of seeded pairs: triangles with edges of about MEAN_EDGE, axis lengths of 1, 4 and 16
    mean edges at r = 0 and r = 0.1 (tools/sweep_capsule_bench.py's), and the middle one moved by 4096"""
    for length in (1.0, 4.0, 16.0):
        for radius in (0.0, 0.1):
            for off in ((0.0, 4096.0) if (length, radius) == (4.0, 0.1) else (0.0,)):
                vert = (rng.uniform(-50, 50, (n, 3)) + off).astype(F)
                e1, e2 = (rng.uniform(-MEAN_EDGE, MEAN_EDGE, (n, 3)).astype(F) for _ in range(2))
                u = rng.random((n, 1))
                v = rng.random((n, 1)) * (1 - u)
                on_tri = vert.astype(D) + u * e1 + v * e2
                axis = rng.normal(size=(n, 3))
                axis *= length * MEAN_EDGE / np.linalg.norm(axis, axis=1, keepdims=True)
                mid = on_tri + rng.normal(size=(n, 3)) * 1.0
                target = on_tri + axis * rng.uniform(-0.5, 0.5, (n, 1)) + rng.normal(size=(n, 3)) * (0.08 + 0.5 * radius)
                p, q = (mid - 0.5 * axis).astype(F), (mid + 0.5 * axis).astype(F)
                d = ((target - mid) * rng.uniform(0.5, 1.6, (n, 1))).astype(F)
                tmax = rng.choice(np.array([0.5, 1.0, 1.0, 2.0], F), n).astype(F)
                yield f"axis {length:g}, r {radius:g}" + (", moved by 4096" if off else ""), p, q, d, np.full(n, radius, F), tmax, vert, e1, e2


def test_restatement_against_truth():
    """the restatement against the clearance of the moved axis (segment_ref's pair distance minus r, restated in plain numpy)
    sampled along the path (1,000 samples) and bisected: hit or miss agrees on every pair whose truth does not graze (least
    clearance within 1e-9 of r, a needle that crosses excepted: its clearance is 0 on a whole interval; at most 1 % of a
    family), and t agrees within 4x the worst error the committed seeds give.  The contact lies at r from the axis point."""
    rng = np.random.default_rng(9)
    worst, excluded, gaps, features = {}, {}, {}, set()
    for name, p, q, d, r, tmax, vert, e1, e2 in _families(rng, 400):
        hit, t, s, feature, region, point = ref.pair_value(p, q, d, r, tmax, vert, e1, e2)
        tt, least = ref.truth(p, q, d, r, tmax, vert, e1, e2)
        graze = (np.abs(least) < 1e-9) & ~((r == 0) & (least == 0))
        excluded[name] = float(graze.mean())
        assert excluded[name] <= 0.01, (name, excluded)
        ok = ~graze
        wrong = ok & (hit != np.isfinite(tt))
        assert not wrong.any(), (name, np.nonzero(wrong)[0][:5], least[wrong][:5])
        both = ok & hit
        assert both.sum() >= 60, (name, int(both.sum()))
        worst[name] = float(np.abs(t[both] - tt[both]).max())
        moving = both & (t > 0)
        pd, qd = p.astype(D), q.astype(D)
        cen = (pd + s[:, None] * (qd - pd)) + t[:, None] * d.astype(D)
        gap = np.abs(np.linalg.norm(cen - point, axis=1) - r.astype(D))[moving]
        assert gap.max() <= 1e-9, (name, gap.max())
        gaps[name] = float(gap.max())
        features |= set(np.unique(feature[moving]).tolist())
    print("worst |t - truth| per family:", worst, "worst | |center - point| - r |:", gaps, "grazing fraction excluded:", excluded, "features:", sorted(features))
    assert max(worst.values()) <= 4 * WORST_T_ERROR, worst


def test_a_point_axis_is_the_swept_sphere():
    """p == q against sweep_ref.sweep on a soup: the same prim; t differs by no more than the restatement's worst error against
    the truth plus the 4e-12 the swept sphere's header states for its own (the two share the candidates' operations, but an
    initial overlap is found by the closest-segment rules here and by the closest-point rules there)"""
    from tyrant_amd import scenes

    prims = scenes.random_soup(300)
    rng = np.random.default_rng(53)
    n = 400
    p = box_points(rng, prims, n)
    d = ((surface_points(rng, prims, n, 0.5) - p) * rng.uniform(0.3, 1.7, (n, 1))).astype(F)
    r = rng.choice(np.array([0.0, 0.05, 0.5, 4.0], F), n).astype(F)
    t, prim, s, feature, region, point, center, normal = ref.sweep_capsule(p, p, d, r, prims)
    st, sprim, sregion, spoint, scenter, snormal = sweep_ref.sweep(p, d, r, prims)
    assert np.array_equal(prim, sprim) and (prim >= 0).sum() >= n // 4 and (prim < 0).sum() >= n // 20
    assert np.abs(t.astype(D) - st.astype(D)).max() <= WORST_T_ERROR + SWEEP_T_ERROR
    assert set(np.unique(feature).tolist()) <= {0, 5, 6, 7, 11, 12, 13} and not s.any() and np.array_equal(region, sregion)


def test_shortlist_keeps_every_winner():
    """the restatement with and without its box cull: the same eight outputs, on part of the lattice fixture"""
    nodes, prims, (p, q, d, r, tmax), want = lattice_case()
    pick = np.concatenate([np.arange(0, 1089, 9), np.arange(1089, 1089 + 448, 3)])
    full = ref.sweep_capsule(p[pick], q[pick], d[pick], r[pick], prims, tmax[pick], cull=False)
    same(full, tuple(a[pick] for a in want), "with and without the cull")


def test_pruning_key_never_passes_the_value_of_a_triangle_in_the_box():
    """hip/sweep_capsule.hip skips a box when the path of p misses the box grown by r + max(a_k, 0) below and r + max(-a_k, 0) above
    and widened by kCapsuleSlack * (|p_k| + max(|lo1_k|, |hi1_k|)) per plane, leaves it before 0 or enters it after `best`.  On a
    triangle's own three-corner box no pair with a value may be skipped with best = its t32, for scenes at the origin and moved by
    OFFSET and by 65536, near and far starts, axis-parallel directions, axis lengths up to 16 and r from 0 to 2; every larger box
    is entered earlier and left later.  What the un-widened test would have needed, over what the widening gives, stays below
    one half (DESIGN.md "Swept-capsule queries": 3.2x by derivation)."""
    src = open(os.path.join(ROOT, "tyrant_amd", "csrc", "hip", "sweep_capsule.hip")).read()
    slack = float(re.search(r"kCapsuleSlack = ([0-9.]+)f \* kCapsuleUlp;", src).group(1)) * float(re.search(r"kCapsuleUlp = ([0-9.e-]+)f;", src).group(1))
    assert 2.0 ** -24 <= slack <= 2.0 ** -16
    rng = np.random.default_rng(10)
    n = 20000
    worst, hits = {}, 0
    for off in (np.zeros(3), OFFSET.astype(D), np.full(3, 65536.0)):
        for far_start in (False, True):
            vert = (rng.uniform(-50, 50, (n, 3)) + off).astype(F)
            e1, e2 = (rng.uniform(-1.5, 1.5, (n, 3)).astype(F) for _ in range(2))
            p = (vert + rng.normal(size=(n, 3)) * (60.0 if far_start else 3.0)).astype(F)
            axis = rng.normal(size=(n, 3))
            axis *= rng.choice([0.0, 0.35, 1.4, 5.6, 16.0], (n, 1)) / np.linalg.norm(axis, axis=1, keepdims=True)
            axis[rng.random(n) < 0.2, rng.integers(0, 3)] = 0
            q = (p + axis).astype(F)
            u = rng.random((n, 1))
            target = vert.astype(D) + u * e1 + rng.random((n, 1)) * (1 - u) * e2 + rng.normal(size=(n, 3)) * 0.5 - axis * rng.random((n, 1))
            d = ((target - p) * rng.uniform(0.5, 1.6, (n, 1))).astype(F)
            kind = rng.integers(0, 8, n)  # three eighths of the directions parallel to an axis, another eighth to a plane
            for k in range(3):
                d[(kind != k) & (kind < 3), k] = 0
            d[kind == 3, 0] = 0
            r = (rng.uniform(0, 2, n) * (rng.random(n) > 0.1)).astype(F)
            tmax = np.ones(n, F)
            hit, t = ref.pair_value(p, q, d, r, tmax, vert, e1, e2)[:2]
            t32 = t[hit].astype(F)
            b, c = (vert + e1).astype(F), (vert + e2).astype(F)
            lo, hi = np.minimum(np.minimum(vert, b), c)[hit], np.maximum(np.maximum(vert, b), c)[hit]
            near0, far0, _ = ref.key32(p[hit], q[hit], d[hit], r[hit], t32, lo, hi, 0.0)
            near, far, visited = ref.key32(p[hit], q[hit], d[hit], r[hit], t32, lo, hi, slack)
            assert visited.all(), (off.tolist(), far_start, int((~visited).sum()))
            assert (near <= t32).all()  # the key itself: a lower bound of the value
            with np.errstate(all="ignore"):
                need = np.maximum.reduce([(near0 - t32) / (near0 - near), -far0 / (far - far0), (near0 - far0) / ((near0 - near) + (far - far0))])
            need = np.where(np.isfinite(need), np.maximum(need, 0.0), 0.0)
            worst[(float(off[0]), far_start)] = float(need.max())
            hits += int(hit.sum())
    print("needed widening / widening:", worst, "pairs with a value:", hits)
    assert hits >= 30000 and max(worst.values()) <= 0.5, worst


def test_fixtures_reach_what_they_are_for():
    """every feature code wins somewhere; bit-equal t32 ties exist (the duplicated scene: all of them); initial overlaps, misses
    and contacts behind tmax exist; the lattice's tree needs more stack than the 12 LDS entries; stack40 has an over-long leaf"""
    from tyrant_amd import binding

    nodes, prims, (p, q, d, r, tmax), (t, prim, s, feature, region, _, _, _) = lattice_case()
    moving = (prim >= 0) & (t > 0)
    assert set(np.unique(feature[moving]).tolist()) == set(range(20)), sorted(set(range(20)) - set(np.unique(feature[moving]).tolist()))
    assert set(np.unique(region[prim >= 0]).tolist()) == set(range(7))
    assert ((prim >= 0) & (t == 0)).sum() >= 20 and (prim < 0).sum() >= 20 and ((s > 0) & (s < 1) & moving).sum() >= 20
    sub = np.nonzero(prim < 0)[0][:128]
    longer = ref.sweep_capsule(p[sub], q[sub], d[sub], r[sub], prims, (tmax[sub] * F(4) + F(1)).astype(F))
    assert (longer[1] >= 0).sum() >= 10  # a contact behind the end of the path
    _, _, ties = ref.brute_values(p[:256], q[:256], d[:256], r[:256], tmax[:256], prims)
    assert (ties >= 2).sum() >= 64  # a capsule dropped onto grid vertices touches all the triangles around them at once
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    nodes, prims, (p, q, d, r), (t, prim, _, _, _, _, _, _) = duplicated_case()
    _, arg, ties = ref.brute_values(p, q, d, r, np.ones(len(p), F), prims)
    assert (arg >= 0).sum() >= 200 and (ties[arg >= 0] >= 2).all()
    nodes, prims = build(stack40())
    assert nodes["primitiveCount"].max() == 40  # an over-long leaf: synthetic records


def test_sweep_capsule_kernel_keeps_registers_and_lds_in_budget():
    """exactly one k_query_sweep_capsule; no vector spills; scratch no larger than the LdsStack's private spill arrays (52 entries
    of 8 bytes, plus the frame's alignment: the compile reports 432 bytes); LDS (24,576 + 7,168 bytes) that admits the two blocks
    per CU the launch bounds plan for.  The occupancy reached is printed (DESIGN.md "Swept-capsule queries" records it)."""
    assert_kernel_budget("sweep_capsule", "k_query_sweep_capsule", 1, (64 - 12) * 8 + 16, 24576 + 7168, planned=launch_bounds_blocks("sweep_capsule", "k_query_sweep_capsule"))


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_sweep_capsule", "tyr_sweep_capsule_out", hip.SweepCapsuleOut, 8)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, p, q, d, r, tmax=None, **kw):
    r = r if np.isscalar(r) else np.array(r)
    return tuple(x.cpu().numpy() for x in g.query_sweep_capsule(np.array(p), np.array(q), np.array(d), r, None if tmax is None else np.array(tmax), normal=True, **kw))


same = functools.partial(same_outputs, NAMES)


def check(g, prims, p, q, d, r, tmax=None, what=""):
    got = ask(g, p, q, d, r, tmax)
    want = ref.sweep_capsule(p, q, d, r, prims, tmax)
    same(got, want, what)
    return got, want


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lattice_and_ties(hip):
    """heightfield(32): a capsule dropped onto every grid vertex with its axis along a grid line (it touches the triangles around
    one or several vertices at once) and seeded capsules; radii 0, small and larger than a cell; axis lengths 0 to 16 cells;
    tmax 0, shorter than the contact, 1 and longer"""
    nodes, prims, (p, q, d, r, tmax), want = lattice_case()
    g = renderer(hip, nodes, prims)
    got = ask(g, p, q, d, r, tmax)
    same(got, want, "lattice")
    assert len(np.unique(got[3])) == 20 and (got[1] < 0).any() and (got[0] == 0).any()
    same(ask(g, p[:1089], q[:1089], d[:1089], r[:1089]), tuple(a[:1089] for a in want), "tmax NULL")  # (the drops' tmax is 1)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_exact_ties_resolve_to_the_lower_index(hip):
    """a scene concatenated with itself: every winner is the lower of the two copies' build-order indices; and 40 identical
    triangles (an over-long leaf behind synthetic records), alone and next to the Cornell box"""
    from tyrant_amd import scenes

    nodes, prims, (p, q, d, r), want = duplicated_case()
    twin = duplicated(22, 2048)[3]
    g = renderer(hip, nodes, prims)
    got = ask(g, p, q, d, r)
    same(got, want, "duplicated")
    prim = got[1][got[1] >= 0]
    assert prim.size >= 200 and (prim < twin[prim]).all()
    for tris in (stack40(), np.concatenate([scenes.cornell_box().triangles, stack40()])):
        nodes, prims = build(tris)
        g.upload(nodes, prims)
        sp, sq, sd, sr = aimed(np.random.default_rng(54), prims, 1000, unit_len=4.0)
        (_, prim, _, _, _, _, _, _), _ = check(g, prims, sp, sq, sd, sr, what="stack40")
        stack = np.nonzero((np.ascontiguousarray(prims).view(np.uint8).reshape(len(prims), -1) == np.ascontiguousarray(stack40()[:1]).view(np.uint8)).all(axis=1))[0]
        on_stack = np.isin(prim, stack)
        assert stack.size == 40 and on_stack.any() and (prim[on_stack] == stack.min()).all()  # the first of the identical records
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_scale_and_slack(hip):
    """a soup with slivers moved by (4096, -4096, 8192): capsules from within 1e-3 of the surface, from the root box and from
    half way to the origin; a quarter of the displacements parallel to an axis"""
    nodes, prims = offset_soup(True)
    rng = np.random.default_rng(55)
    p = np.concatenate([surface_points(rng, prims, 256, 1e-3), box_points(rng, prims, 384), (box_points(rng, prims, 128) - OFFSET * F(0.5)).astype(F)])
    n = len(p)
    d = ((surface_points(rng, prims, n, 0.5) - p) * rng.uniform(0.3, 1.7, (n, 1))).astype(F)
    kind = rng.integers(0, 12, n)
    for k in range(3):
        d[(kind != k) & (kind < 3), k] = 0
    axis = rng.normal(size=(n, 3))
    axis *= rng.choice([0.0, 0.5, 3.0, 12.0], (n, 1)) / np.linalg.norm(axis, axis=1, keepdims=True)
    q = (p + axis).astype(F)
    r = rng.choice(np.array([0.0, 0.01, 0.5, 3.0], F), n).astype(F)
    g = renderer(hip, nodes, prims)
    (t, prim, _, _, _, _, _, _), _ = check(g, prims, p, q, d, r, what="offset soup with slivers")
    assert (prim >= 0).sum() >= n // 4 and (prim < 0).sum() >= n // 20
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_radii_tmax_hostile_input_batch_sizes_and_optional_outputs(hip):
    """the Cornell box: capsules starting in overlap with several triangles (the corners), radii 0 to larger than the room, tmax 0,
    shorter than the contact, per capsule and NULL, zero and axis-parallel displacements, subnormal displacements with a huge
    tmax, NaN / infinite / negative input; n = 0 .. 4097 (65 feed chunks); a scene without triangles; every optional output NULL
    in turn"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    g = renderer(hip, nodes, prims)
    rng = np.random.default_rng(56)
    n = 4097
    lo, hi = nodes[0]["bounds"][0].astype(F), nodes[0]["bounds"][1].astype(F)
    p = (lo - 5 + (hi - lo + 10) * rng.random((n, 3))).astype(F)
    d = (rng.normal(size=(n, 3)) * rng.choice([1.0, 20.0, 150.0], (n, 1))).astype(F)
    axis = rng.normal(size=(n, 3)) * rng.choice([0.0, 1.0, 10.0, 60.0], (n, 1))
    r = rng.choice(np.array([0.0, 0.0, 0.5, 3.0, 10.0, 200.0], F), n).astype(F)
    tmax = rng.choice(np.array([0.0, 0.25, 1.0, 1.0, 3.0], F), n).astype(F)
    kind = rng.integers(0, 30, n)
    p[kind < 6] = np.round(p[kind < 6])  # whole numbers, some of them on the walls' planes
    for k in range(3):
        d[(kind < 6) & (kind % 3 != k), k] = 0  # parallel to an axis
        axis[(kind < 3) & (kind != k), k] = 0
    d[kind == 6] = 0
    corner = np.nonzero(kind == 7)[0]  # in a corner of the room: overlapping both triangles of up to three walls
    p[corner] = np.where(rng.random((corner.size, 3)) < 0.5, lo, hi) + rng.uniform(-0.4, 0.4, (corner.size, 3)).astype(F)
    r[corner] = 1.0
    q = (p + axis).astype(F)
    bad = np.array([np.nan, np.inf, -np.inf], F)
    for code, arr in ((8, p), (9, d), (12, q)):
        w = np.nonzero(kind == code)[0]
        arr[w, rng.integers(0, 3, w.size)] = bad[rng.integers(0, 3, w.size)]
    r[kind == 10] = rng.choice(np.array([np.nan, np.inf, -1.0, -0.0], F), (kind == 10).sum())
    tmax[kind == 11] = rng.choice(np.array([np.nan, np.inf, -1.0, -0.0], F), (kind == 11).sum())
    tiny = np.nonzero(kind == 13)[0]  # subnormal displacements: 1 / d_k is infinite, yet with this tmax p moves by some tenths of a unit
    d[tiny] = (rng.normal(size=(tiny.size, 3)) * 1e-39).astype(F)
    tmax[tiny] = F(3e38)
    want = ref.sweep_capsule(p, q, d, r, prims, tmax)
    invalid = np.isposinf(want[0])
    assert invalid.sum() >= n // 12 and (want[1][corner] >= 0).all() and (want[0][corner] == 0).all()
    assert ((np.abs(d[tiny]) < 2.0 ** -126) & (d[tiny] != 0)).any() and (want[1][tiny] >= 0).sum() >= 5
    got = ask(g, p, q, d, r, tmax)
    same(got, want, "cornell")
    m = 1000
    same(ask(g, p[:m], q[:m], d[:m], r[:m]), ref.sweep_capsule(p[:m], q[:m], d[:m], r[:m], prims), "tmax NULL")
    same(ask(g, p[:m], q[:m], d[:m], 3.0), ref.sweep_capsule(p[:m], q[:m], d[:m], F(3.0), prims), "a scalar radius")
    for k in (0, 1, 63, 64, 65):  # every prefix answers as the whole batch did
        same(ask(g, p[:k], q[:k], d[:k], r[:k], tmax[:k]), tuple(a[:k] for a in want), f"n = {k}")
    # each optional output NULL in turn, through the C call; the array not passed stays untouched, the others' bits are the same
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a[:m])).cuda()  # noqa: E731
    tp, tq, td, tr, tt = on(p), on(q), on(d), on(r), on(tmax)
    P = C.c_void_p
    dtypes = (torch.float32, torch.int32, torch.float32, torch.uint8, torch.uint8)
    for skip in range(2, 8):
        outs = [torch.full((m,), 7, dtype=dt).cuda() for dt in dtypes] + [torch.full((m, 3), 7, dtype=torch.float32).cuda() for _ in range(3)]
        torch.cuda.synchronize()
        out = hip.SweepCapsuleOut(*[None if k == skip else x.data_ptr() for k, x in enumerate(outs)])
        assert hip.lib().tyr_query_sweep_capsule(g.h, m, P(tp.data_ptr()), P(tq.data_ptr()), P(td.data_ptr()), P(tr.data_ptr()), P(tt.data_ptr()), 0, C.byref(out), None) == 0
        assert g.query_error() == 0
        res = [x.cpu().numpy() for x in outs]
        same([None if k == skip else x for k, x in enumerate(res)], [w[:m] for w in want], f"without {NAMES[skip]}")
        assert (res[skip] == 7).all(), NAMES[skip]
    # a scene without triangles: every valid capsule a miss
    g.upload(*no_triangles())
    same(ask(g, p, q, d, r, tmax), ref.sweep_capsule(p, q, d, r, prims[:0], tmax), "empty scene")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_sweep_capsule_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with capsule sweeps between its tyr_render calls: the same accumulation buffer and
    counters as without them"""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    rng = np.random.default_rng(57)
    n = 4000
    p = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(5, 80, n)], axis=1).astype(F)
    q = (p + rng.normal(size=(n, 3)) * 5).astype(F)
    d = (rng.normal(size=(n, 3)) * 40).astype(F)
    r = rng.uniform(0, 3, n).astype(F)
    want = ref.sweep_capsule(p, q, d, r, prims)

    def between(g):
        same(ask(g, p, q, d, r), want, "between two renders")
        ask(g, p, q, d, 0.0, np.full(n, 0.5, F))

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the answers to the refitted scene's; a torch side stream and the ctx's stream work; bad
    arguments are refused before any launch; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(16))
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    rng = np.random.default_rng(58)
    n = 800
    p, q, d, r = aimed(rng, prims, n, unit_len=100.0 / 16)
    check(g, prims, p, q, d, r, what="before the refit")
    moved = deformed(prims, 4.0)
    g.refit(moved)
    got, want = check(g, moved, p, q, d, r, what="after the refit")
    assert not np.array_equal(want[1], ref.sweep_capsule(p, q, d, r, prims)[1])
    # a side stream, device tensors taken in place; then the ctx's own stream (NULL) through the C call
    tp, tq, td, tr = (torch.from_numpy(a).cuda() for a in (p, q, d, r))
    tt = torch.full((n,), 0.5).cuda()
    res = on_side_stream(lambda side: g.query_sweep_capsule(tp, tq, td, tr, tt, normal=True, stream=side))
    half = ref.sweep_capsule(p, q, d, r, moved, np.full(n, 0.5, F))
    same(tuple(x.cpu().numpy() for x in res), half, "side stream")

    L, h, P = hip.lib(), g.h, C.c_void_p
    t, prim = torch.full((n,), 7.0).cuda(), torch.full((n,), 7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    rest = (None,) * 6
    ok = hip.SweepCapsuleOut(t.data_ptr(), prim.data_ptr(), *rest)
    pp, pq, pd, pr, pt = P(tp.data_ptr()), P(tq.data_ptr()), P(td.data_ptr()), P(tr.data_ptr()), P(tt.data_ptr())
    assert L.tyr_query_sweep_capsule(h, n, pp, pq, pd, pr, pt, 0, C.byref(ok), None) == 0
    assert g.query_error() == 0  # (waits for the ctx's stream)
    same((t.cpu().numpy(), prim.cpu().numpy()), half[:2], "the ctx's stream")
    before = prim.cpu().numpy().copy()
    inv = hip.TYR_ERR_INVALID
    assert L.tyr_query_sweep_capsule(None, 4, pp, pq, pd, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep_capsule(h, 4, None, pq, pd, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep_capsule(h, 4, pp, None, pd, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep_capsule(h, 4, pp, pq, None, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep_capsule(h, 4, pp, pq, pd, None, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep_capsule(h, 4, pp, pq, pd, pr, None, 0, None, None) == inv
    assert L.tyr_query_sweep_capsule(h, 4, pp, pq, pd, pr, None, 0, C.byref(hip.SweepCapsuleOut(None, prim.data_ptr(), *rest)), None) == inv
    assert L.tyr_query_sweep_capsule(h, 4, pp, pq, pd, pr, None, 0, C.byref(hip.SweepCapsuleOut(t.data_ptr(), None, *rest)), None) == inv
    assert L.tyr_query_sweep_capsule(h, 4, pp, pq, pd, pr, None, 1, C.byref(ok), None) == inv  # flags must be 0
    assert L.tyr_query_sweep_capsule(h, 1 << 31, pp, pq, pd, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep_capsule(h, 0, None, None, None, None, None, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_sweep_capsule(empty.h, 4, pp, pq, pd, pr, None, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_sweep_capsule(tp.double(), tq, td, tr)
    with pytest.raises(ValueError):
        g.query_sweep_capsule(tp, tq[:, :2].contiguous(), td, tr)
    with pytest.raises(ValueError):
        g.query_sweep_capsule(tp, tq, td, tr[:5])
    with pytest.raises(ValueError):
        g.query_sweep_capsule(tp, tq, td, tr, tt[:5])
    assert np.array_equal(prim.cpu().numpy(), before)  # the refused calls wrote nothing
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_c3_tree(hip):
    """one pass on C3's 1 M-triangle tree: the 256 capsules of tests/golden/sweep_capsule_c3.npz (p within 1.5 of the surface,
    axis lengths 0 to 16 mean edges, radii 0 to 1) against the winners tools/sweep_capsule_c3_golden.py recorded with the
    restatement.  Every run checks that the file belongs to these triangles, recomputes one capsule by brute force and
    evaluates the winners' other outputs from the restatement."""
    sc, nodes, prims = built_scene("mesh706")
    z = np.load(C3_ANSWERS)
    assert str(z["digest"]) == hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest(), "the recorded answers belong to other triangles"
    p, q, d, r, tmax, t, arg = (z[k] for k in ("p", "q", "directions", "radius", "tmax", "t", "prim"))
    assert len(p) == 256 and (arg >= 0).sum() >= 64 and (arg < 0).sum() >= 16
    live = int(np.random.default_rng(59).integers(0, 256))
    one = slice(live, live + 1)
    lb, la, _ = ref.brute_values(p[one], q[one], d[one], r[one], tmax[one], prims)
    assert int(la[0]) == int(arg[live]) and (la[0] < 0 or bits(lb)[0] == bits(t)[live])
    want = ref.answers(p, q, d, r, tmax, ref.valid_inputs(p, q, d, r, tmax), arg.astype(np.int64), prims)
    assert np.array_equal(bits(want[0]), bits(t))
    g = renderer(hip, nodes, prims)
    same(ask(g, p, q, d, r, tmax), want, "C3")
    assert g.query_error() == 0
    g.close()
