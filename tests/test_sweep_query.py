"""Batched swept-sphere queries on the uploaded scene (tyr_query_sweep, hip/sweep.hip; Renderer.query_sweep): the first contact
of include/tyr_c.h "Swept-sphere queries" as an argmin over all triangles, bit for bit against its numpy restatement
(tests/sweep_ref.py) by brute force -- the definition has no traversal order in it, so nothing else is needed as an oracle.

CPU: the restatement by hand, the restatement against a sampled-and-bisected binary64 truth, the pruning key against the
value, what the fixtures are for, what the compiler made of the kernel, the ABI.  GPU: lattices with shared edges and vertices,
exact ties by index, over-long leaves, offset scenes and slivers, radii and tmax, hostile input, batch sizes, optional outputs,
isolation from the render, refit, streams, argument checks, and one pass on C3's 1 M-triangle tree."""
import ctypes as C
import functools
import hashlib
import itertools
import os
import re

import numpy as np
import pytest

import sweep_ref as ref
from conftest import GOLDEN, ROOT, bits, built_scene
from query_support import (OFFSET, assert_kernel_budget, assert_query_abi, assert_render_undisturbed, box_points, build, deformed, duplicated, lattice, launch_bounds_blocks,
                           no_triangles, offset_soup, on_side_stream, renderer, stack40, surface_points, tri)
from query_support import same as same_outputs

F = np.float32
D = np.float64
C3_ANSWERS = os.path.join(GOLDEN, "sweep_c3.npz")
NAMES = ("t", "prim", "region", "point", "center", "normal")
# |t - truth| of the restatement on the committed seeds (test_restatement_against_truth prints it; DESIGN.md "Swept-sphere
# queries" has the table): the worst family's value, asserted with 4x room for other seeds
WORST_T_ERROR = 3.9e-12


# ---- fixtures (numpy only) --------------------------------------------------------------------------------------------
def aimed(rng, prims, n, radii=(0.0, 0.05, 0.5, 4.0)):
    """seeded sweeps from the inflated root box towards points near the surface, some stopping short, some passing through"""
    o = box_points(rng, prims, n)
    target = surface_points(rng, prims, n, 0.5)
    d = ((target - o) * rng.uniform(0.3, 1.7, (n, 1))).astype(F)
    r = rng.choice(np.array(radii, F), n).astype(F)
    return o, d, r


@functools.lru_cache(maxsize=None)
def lattice_case():
    """heightfield(32): a sphere dropped onto every grid vertex, and seeded sweeps -- (nodes, prims, sweeps, answers)"""
    nodes, prims, grid, _ = lattice(32, 21)
    rng = np.random.default_rng(41)
    drop = np.tile(np.array([0, 0, -60], F), (len(grid), 1))
    so, sd, sr = aimed(rng, prims, 448)
    o, d = np.concatenate([grid, so]), np.concatenate([drop, sd])
    r = np.concatenate([rng.choice(np.array([0.0, 0.25, 2.0, 5.0], F), len(grid)).astype(F), sr])
    tmax = np.concatenate([np.ones(len(grid), F), rng.choice(np.array([0.0, 0.5, 1.0, 1.0, 2.0], F), len(so)).astype(F)])
    sweeps = tuple(np.ascontiguousarray(a) for a in (o, d, r, tmax))
    return nodes, prims, sweeps, ref.sweep(o, d, r, prims, tmax)


@functools.lru_cache(maxsize=None)
def duplicated_case():
    nodes, prims, pts, _ = duplicated(22, 2048)
    rng = np.random.default_rng(42)
    n = 640
    o = pts[:n].copy()
    target = surface_points(rng, prims, n, 0.5)
    d = ((target - o) * rng.uniform(0.5, 1.5, (n, 1))).astype(F)
    r = rng.choice(np.array([0.0, 0.3, 3.0], F), n).astype(F)
    return nodes, prims, (o, d, r), ref.sweep(o, d, r, prims)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
S2 = float(np.sqrt(2.0))
HAND = [  # vert (0,0,0), e1 (1,0,0), e2 (0,1,0), r = 0.5: o, d, t, region, point
    ((0.25, 0.25, 2.0), (0, 0, -2), 0.75, 0, (0.25, 0.25, 0)),
    ((-1, -1, 0), (1, 1, 0), 1 - 0.25 * S2, 1, (0, 0, 0)),
    ((2, -1, 0), (-1, 1, 0), 1 - 0.25 * S2, 2, (1, 0, 0)),
    ((-1, 2, 0), (1, -1, 0), 1 - 0.25 * S2, 3, (0, 1, 0)),
    ((0.5, -2, 0), (0, 2, 0), 0.75, 4, (0.5, 0, 0)),
    ((-2, 0.5, 0), (2, 0, 0), 0.75, 5, (0, 0.5, 0)),
    ((2, 2, 0), (-2, -2, 0), 0.75 - 0.125 * S2, 6, (0.5, 0.5, 0)),
    ((-2, 0, 0), (2, 0, 0), 0.75, 1, (0, 0, 0)),  # the vertex and the edge from it along e2 at the same t: the lower region code
]


def test_hand_cases():
    """exactly representable numbers on the unit right triangle: one sweep per region, an initial overlap, a grazing miss, a
    sweep moving away, a zero and a degenerate triangle, r = 0, d = 0, the argmin, tmax inclusive, every invalid input"""
    unit = tri((0, 0, 0), (1, 0, 0), (0, 1, 0))

    def one(o, d, r, tmax=None, prims=unit):
        res = ref.sweep(np.array([o], F), np.array([d], F), F(r), prims, None if tmax is None else np.array([tmax], F))
        return tuple(a[0] for a in res)

    for o, d, t, region, point in HAND:
        gt, prim, reg, pt, cen, nrm = one(o, d, 0.5)
        assert prim == 0 and int(reg) == region and abs(float(gt) - t) <= 6e-8 * t, (o, float(gt), int(reg))
        assert np.allclose(pt, point, atol=1e-7) and np.allclose(cen, np.array(o) + float(gt) * np.array(d), atol=1e-6), o
        assert abs(float(np.linalg.norm(nrm.astype(D))) - 1) < 1e-6 and np.allclose(cen - pt, 0.5 * nrm, atol=1e-6), o
    gt, prim, reg, pt, cen, nrm = one((0.25, 0.25, 2), (0, 0, -2), 0.5)
    assert (float(gt), pt.tolist(), cen.tolist(), nrm.tolist()) == (0.75, [0.25, 0.25, 0], [0.25, 0.25, 0.5], [0, 0, 1])
    # an initial overlap: t = 0, the closest point, a normal of length distance / r
    gt, prim, reg, pt, cen, nrm = one((0.25, 0.25, 0.25), (0, 0, -2), 0.5)
    assert (float(gt), prim, int(reg), pt.tolist(), cen.tolist(), nrm.tolist()) == (0.0, 0, 0, [0.25, 0.25, 0], [0.25, 0.25, 0.25], [0, 0, 0.5])
    gt, prim, reg, pt, cen, nrm = one((-0.25, -0.25, 0), (5, 5, 5), 0.5)
    assert (float(gt), prim, int(reg), pt.tolist()) == (0.0, 0, 1, [0, 0, 0])
    # past the edge from vert along e1 at exactly r: touched; one binary32 step farther out: a miss
    gt, prim, reg, pt, cen, nrm = one((0.5, -0.5, -2), (0, 0, 4), 0.5)
    assert (float(gt), prim, int(reg), pt.tolist()) == (0.5, 0, 4, [0.5, 0, 0])
    gt, prim, reg, pt, cen, nrm = one((0.5, np.nextafter(F(-0.5), F(-1)), -2), (0, 0, 4), 0.5)
    assert (float(gt), prim, int(reg)) == (1.0, -1, 0) and cen.tolist() == pt.tolist() == [0.5, float(np.nextafter(F(-0.5), F(-1))), 2.0] and not nrm.any()
    # moving away
    gt, prim, reg, pt, cen, nrm = one((0.25, 0.25, 2), (0, 0, 2), 0.5)
    assert (float(gt), prim, cen.tolist()) == (1.0, -1, [0.25, 0.25, 4])
    # the zero triangle: its one point, as its first vertex; e2 = 2 e1: a segment, whose middle is the corner vert + e1
    gt, prim, reg, pt, cen, nrm = one((0, 0, 2), (0, 0, -2), 0.5, prims=tri((0, 0, 0), (0, 0, 0), (0, 0, 0)))
    assert (float(gt), prim, int(reg), pt.tolist()) == (0.75, 0, 1, [0, 0, 0])
    gt, prim, reg, pt, cen, nrm = one((1, 0, 3), (0, 0, -4), 1.0, prims=tri((0, 0, 0), (1, 0, 0), (2, 0, 0)))
    assert (float(gt), prim, int(reg), pt.tolist(), nrm.tolist()) == (0.5, 0, 2, [1, 0, 0], [0, 0, 1])
    gt, prim, reg, pt, cen, nrm = one((1.5, 0, 3), (0, 0, -4), 1.0, prims=tri((0, 0, 0), (1, 0, 0), (2, 0, 0)))
    assert (float(gt), prim, int(reg), pt.tolist()) == (0.5, 0, 5, [1.5, 0, 0])
    # r = 0: a swept point, from either side; d = 0: only the overlap rule
    for z in (2.0, -2.0):
        gt, prim, reg, pt, cen, nrm = one((0.25, 0.25, z), (0, 0, -2 * z), 0.0)
        assert (float(gt), prim, int(reg), pt.tolist(), cen.tolist()) == (0.5, 0, 0, [0.25, 0.25, 0], [0.25, 0.25, 0]) and not nrm.any()
    assert (float(one((0.25, 0.25, 0.25), (0, 0, 0), 0.5)[0]), int(one((0.25, 0.25, 0.25), (0, 0, 0), 0.5)[1])) == (0.0, 0)
    gt, prim, reg, pt, cen, nrm = one((0.25, 0.25, 0.25), (0, 0, 0), 0.125)
    assert (float(gt), prim, cen.tolist(), pt.tolist()) == (1.0, -1, [0.25, 0.25, 0.25], [0.25, 0.25, 0.25])
    # tmax is inclusive; one step below the contact: none, with the end of the shortened path
    below = float(np.nextafter(F(0.75), F(0)))
    assert [int(one((0.25, 0.25, 2), (0, 0, -2), 0.5, tm)[1]) for tm in (0.75, below, 0.0)] == [0, -1, -1]
    gt, prim, reg, pt, cen, nrm = one((0.25, 0.25, 2), (0, 0, -2), 0.5, below)
    assert float(gt) == below and cen.tolist() == pt.tolist() == [0.25, 0.25, float(F(2.0 - 2.0 * below))]
    # the argmin: the lowest index of equal t32; every invalid input
    three = np.concatenate([tri((0, 0, 5), (1, 0, 0), (0, 1, 0)), unit, unit])
    nan, inf = np.nan, np.inf
    o = np.array([[0.25, 0.25, 2]] * 11, F)
    d = np.array([[0, 0, -2]] * 11, F)
    r = np.full(11, 0.5, F)
    tm = np.ones(11, F)
    o[1, 0], o[2, 2], d[3, 1], d[4, 0] = nan, -inf, nan, inf
    r[5], r[6], r[7] = nan, -1.0, inf
    tm[8], tm[9], tm[10] = nan, -1.0, inf
    gt, prim, reg, pt, cen, nrm = ref.sweep(o, d, r, three, tm)
    assert prim.tolist() == [1] + [-1] * 10 and float(gt[0]) == 0.75 and np.isposinf(gt[1:]).all()
    assert np.array_equal(bits(cen[1:]), bits(o[1:])) and np.array_equal(bits(pt[1:]), bits(o[1:])) and not nrm[1:].any() and not reg.any()
    assert ref.sweep(o[:1], d[:1], r[:1], three[:0])[1].tolist() == [-1]  # no triangles: none


def _families(rng, n):
    """(name, scale, o, d, r, tmax, vert, e1, e2) of seeded pairs: soup, large triangles, an offset of 4096, slivers (as
    test_point_query's), paths aimed past an edge at a clearance of r give or take 1e-7 .. 1e-2, and swept points (r = 0)"""
    def soup(edge, spread, off=0.0):
        vert = (rng.uniform(-50, 50, (n, 3)) + off).astype(F)
        e1, e2 = (rng.uniform(-edge, edge, (n, 3)).astype(F) for _ in range(2))
        return vert, e1, e2, spread

    def sweeps(vert, e1, e2, spread, noise=0.15):
        o = (vert + rng.normal(size=(n, 3)) * spread).astype(F)
        u = rng.random((n, 1))
        v = rng.random((n, 1)) * (1 - u)
        target = vert.astype(D) + u * e1 + v * e2 + rng.normal(size=(n, 3)) * noise * spread
        d = ((target - o) * rng.uniform(0.5, 1.6, (n, 1))).astype(F)
        r = (rng.uniform(0.003, 0.3, n) * spread).astype(F)
        return o, d, r, rng.choice(np.array([0.5, 1.0, 1.0, 2.0], F), n).astype(F)

    for name, args in (("soup", (1.5, 3.0)), ("large", (200.0, 50.0)), ("offset", (1.5, 3.0, 4096.0))):
        vert, e1, e2, spread = soup(*args)
        yield (name, spread) + sweeps(vert, e1, e2, spread) + (vert, e1, e2)
    vert, e1, _, spread = soup(1.5, 1.0)
    perp = np.cross(e1.astype(D), rng.normal(size=(n, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    thin = 10.0 ** rng.uniform(-6, -2, (n, 1))
    e2 = (rng.uniform(-1.5, 1.5, (n, 1)) * e1 + thin * np.linalg.norm(e1, axis=1, keepdims=True) * perp).astype(F)
    yield ("slivers", spread) + sweeps(vert, e1, e2, spread) + (vert, e1, e2)
    # grazing: past the edge vert -> vert + e1, on the side away from the triangle, perpendicular to the edge
    vert, e1, e2, spread = soup(1.5, 3.0)
    A, B, Cc = ref.corners(vert, e1, e2)
    e = B - A
    eh = e / np.linalg.norm(e, axis=1, keepdims=True)
    inward = (Cc - A) - ((Cc - A) * eh).sum(1, keepdims=True) * eh
    w = -inward / np.linalg.norm(inward, axis=1, keepdims=True)
    nrm = np.cross(eh, w)
    tilt = rng.uniform(-0.6, 0.6, (n, 1))
    w = w * np.cos(tilt) + nrm * np.sin(tilt)  # still perpendicular to the edge, still facing away from the triangle
    g = np.cross(eh, w)
    r = rng.uniform(0.1, 1.0, n)
    delta = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -2, n)
    m = A + rng.uniform(0.2, 0.8, (n, 1)) * e
    o = (m + (r + delta)[:, None] * w - 3.0 * g).astype(F)
    d = (6.0 * g).astype(F)
    yield "grazing", spread, o, d, r.astype(F), np.ones(n, F), vert, e1, e2
    # swept points: r = 0, whose truth is where the segment crosses the triangle (the distance never goes below r)
    vert, e1, e2, spread = soup(1.5, 3.0)
    o, d, _, tmax = sweeps(vert, e1, e2, spread, noise=0.02)
    yield "points", spread, o, d, np.zeros(n, F), tmax, vert, e1, e2


def test_restatement_against_truth():
    """the restatement against the distance to the triangle sampled along the path (4,000 samples) and bisected: hit or miss
    agrees on every pair whose truth does not graze (least clearance within 1e-9 of the family's scale of r; at most 1 % of a
    family), and t agrees within 4x the worst error the committed seeds give.  The contact lies at r from the centre."""
    rng = np.random.default_rng(7)
    worst, excluded, gaps, regions = {}, {}, {}, set()
    for name, scale, o, d, r, tmax, vert, e1, e2 in _families(rng, 600):
        hit, t, region, contact = ref.pair_value(o, d, r, tmax, vert, e1, e2)
        tt, least = ref.truth_point(o, d, tmax, vert, e1, e2) if name == "points" else ref.truth(o, d, r, tmax, vert, e1, e2)
        graze = np.abs(least) < 1e-9 * scale
        excluded[name] = float(graze.mean())
        assert excluded[name] <= 0.01, (name, excluded)
        ok = ~graze
        assert np.array_equal(hit[ok], np.isfinite(tt)[ok]), (name, np.nonzero(ok & (hit != np.isfinite(tt)))[0][:5], least[ok & (hit != np.isfinite(tt))][:5])
        both = ok & hit
        assert both.sum() >= 100, name
        worst[name] = float(np.abs(t[both] - tt[both]).max())
        moving = both & (t > 0)
        cen = o.astype(D) + t[:, None] * d.astype(D)
        gap = np.abs(np.linalg.norm(cen - contact, axis=1) - r.astype(D))[moving]
        assert gap.max() <= 1e-9 * scale, (name, gap.max())
        gaps[name] = float(gap.max())
        regions |= set(np.unique(region[both]).tolist())
    print("worst |t - truth| per family:", worst, "worst | |center - point| - r |:", gaps, "grazing fraction excluded:", excluded)
    assert regions == set(range(7)), regions
    assert max(worst.values()) <= 4 * WORST_T_ERROR, worst


def _key32(o, inv, r, best, lo, hi, slack):
    """hip/sweep.hip's sweep_key in numpy binary32 (operation by operation): (near, far, visited)"""
    with np.errstate(all="ignore"):
        lo1, hi1 = (lo - r[:, None]).astype(F), (hi + r[:, None]).astype(F)
        e = (F(slack) * (np.abs(o) + np.maximum(np.abs(lo1), np.abs(hi1))).astype(F)).astype(F)
        t1 = (((lo1 - e).astype(F) - o).astype(F) * inv).astype(F)
        t2 = (((hi1 + e).astype(F) - o).astype(F) * inv).astype(F)
        nan = np.isnan(t1) | np.isnan(t2)
        near = np.where(nan, -np.inf, np.fmin(t1, t2)).astype(F).max(axis=1)
        far = np.where(nan, np.inf, np.fmax(t1, t2)).astype(F).min(axis=1)
    return near, far, (near <= far) & (far >= 0) & (near <= best)


def test_pruning_key_never_passes_the_value_of_a_triangle_in_the_box():
    """hip/sweep.hip skips a box when the segment misses the box inflated by r and widened by kSweepSlack * (|o_k| + max(|lo_k - r|,
    |hi_k + r|)) per plane, leaves it before 0 or enters it after `best`.  On a triangle's own three-corner box no pair with a
    value may be skipped with best = its t32, for scenes at the origin and moved by 4096 and 65536, near and far origins,
    axis-parallel directions and r from 0 to 2; every larger box is entered earlier and left later.  What the un-widened test
    would have needed, over what the widening gives, stays below one half (DESIGN.md "Swept-sphere queries": 2.6x by derivation)."""
    src = open(os.path.join(ROOT, "tyrant_amd", "csrc", "hip", "sweep.hip")).read()
    slack = float(re.search(r"kSweepSlack = ([0-9.]+)f \* kSweepUlp;", src).group(1)) * float(re.search(r"kSweepUlp = ([0-9.e-]+)f;", src).group(1))
    assert 2.0 ** -24 <= slack <= 2.0 ** -16
    rng = np.random.default_rng(8)
    n = 40000
    worst, hits = {}, 0
    for off in (0.0, 4096.0, 65536.0):
        for far_origin in (False, True):
            vert = (rng.uniform(-50, 50, (n, 3)) + off).astype(F)
            e1, e2 = (rng.uniform(-1.5, 1.5, (n, 3)).astype(F) for _ in range(2))
            o = (vert + rng.normal(size=(n, 3)) * (60.0 if far_origin else 3.0)).astype(F)
            u = rng.random((n, 1))
            target = vert.astype(D) + u * e1 + rng.random((n, 1)) * (1 - u) * e2 + rng.normal(size=(n, 3)) * 0.5
            d = ((target - o) * rng.uniform(0.5, 1.6, (n, 1))).astype(F)
            axis = rng.integers(0, 8, n)  # three eighths of the directions parallel to an axis, another eighth to a plane
            for k in range(3):
                d[(axis != k) & (axis < 3), k] = 0
            d[axis == 3, 0] = 0
            r = (rng.uniform(0, 2, n) * (rng.random(n) > 0.1)).astype(F)
            tmax = np.ones(n, F)
            hit, t, _, _ = ref.pair_value(o, d, r, tmax, vert, e1, e2)
            t32 = t[hit].astype(F)
            b, c = (vert + e1).astype(F), (vert + e2).astype(F)
            lo, hi = np.minimum(np.minimum(vert, b), c)[hit], np.maximum(np.maximum(vert, b), c)[hit]
            with np.errstate(all="ignore"):
                inv = (F(1) / d[hit]).astype(F)
            near0, far0, _ = _key32(o[hit], inv, r[hit], t32, lo, hi, 0.0)
            near, far, visited = _key32(o[hit], inv, r[hit], t32, lo, hi, slack)
            assert visited.all(), (off, far_origin, int((~visited).sum()))
            with np.errstate(all="ignore"):
                need = np.maximum.reduce([(near0 - t32) / (near0 - near), -far0 / (far - far0), (near0 - far0) / ((near0 - near) + (far - far0))])
            need = np.where(np.isfinite(need), np.maximum(need, 0.0), 0.0)
            worst[(off, far_origin)] = float(need.max())
            hits += int(hit.sum())
    print("needed widening / widening:", worst, "pairs with a value:", hits)
    assert hits >= 60000 and max(worst.values()) <= 0.5, worst


def test_fixtures_reach_what_they_are_for():
    """every region wins somewhere; bit-equal t32 ties exist (the duplicated scene: all of them); initial overlaps, misses and
    hits beyond tmax exist; the lattice's tree needs more stack than the 12 LDS entries; stack40 has an over-long leaf"""
    from tyrant_amd import binding

    nodes, prims, (o, d, r, tmax), (t, prim, region, _, _, _) = lattice_case()
    assert set(np.unique(region[prim >= 0]).tolist()) == set(range(7))
    assert ((prim >= 0) & (t == 0)).sum() >= 20 and (prim < 0).sum() >= 20
    sub = np.nonzero(prim < 0)[0][:256]
    longer = ref.sweep(o[sub], d[sub], r[sub], prims, (tmax[sub] * F(4) + F(1)).astype(F))
    assert (longer[1] >= 0).sum() >= 10  # a contact behind the end of the path
    _, _, ties = ref.brute_values(o[:256], d[:256], r[:256], tmax[:256], prims)
    assert (ties >= 2).sum() >= 64  # a sphere dropped onto a grid vertex touches all the triangles around it at once
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    nodes, prims, (o, d, r), (t, prim, _, _, _, _) = duplicated_case()
    _, arg, ties = ref.brute_values(o, d, r, np.ones(len(o), F), prims)
    assert (arg >= 0).sum() >= 200 and (ties[arg >= 0] >= 2).all()
    nodes, prims = build(stack40())
    assert nodes["primitiveCount"].max() == 40  # an over-long leaf: synthetic records


def test_sweep_kernel_keeps_registers_and_lds_in_budget():
    """exactly one k_query_sweep; no vector spills; scratch no larger than the LdsStack's private spill arrays (52 entries of 8
    bytes, plus the frame's alignment); LDS (24,576 + 7,168 bytes) that admits the three blocks per CU the launch bounds plan
    for.  The occupancy reached is printed (DESIGN.md "Swept-sphere queries" records it), not prescribed."""
    assert_kernel_budget("sweep", "k_query_sweep", 1, (64 - 12) * 8 + 16, 24576 + 7168, planned=launch_bounds_blocks("sweep", "k_query_sweep"))


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_sweep", "tyr_sweep_out", hip.SweepOut, 6)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, o, d, r, tmax=None, **kw):
    r = r if np.isscalar(r) else np.array(r)
    return tuple(x.cpu().numpy() for x in g.query_sweep(np.array(o), np.array(d), r, None if tmax is None else np.array(tmax), normal=True, **kw))


same = functools.partial(same_outputs, NAMES)


def check(g, prims, o, d, r, tmax=None, what=""):
    got = ask(g, o, d, r, tmax)
    want = ref.sweep(o, d, r, prims, tmax)
    same(got, want, what)
    return got, want


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lattice_and_ties(hip):
    """heightfield(32): a sphere dropped onto every grid vertex (it touches all the triangles around it at once) and seeded
    sweeps; radii 0, small and larger than a cell; tmax 0, shorter than the contact, 1 and longer"""
    nodes, prims, (o, d, r, tmax), want = lattice_case()
    g = renderer(hip, nodes, prims)
    got = ask(g, o, d, r, tmax)
    same(got, want, "lattice")
    assert len(np.unique(got[2])) == 7 and (got[1] < 0).any() and (got[0] == 0).any()
    same(ask(g, o[:1089], d[:1089], r[:1089]), tuple(a[:1089] for a in want), "tmax NULL")  # (the drops' tmax is 1)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_exact_ties_resolve_to_the_lower_index(hip):
    """a scene concatenated with itself: every winner is the lower of the two copies' build-order indices; and 40 identical
    triangles (an over-long leaf behind synthetic records), alone and next to the Cornell box"""
    from tyrant_amd import scenes

    nodes, prims, (o, d, r), want = duplicated_case()
    twin = duplicated(22, 2048)[3]
    g = renderer(hip, nodes, prims)
    got = ask(g, o, d, r)
    same(got, want, "duplicated")
    prim = got[1][got[1] >= 0]
    assert prim.size >= 200 and (prim < twin[prim]).all()
    for tris in (stack40(), np.concatenate([scenes.cornell_box().triangles, stack40()])):
        nodes, prims = build(tris)
        g.upload(nodes, prims)
        so, sd, sr = aimed(np.random.default_rng(43), prims, 1500)
        (_, prim, _, _, _, _), _ = check(g, prims, so, sd, sr, what="stack40")
        stack = np.nonzero((np.ascontiguousarray(prims).view(np.uint8).reshape(len(prims), -1) == np.ascontiguousarray(stack40()[:1]).view(np.uint8)).all(axis=1))[0]
        on_stack = np.isin(prim, stack)
        assert stack.size == 40 and on_stack.any() and (prim[on_stack] == stack.min()).all()  # the first of the identical records
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slivers", [False, True])
def test_scale_and_slack(hip, slivers):
    """a soup moved by (4096, -4096, 8192), without and with slivers: sweeps from within 1e-3 of the surface, from the root box
    and from half way to the origin; a quarter of them parallel to an axis"""
    nodes, prims = offset_soup(slivers)
    rng = np.random.default_rng(44)
    o = np.concatenate([surface_points(rng, prims, 384, 1e-3), box_points(rng, prims, 512), (box_points(rng, prims, 128) - OFFSET * F(0.5)).astype(F)])
    n = len(o)
    d = ((surface_points(rng, prims, n, 0.5) - o) * rng.uniform(0.3, 1.7, (n, 1))).astype(F)
    axis = rng.integers(0, 12, n)
    for k in range(3):
        d[(axis != k) & (axis < 3), k] = 0
    r = rng.choice(np.array([0.0, 0.01, 0.5, 3.0], F), n).astype(F)
    g = renderer(hip, nodes, prims)
    (t, prim, _, _, _, _), _ = check(g, prims, o, d, r, what=f"offset soup, slivers={slivers}")
    assert (prim >= 0).sum() >= n // 4 and (prim < 0).sum() >= n // 20
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_directions_whose_reciprocal_is_no_normal_number(hip):
    """the Cornell box: displacements with subnormal components (1 / d_k is infinite, yet with a tmax near 2^128 the centre
    moves by a third of a unit) and with components near 2^128 (1 / d_k is subnormal) and a tmax near 2^-122, each sphere a
    little short of touching at the start; such an axis must not prune"""
    import nearest_ref

    sc, nodes, prims = built_scene("cornell36")
    g = renderer(hip, nodes, prims)
    rng = np.random.default_rng(49)
    n = 1536
    lo, hi = nodes[0]["bounds"][0].astype(F), nodes[0]["bounds"][1].astype(F)
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(F)
    dist = np.sqrt(nearest_ref.nearest(o, prims)[0].astype(D))
    small = np.arange(n) < n // 2
    reach = np.where(small, 0.3, 40.0)  # how far the centre moves at most
    r = np.maximum(dist - rng.uniform(0, 1, n) * reach, 0).astype(F)
    unit = rng.normal(size=(n, 3))
    unit[rng.random((n, 3)) < 0.3] = 0  # some components exactly zero: parallel to those planes
    unit /= np.maximum(np.abs(unit).max(axis=1, keepdims=True), 1e-30)
    d = (unit * np.where(small, 1e-39, 3e38)[:, None]).astype(F)
    tmax = (reach / np.where(small, 1e-39, 3e38) * rng.uniform(0.5, 1, n)).astype(F)
    assert ((np.abs(d[small]) < 2.0 ** -126) & (d[small] != 0)).any() and np.isfinite(d).all() and np.isfinite(tmax).all()
    (t, prim, _, _, _, _), _ = check(g, prims, o, d, r, tmax, what="subnormal and huge displacements")
    for part in (small, ~small):
        assert ((prim >= 0) & (t > 0))[part].sum() >= 50 and (prim < 0)[part].sum() >= 50, (int(((prim >= 0) & (t > 0))[part].sum()), int((prim < 0)[part].sum()))
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_radii_tmax_hostile_input_and_batch_sizes(hip):
    """the Cornell box: sweeps starting in overlap with several triangles (the corners), radii 0 to larger than the room, tmax 0,
    shorter than the contact, per sweep and NULL, zero and axis-parallel directions through the walls' box faces, NaN / infinite /
    negative input; n = 0 .. 4097; a scene without triangles; every combination of the optional outputs"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    g = renderer(hip, nodes, prims)
    rng = np.random.default_rng(45)
    n = 6000
    lo, hi = nodes[0]["bounds"][0].astype(F), nodes[0]["bounds"][1].astype(F)
    o = (lo - 5 + (hi - lo + 10) * rng.random((n, 3))).astype(F)
    d = (rng.normal(size=(n, 3)) * rng.choice([1.0, 20.0, 150.0], (n, 1))).astype(F)
    r = rng.choice(np.array([0.0, 0.0, 0.5, 3.0, 10.0, 200.0], F), n).astype(F)
    tmax = rng.choice(np.array([0.0, 0.25, 1.0, 1.0, 3.0], F), n).astype(F)
    kind = rng.integers(0, 30, n)
    o[kind < 6] = np.round(o[kind < 6])  # whole numbers, some of them on the walls' planes
    for k in range(3):
        d[(kind < 6) & (kind % 3 != k), k] = 0  # parallel to an axis
    d[kind == 6] = 0
    corner = np.nonzero(kind == 7)[0]  # in a corner of the room: overlapping both triangles of up to three walls
    o[corner] = np.where(rng.random((corner.size, 3)) < 0.5, lo, hi) + rng.uniform(-0.4, 0.4, (corner.size, 3)).astype(F)
    r[corner] = 1.0
    bad = np.array([np.nan, np.inf, -np.inf], F)
    for code, arr in ((8, o), (9, d)):
        w = np.nonzero(kind == code)[0]
        arr[w, rng.integers(0, 3, w.size)] = bad[rng.integers(0, 3, w.size)]
    r[kind == 10] = rng.choice(np.array([np.nan, np.inf, -1.0, -0.0], F), (kind == 10).sum())
    tmax[kind == 11] = rng.choice(np.array([np.nan, np.inf, -1.0, -0.0], F), (kind == 11).sum())
    want = ref.sweep(o, d, r, prims, tmax)
    invalid = np.isposinf(want[0])
    assert invalid.sum() >= n // 12 and (want[1][corner] >= 0).all() and (want[0][corner] == 0).all()
    got = ask(g, o, d, r, tmax)
    same(got, want, "cornell")
    unit_tmax = ref.sweep(o[:1500], d[:1500], r[:1500], prims)
    same(ask(g, o[:1500], d[:1500], r[:1500]), unit_tmax, "tmax NULL")
    same(ask(g, o[:1500], d[:1500], 3.0), ref.sweep(o[:1500], d[:1500], F(3.0), prims), "a scalar radius")
    for m in (0, 1, 63, 64, 65, 4097):  # every prefix answers as the whole batch did
        same(ask(g, o[:m], d[:m], r[:m], tmax[:m]), tuple(a[:m] for a in want), f"n = {m}")
    # optional outputs NULL, in every combination, through the C call; the arrays not passed stay untouched
    m = 1000
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a[:m])).cuda()  # noqa: E731
    to, td, tr, tt = on(o), on(d), on(r), on(tmax)
    P = C.c_void_p
    for use in itertools.product((False, True), repeat=4):
        outs = [torch.full((m,), 7, dtype=torch.float32).cuda(), torch.full((m,), 7, dtype=torch.int32).cuda(), torch.full((m,), 7, dtype=torch.uint8).cuda()]
        outs += [torch.full((m, 3), 7, dtype=torch.float32).cuda() for _ in range(3)]
        torch.cuda.synchronize()
        ptrs = [outs[0].data_ptr(), outs[1].data_ptr()] + [outs[2 + k].data_ptr() if use[k] else None for k in range(4)]
        out = hip.SweepOut(*ptrs)
        assert hip.lib().tyr_query_sweep(g.h, m, P(to.data_ptr()), P(td.data_ptr()), P(tr.data_ptr()), P(tt.data_ptr()), 0, C.byref(out), None) == 0
        assert g.query_error() == 0
        res = [x.cpu().numpy() for x in outs]
        used = (True, True) + use
        same_outputs([nm for nm, u in zip(NAMES, used) if u], [x for x, u in zip(res, used) if u], [w[:m] for w, u in zip(want, used) if u], f"outputs {use}")
        assert all((x == 7).all() for x, u in zip(res, used) if not u), use
    # a scene without triangles: every valid sweep a miss
    g.upload(*no_triangles())
    same(ask(g, o, d, r, tmax), ref.sweep(o, d, r, prims[:0], tmax), "empty scene")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_sweep_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with sweeps between its tyr_render calls: the same accumulation buffer and counters
    as without them"""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    rng = np.random.default_rng(46)
    n = 20000
    o = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(5, 80, n)], axis=1).astype(F)
    d = (rng.normal(size=(n, 3)) * 40).astype(F)
    r = rng.uniform(0, 3, n).astype(F)
    want = ref.sweep(o, d, r, prims)

    def between(g):
        same(ask(g, o, d, r), want, "between two renders")
        ask(g, o, d, 0.0, np.full(n, 0.5, F))

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the answers to the refitted scene's; a torch side stream and the ctx's stream work; bad
    arguments are refused before any launch; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(16))
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    rng = np.random.default_rng(47)
    n = 1000
    o, d, r = aimed(rng, prims, n)
    check(g, prims, o, d, r, what="before the refit")
    moved = deformed(prims, 4.0)
    g.refit(moved)
    got, want = check(g, moved, o, d, r, what="after the refit")
    assert not np.array_equal(want[1], ref.sweep(o, d, r, prims)[1])
    # a side stream, device tensors taken in place; then the ctx's own stream (NULL) through the C call
    to, td, tr = (torch.from_numpy(a).cuda() for a in (o, d, r))
    tt = torch.full((n,), 0.5).cuda()
    res, side = on_side_stream(lambda side: (g.query_sweep(to, td, tr, tt, normal=True, stream=side), side))
    half = ref.sweep(o, d, r, moved, np.full(n, 0.5, F))
    same(tuple(x.cpu().numpy() for x in res), half, "side stream")
    # a number as the radius, device tensors, and a side stream named from outside its context: the radius tensor is filled on
    # the current stream, behind work that keeps it busy, and the sweep on `side` has to wait for that fill
    busy = torch.randn(2048, 2048, device="cuda")
    for _ in range(8):
        busy = busy @ busy * 1e-3
    res = g.query_sweep(to, td, 0.5, tt, normal=True, stream=side)
    side.synchronize()
    same(tuple(x.cpu().numpy() for x in res), ref.sweep(o, d, F(0.5), moved, np.full(n, 0.5, F)), "a scalar radius on a side stream")
    del busy

    L, h, P = hip.lib(), g.h, C.c_void_p
    t, prim = torch.full((n,), 7.0).cuda(), torch.full((n,), 7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    ok = hip.SweepOut(t.data_ptr(), prim.data_ptr(), None, None, None, None)
    po, pd, pr, pt = P(to.data_ptr()), P(td.data_ptr()), P(tr.data_ptr()), P(tt.data_ptr())
    assert L.tyr_query_sweep(h, n, po, pd, pr, pt, 0, C.byref(ok), None) == 0
    assert g.query_error() == 0  # (waits for the ctx's stream)
    same((t.cpu().numpy(), prim.cpu().numpy()), half[:2], "the ctx's stream")
    before = prim.cpu().numpy().copy()
    inv = hip.TYR_ERR_INVALID
    assert L.tyr_query_sweep(None, 4, po, pd, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep(h, 4, None, pd, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep(h, 4, po, None, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep(h, 4, po, pd, None, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep(h, 4, po, pd, pr, None, 0, None, None) == inv
    assert L.tyr_query_sweep(h, 4, po, pd, pr, None, 0, C.byref(hip.SweepOut(None, prim.data_ptr(), None, None, None, None)), None) == inv
    assert L.tyr_query_sweep(h, 4, po, pd, pr, None, 0, C.byref(hip.SweepOut(t.data_ptr(), None, None, None, None, None)), None) == inv
    assert L.tyr_query_sweep(h, 4, po, pd, pr, None, 1, C.byref(ok), None) == inv  # flags must be 0
    assert L.tyr_query_sweep(h, 1 << 31, po, pd, pr, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_sweep(h, 0, None, None, None, None, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_sweep(empty.h, 4, po, pd, pr, None, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_sweep(to.double(), td, tr)
    with pytest.raises(ValueError):
        g.query_sweep(to, td[:, :2].contiguous(), tr)
    with pytest.raises(ValueError):
        g.query_sweep(to, td, tr[:5])
    with pytest.raises(ValueError):
        g.query_sweep(to, td, tr, tt[:5])
    assert np.array_equal(prim.cpu().numpy(), before)  # the refused calls wrote nothing
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_c3_tree(hip):
    """one pass on C3's 1 M-triangle tree: the 256 sweeps of tests/golden/sweep_c3.npz (origins within 1.5 of the surface, radii 0
    to 1) against the winners tools/sweep_c3_golden.py recorded by brute force -- a one-off ten minutes of numpy.  Every run
    checks that the file belongs to these triangles, recomputes one sweep by brute force and evaluates the winners' other
    outputs from the restatement."""
    sc, nodes, prims = built_scene("mesh706")
    z = np.load(C3_ANSWERS)
    assert str(z["digest"]) == hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest(), "the recorded answers belong to other triangles"
    o, d, r, tmax, t, arg = (z[k] for k in ("origins", "directions", "radius", "tmax", "t", "prim"))
    assert len(o) == 256 and (arg >= 0).sum() >= 64 and (arg < 0).sum() >= 16
    live = int(np.random.default_rng(48).integers(0, 256))
    lb, la, _ = ref.brute_values(o[live:live + 1], d[live:live + 1], r[live:live + 1], tmax[live:live + 1], prims, chunk_pairs=1 << 16)
    assert int(la[0]) == int(arg[live]) and (la[0] < 0 or bits(lb)[0] == bits(t)[live])
    hit = arg >= 0
    want = list(ref.sweep(o, d, r, prims[:0], tmax))  # every sweep as a miss; then the winners' pairs
    vert, e1, e2 = ref.records(prims)
    w = arg[hit]
    ok, tv, reg, c = ref.pair_value(o[hit], d[hit], r[hit], tmax[hit], vert[w], e1[w], e2[w])
    assert ok.all() and np.array_equal(bits(tv.astype(F)), bits(t[hit]))
    cen = o[hit].astype(D) + tv[:, None] * d[hit].astype(D)
    rad = r[hit].astype(D)[:, None]
    with np.errstate(all="ignore"):
        nrm = np.where(rad == 0, 0.0, (cen - c) / rad)
    want[0][hit], want[1][hit], want[2][hit] = t[hit], w.astype(np.int32), reg
    want[3][hit], want[4][hit], want[5][hit] = c.astype(F), cen.astype(F), nrm.astype(F)
    g = renderer(hip, nodes, prims)
    same(ask(g, o, d, r, tmax), want, "C3")
    assert g.query_error() == 0
    g.close()
