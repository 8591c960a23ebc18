"""Batched closest-segment queries on the uploaded scene (tyr_query_segment, hip/segment.hip; Renderer.query_segment): the least
distance between a segment and the mesh of include/tyr_c.h "Closest-segment queries" as an argmin over all triangles, bit for bit
against its numpy restatement (tests/segment_ref.py) by brute force -- the definition has no traversal order in it, so nothing
else is needed as an oracle.

CPU: the restatement by hand, the restatement against a binary64 truth (ternary search and a crossing test), the pruning key
against the value, what the fixtures are for, what the compiler made of the kernel, the ABI.  GPU: lattices with shared edges and
vertices, exact ties by index, over-long leaves, offset scenes and slivers, bounds, hostile input, batch sizes, optional outputs,
isolation from the render, refit, streams, argument checks, and one pass on C3's 1 M-triangle tree."""
import ctypes as C
import functools
import hashlib
import itertools
import os
import re

import numpy as np
import pytest

import segment_ref as ref
from conftest import GOLDEN, ROOT, bits, built_scene
from query_support import (OFFSET, assert_kernel_budget, assert_query_abi, assert_render_undisturbed, box_points, build, deformed, duplicated, lattice, launch_bounds_blocks,
                           no_triangles, offset_soup, on_side_stream, query_exists, renderer, stack40, surface_points, tri)
from query_support import same as same_outputs

F = np.float32
D = np.float64
C3_ANSWERS = os.path.join(GOLDEN, "segment_c3.npz")
NAMES = ref.NAMES
# |sqrt(F) - truth| of the restatement on the committed seeds, per family (test_restatement_against_truth prints it; DESIGN.md
# "Closest-segment queries" has the table): each is asserted with 4x room for other seeds
WORST_ERROR = {"soup": 1.3e-14, "large": 3.5e-14, "offset": 1.1e-12, "slivers": 1.0e-14, "parallel": 8.6e-15, "grazing": 1.2e-14, "points": 4.5e-15}

_the_query_exists = query_exists("tyr_query_segment")


# ---- fixtures (numpy only) --------------------------------------------------------------------------------------------
def aimed(rng, prims, n, reach=(0.3, 1.7)):
    """seeded segments from the inflated root box towards points near the surface, some stopping short, some passing through"""
    p = box_points(rng, prims, n)
    target = surface_points(rng, prims, n, 0.5)
    q = (p + (target - p) * rng.uniform(*reach, (n, 1))).astype(F)
    return p, q


@functools.lru_cache(maxsize=None)
def lattice_case():
    """heightfield(32): over every grid vertex a short vertical segment (every other one through the vertex, the rest ending above
    it) and a long diagonal one; the 4096 box points as p with seeded q; a quarter of all with a bound -- (nodes, prims, segments,
    answers)"""
    nodes, prims, grid, pts = lattice(32, 21)
    rng = np.random.default_rng(51)
    down = np.where((np.arange(len(grid)) % 2 == 0)[:, None], np.array([0, 0, -35], F), np.array([0, 0, -4], F))
    diag = np.array([70, -55, -35], F) * rng.choice(np.array([-1.0, 1.0], F), (len(grid), 1))
    p = np.concatenate([grid, grid, pts])
    q = np.concatenate([grid + down, grid + diag, (pts + rng.normal(size=pts.shape) * rng.choice([0.5, 4.0, 30.0], (len(pts), 1))).astype(F)]).astype(F)
    md = rng.choice(np.array([np.inf, np.inf, np.inf, 2.0], F), len(p)).astype(F)
    seg = tuple(np.ascontiguousarray(a) for a in (p, q, md))
    return nodes, prims, seg, ref.segment(p, q, prims, md)


@functools.lru_cache(maxsize=None)
def duplicated_case():
    nodes, prims, pts, _ = duplicated(22, 2048)
    rng = np.random.default_rng(52)
    n = 640
    p = pts[:n].copy()
    q = (p + (surface_points(rng, prims, n, 0.5) - p) * rng.uniform(0.5, 1.5, (n, 1))).astype(F)
    return nodes, prims, (p, q), ref.segment(p, q, prims)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
HAND = [  # vert (0,0,0), e1 (1,0,0), e2 (0,1,0): p, q, dist2, s, feature, region, on_segment, on_triangle
    ((0.25, 0.25, 1), (0.25, 0.25, -1), 0.0, 0.5, 0, 0, (0.25, 0.25, 0), (0.25, 0.25, 0)),  # through the interior
    ((0.5, 0, 1), (0.5, 0, -1), 0.0, 0.5, 0, 0, (0.5, 0, 0), (0.5, 0, 0)),  # through an edge
    ((0, 0, 1), (0, 0, -1), 0.0, 0.5, 0, 0, (0, 0, 0), (0, 0, 0)),  # through a corner
    ((0.25, 0.25, 1), (0.25, 0.25, 2), 1.0, 0.0, 1, 0, (0.25, 0.25, 1), (0.25, 0.25, 0)),
    ((0.25, 0.25, 2), (0.25, 0.25, 1), 1.0, 1.0, 2, 0, (0.25, 0.25, 1), (0.25, 0.25, 0)),
    ((0.5, -1, 1), (0.5, -1, -1), 1.0, 0.5, 3, 4, (0.5, -1, 0), (0.5, 0, 0)),
    ((-1, 0.5, 1), (-1, 0.5, -1), 1.0, 0.5, 4, 5, (-1, 0.5, 0), (0, 0.5, 0)),
    ((1, 1, 1), (1, 1, -1), 0.5, 0.5, 5, 6, (1, 1, 0), (0.5, 0.5, 0)),
    ((-1, -1, 1), (-1, -1, -1), 2.0, 0.5, 3, 1, (-1, -1, 0), (0, 0, 0)),  # both edges from vert at the same F: the lower feature code
    ((2, -1, 1), (2, -1, -1), 2.0, 0.5, 3, 2, (2, -1, 0), (1, 0, 0)),
    ((-1, 2, 1), (-1, 2, -1), 2.0, 0.5, 4, 3, (-1, 2, 0), (0, 1, 0)),
    ((-1, 0.25, 0), (2, 0.25, 0), 0.0, 1.0 / 3.0, 4, 5, (0, 0.25, 0), (0, 0.25, 0)),  # in the plane, across the triangle: an edge
    ((0.25, 0.25, 0), (3, 3, 0), 0.0, 0.0, 1, 0, (0.25, 0.25, 0), (0.25, 0.25, 0)),  # in the plane, from inside: an endpoint
    ((0, -1, 0), (1, -1, 0), 1.0, 0.0, 1, 1, (0, -1, 0), (0, 0, 0)),  # parallel to the edge along e1 (den == 0): every feature ties
    ((0.25, 0.25, 1), (0.25, 0.25, 1), 1.0, 0.0, 1, 0, (0.25, 0.25, 1), (0.25, 0.25, 0)),  # p == q over the face
    ((-1, -1, 0), (-1, -1, 0), 2.0, 0.0, 1, 1, (-1, -1, 0), (0, 0, 0)),  # p == q outside
]


def test_hand_cases():
    """exactly representable numbers on the unit right triangle: every feature and region, crossings through the interior, an edge
    and a corner, segments in the plane, parallel to an edge, of zero length; a zero-area and a point triangle; the argmin; the
    strict bound; every invalid input"""
    unit = tri((0, 0, 0), (1, 0, 0), (0, 1, 0))

    def one(p, q, md=None, prims=unit):
        res = ref.segment(np.array([p], F), np.array([q], F), prims, None if md is None else np.array([md], F))
        return tuple(a[0] for a in res)

    features, regions = set(), set()
    for p, q, dist2, s, feature, region, x, y in HAND:
        got = one(p, q)
        assert (float(got[0]), int(got[1]), float(got[2]), int(got[3]), int(got[4])) == (dist2, 0, float(F(s)), feature, region), (p, q, got)
        assert got[5].tolist() == list(map(float, x)) and got[6].tolist() == list(map(float, y)), (p, q, got)
        features.add(feature), regions.add(region)
    assert features == set(range(6)) and regions == set(range(7))
    # e2 = 2 e1: a segment from vert to vert + e2, whose nearest point is on the edge along e2; the zero triangle: its one point
    got = one((1.5, 1, 1), (1.5, 1, -1), prims=tri((0, 0, 0), (1, 0, 0), (2, 0, 0)))
    assert (float(got[0]), int(got[1]), int(got[3]), int(got[4]), got[6].tolist()) == (1.0, 0, 4, 5, [1.5, 0, 0])
    got = one((0, 0, 2), (0, 0, 1), prims=tri((0, 0, 0), (0, 0, 0), (0, 0, 0)))
    assert (float(got[0]), int(got[1]), float(got[2]), int(got[3]), int(got[4]), got[6].tolist()) == (1.0, 0, 1.0, 2, 1, [0, 0, 0])
    # the bound is strict: at exactly max_dist "none" (dist2 = bound2, both points p), one binary32 step more: found
    got = one((0.25, 0.25, 2), (0.25, 0.25, 1), 1.0)
    assert (float(got[0]), int(got[1]), float(got[2]), int(got[3]), int(got[4])) == (1.0, -1, 0.0, 0, 0) and got[5].tolist() == got[6].tolist() == [0.25, 0.25, 2]
    assert int(one((0.25, 0.25, 2), (0.25, 0.25, 1), np.nextafter(F(1), F(2)))[1]) == 0
    assert (float(one((0.25, 0.25, 2), (0.25, 0.25, 1), 0.5)[0]), int(one((0.25, 0.25, 1), (0.25, 0.25, -1), 0.0)[1])) == (0.25, -1)  # F = 0 is not < 0
    # the argmin: the lowest index of equal F32; every invalid input; max_dist = +inf and -0 are valid
    three = np.concatenate([tri((0, 0, 5), (1, 0, 0), (0, 1, 0)), unit, unit])
    nan, inf = np.nan, np.inf
    p = np.array([[0.25, 0.25, 2]] * 9, F)
    q = np.array([[0.25, 0.25, 1]] * 9, F)
    md = np.full(9, 8.0, F)
    p[1, 0], p[2, 2], q[3, 1], q[4, 0], md[5], md[6], md[7], md[8] = nan, -inf, nan, inf, nan, -1.0, inf, -0.0
    got = ref.segment(p, q, three, md)
    assert got[1].tolist() == [1] + [-1] * 6 + [1, -1] and float(got[0][0]) == 1.0 and np.isposinf(got[0][1:7]).all() and float(got[0][8]) == 0.0
    assert np.array_equal(bits(got[5][1:7]), bits(p[1:7])) and np.array_equal(bits(got[6][1:7]), bits(p[1:7])) and not got[2][1:7].any() and not got[3][1:7].any()
    assert ref.segment(p[:1], q[:1], three[:0])[1].tolist() == [-1] and np.isposinf(ref.segment(p[:1], q[:1], three[:0])[0]).all()  # no triangles: none


def _families(rng, n):
    """(name, scale, p, q, vert, e1, e2) of seeded pairs: soup, large triangles, an offset of 4096, slivers (as test_sweep_query's),
    segments nearly parallel to the edge along e1, segments that pass that edge on the outside at 1e-7 .. 1e-2, segments of zero
    length"""
    def soup(edge, spread, off=0.0):
        vert = (rng.uniform(-50, 50, (n, 3)) + off).astype(F)
        e1, e2 = (rng.uniform(-edge, edge, (n, 3)).astype(F) for _ in range(2))
        return vert, e1, e2, spread

    def segments(vert, e1, e2, spread, noise=0.3):
        p = (vert + rng.normal(size=(n, 3)) * spread).astype(F)
        u = rng.random((n, 1))
        v = rng.random((n, 1)) * (1 - u)
        target = vert.astype(D) + u * e1 + v * e2 + rng.normal(size=(n, 3)) * rng.choice([0.02, noise], (n, 1)) * spread  # half aimed at the triangle
        q = (p + (target - p) * rng.uniform(0.3, 1.8, (n, 1))).astype(F)
        return p, q

    for name, args in (("soup", (1.5, 3.0)), ("large", (200.0, 50.0)), ("offset", (1.5, 3.0, 4096.0))):
        vert, e1, e2, spread = soup(*args)
        yield (name, spread) + segments(vert, e1, e2, spread) + (vert, e1, e2)
    vert, e1, _, spread = soup(1.5, 1.0)
    perp = np.cross(e1.astype(D), rng.normal(size=(n, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    thin = 10.0 ** rng.uniform(-6, -2, (n, 1))
    e2 = (rng.uniform(-1.5, 1.5, (n, 1)) * e1 + thin * np.linalg.norm(e1, axis=1, keepdims=True) * perp).astype(F)
    yield ("slivers", spread) + segments(vert, e1, e2, spread) + (vert, e1, e2)
    # the frame of the edge vert -> vert + e1: along it, away from the triangle in its plane (tilted out of it), and across
    def frame(vert, e1, e2):
        A, B, Cc = ref.corners(vert, e1, e2)
        e = B - A
        eh = e / np.linalg.norm(e, axis=1, keepdims=True)
        inward = (Cc - A) - ((Cc - A) * eh).sum(1, keepdims=True) * eh
        w = -inward / np.linalg.norm(inward, axis=1, keepdims=True)
        nrm = np.cross(eh, w)
        tilt = rng.uniform(-0.6, 0.6, (n, 1))
        w = w * np.cos(tilt) + nrm * np.sin(tilt)
        return A, e, eh, w, np.cross(eh, w)

    vert, e1, e2, spread = soup(1.5, 3.0)
    A, e, eh, w, g = frame(vert, e1, e2)
    off = rng.uniform(0.05, 1.0, (n, 1)) * w
    slope = rng.choice([-1.0, 1.0], (n, 1)) * 10.0 ** rng.uniform(-7, -3, (n, 1))
    length = rng.uniform(0.3, 1.5, (n, 1)) * np.linalg.norm(e, axis=1, keepdims=True)
    start = A + rng.uniform(-0.3, 0.6, (n, 1)) * e + off
    yield "parallel", spread, start.astype(F), (start + length * (eh + slope * w)).astype(F), vert, e1, e2
    vert, e1, e2, spread = soup(1.5, 3.0)
    A, e, eh, w, g = frame(vert, e1, e2)
    delta = 10.0 ** rng.uniform(-7, -2, (n, 1))
    m = A + rng.uniform(0.2, 0.8, (n, 1)) * e
    yield "grazing", spread, (m + delta * w - 3.0 * g).astype(F), (m + delta * w + 3.0 * g).astype(F), vert, e1, e2
    vert, e1, e2, spread = soup(1.5, 3.0)
    p, _ = segments(vert, e1, e2, spread)
    yield "points", spread, p, p.copy(), vert, e1, e2


def test_restatement_against_truth():
    """the restatement against the least point-to-triangle distance along the segment (a ternary search: the distance is convex) and
    a Moeller-Trumbore crossing test: a pair whose segment crosses the triangle more than 1e-9 inside its rim and its own ends has
    F = 0 from feature 0, a pair farther than 1e-9 of the family's scale from the triangle has F > 0 and sqrt(F) within 4x the
    worst error the committed seeds give; the rest (at most 1 % of a family) grazes.  s and the two points belong to F."""
    rng = np.random.default_rng(9)
    worst, excluded, features, regions = {}, {}, set(), set()
    for name, scale, p, q, vert, e1, e2 in _families(rng, 600):
        Fv, s, feature, region, x, y = ref.pair_value(p, q, vert, e1, e2)
        dist, crossing, margin = ref.truth(p, q, vert, e1, e2)
        crossed = margin > 1e-9
        clear = ~crossing & (dist > 1e-9 * scale)
        excluded[name] = float((~crossed & ~clear).mean())
        assert excluded[name] <= 0.01, (name, excluded)
        assert (Fv[crossed] == 0).all() and (feature[crossed] == 0).all(), (name, np.nonzero(crossed & (Fv != 0))[0][:5])
        assert (Fv[clear] > 0).all() and (feature[clear] > 0).all(), (name, np.nonzero(clear & (Fv == 0))[0][:5])
        assert clear.sum() >= 100 and (name not in ("soup", "large", "offset") or crossed.sum() >= 100), (name, int(clear.sum()), int(crossed.sum()))
        worst[name] = float(np.abs(np.sqrt(Fv[clear]) - dist[clear]).max())
        # x is the segment's point at s, y a point of the triangle (its distance to it is rounding), and F is their distance
        assert ((s >= 0) & (s <= 1)).all()
        P0, P1 = p.astype(D), q.astype(D)
        assert np.abs(x - (P0 + s[:, None] * (P1 - P0))).max() <= 1e-12 * (scale + np.abs(P0).max())
        A, B, Cc = ref.corners(vert, e1, e2)
        assert ref.true_dist(y, A, B, Cc).max() <= 1e-9 * (scale + np.abs(P0).max())
        assert np.abs(np.sqrt(Fv) - np.linalg.norm(x - y, axis=1)).max() <= 1e-12 * scale
        features |= set(np.unique(feature).tolist())
        regions |= set(np.unique(region).tolist())
    print("worst |sqrt(F) - truth| per family:", worst, "grazing fraction excluded:", excluded)
    assert features == set(range(6)) and regions == set(range(7)), (features, regions)
    assert set(worst) == set(WORST_ERROR)
    for name in worst:
        assert worst[name] <= 4 * WORST_ERROR[name], (name, worst)


def test_shortlist_keeps_every_winner():
    """segment_ref.brute_values evaluates only the pairs its triangle-inequality shortlist keeps: the same values, winners and tie
    counts as all pairs, on lattice segments short and long, with and without a bound"""
    nodes, prims, (p, q, md), _ = lattice_case()
    pick = np.r_[0:48, 1089:1137, 2178:2274]
    for b2 in (ref.bound2(None, len(pick)), ref.bound2(md[pick], len(pick))):
        a = ref.brute_values(p[pick], q[pick], b2, prims, cull=True)
        b = ref.brute_values(p[pick], q[pick], b2, prims, cull=False)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_fixtures_reach_what_they_are_for():
    """every feature and region wins somewhere; bit-equal F32 ties exist (the duplicated scene: all of them); "none" answers exist;
    long diagonal segments win in nodes the box-to-box bound alone would not have pruned; the lattice's tree needs more stack than
    the 12 LDS entries; stack40 has an over-long leaf"""
    from tyrant_amd import binding

    nodes, prims, (p, q, md), (dist2, prim, s, feature, region, _, _) = lattice_case()
    hit = prim >= 0
    assert set(np.unique(feature[hit]).tolist()) == set(range(6)) and set(np.unique(region[hit]).tolist()) == set(range(7))
    assert (~hit).sum() >= 100 and ((dist2 == 0) & hit).sum() >= 500
    _, arg, ties = ref.brute_values(p[:256], q[:256], ref.bound2(None, 256), prims)
    assert (ties >= 2).sum() >= 64  # a vertical segment over a grid vertex is equally near to all the triangles around it
    # the long diagonals: the segment's own box reaches over the winner's triangle and most of the others (bound (a) is 0 there)
    vert, e1, e2 = ref.records(prims)
    diag = slice(1089, 2178)
    lo, hi = np.minimum(p[diag], q[diag]), np.maximum(p[diag], q[diag])
    inside = ((vert[None, :, :2] >= lo[:, None, :2]) & (vert[None, :, :2] <= hi[:, None, :2])).all(-1)
    assert (hit[diag]).sum() >= 700 and np.median(inside.mean(axis=1)) >= 0.1
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    nodes, prims, (p, q), (_, prim, _, _, _, _, _) = duplicated_case()
    _, arg, ties = ref.brute_values(p, q, ref.bound2(None, len(p)), prims)
    assert (arg >= 0).all() and (ties >= 2).all()
    nodes, prims = build(stack40())
    assert nodes["primitiveCount"].max() == 40  # an over-long leaf: synthetic records


def test_pruning_key_never_passes_the_value_of_a_triangle_in_the_box():
    """hip/segment.hip skips a box when its key -- the larger of the box-to-box distance and the centre's distance less the half
    diagonal, reduced by kSegSlack * M + kSegFloor, squared -- is above `best`.  On a triangle's own three-corner box, and on boxes
    inflated around it, no pair may be skipped with best = its F32, for scenes at the origin and moved by 4096 and 65536, short and
    long segments, half of them parallel to an axis or a plane.  What the unreduced bound would have needed, over what the
    reduction gives, stays below one half (DESIGN.md "Closest-segment queries": 2.9x by derivation)."""
    src = open(os.path.join(ROOT, "tyrant_amd", "csrc", "hip", "segment.hip")).read()
    slack = float(re.search(r"kSegSlack = ([0-9.]+)f \* kSegUlp;", src).group(1)) * float(re.search(r"kSegUlp = ([0-9.e-]+)f;", src).group(1))
    floor = float(re.search(r"kSegFloor = ([0-9.e-]+)f;", src).group(1))
    assert 2.0 ** -24 <= slack <= 2.0 ** -16 and floor == 2.0 ** -70
    rng = np.random.default_rng(10)
    n = 30000
    worst, pairs, pruned = {}, 0, 0
    for off in (0.0, 4096.0, 65536.0):
        for long_segments in (False, True):
            vert = (rng.uniform(-50, 50, (n, 3)) + off).astype(F)
            e1, e2 = (rng.uniform(-1.5, 1.5, (n, 3)).astype(F) for _ in range(2))
            e1[::8], e2[::8] = 0, 0  # a point: its box is the point, and bound (b) is the value but for rounding
            e1[1::8, 1:], e2[1::8, 1:] = 0, 0  # a piece of a line parallel to x
            p = (vert + rng.normal(size=(n, 3)) * rng.choice([0.5, 3.0, 40.0], (n, 1))).astype(F)
            d = rng.normal(size=(n, 3)) * (60.0 if long_segments else 2.0)
            axis = rng.integers(0, 12, n)  # a quarter of the segments parallel to an axis, another quarter to a plane
            for k in range(3):
                d[(axis != k) & (axis < 3), k] = 0
                d[axis == 3 + k, k] = 0
            q = (p + d).astype(F)
            Fv = ref.pair_value(p, q, vert, e1, e2)[0]
            F32 = Fv.astype(F)
            b, c = (vert + e1).astype(F), (vert + e2).astype(F)
            lo, hi = np.minimum(np.minimum(vert, b), c), np.maximum(np.maximum(vert, b), c)
            for grow in (0.0, 0.7, 25.0):  # the triangle's own box, and larger boxes around it, off centre
                pad = (rng.random((n, 3)) * grow).astype(F), (rng.random((n, 3)) * grow).astype(F)
                blo, bhi = (lo - pad[0]).astype(F), (hi + pad[1]).astype(F)
                key, Dv, E = ref.key32(p, q, blo, bhi, slack, floor)
                assert not (key > F32).any(), (off, long_segments, grow, int((key > F32).sum()))
                need = (Dv.astype(D) - np.sqrt(F32.astype(D))) / E.astype(D)
                worst[(off, long_segments, grow)] = float(need.max())
                pairs += n
                # the key prunes: against half the pair's value it skips most boxes that are farther than that
                pruned += int((key > F32 * F(0.25)).sum())
    print("needed reduction / reduction:", worst, "pairs:", pairs, "keys above a quarter of the value:", pruned / pairs)
    assert pairs >= 500000 and max(worst.values()) <= 0.5, worst
    assert pruned / pairs >= 0.3


def test_segment_kernel_keeps_registers_and_lds_in_budget():
    """exactly one k_query_segment; no vector spills; scratch no larger than the LdsStack's private spill arrays (52 entries of 8
    bytes, plus the frame's alignment); LDS (24,576 + 7,168 bytes) that admits the three blocks per CU the launch bounds plan for,
    as tyr_query_sweep's.  The occupancy reached is printed (DESIGN.md "Closest-segment queries" records it)."""
    assert_kernel_budget("segment", "k_query_segment", 1, (64 - 12) * 8 + 16, 24576 + 7168, planned=launch_bounds_blocks("segment", "k_query_segment"))
    assert launch_bounds_blocks("segment", "k_query_segment") == launch_bounds_blocks("sweep", "k_query_sweep")


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_segment", "tyr_segment_out", hip.SegmentOut, 7)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, p, q, md=None, **kw):
    md = md if md is None or np.isscalar(md) else np.array(md)
    return tuple(x.cpu().numpy() for x in g.query_segment(np.array(p), np.array(q), md, **kw))


same = functools.partial(same_outputs, NAMES)


def check(g, prims, p, q, md=None, what=""):
    got = ask(g, p, q, md)
    want = ref.segment(p, q, prims, md)
    same(got, want, what)
    return got, want


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lattice_and_ties(hip):
    """heightfield(32): short vertical segments through and above every grid vertex (equally near to all the triangles around it),
    long diagonals across the field, seeded segments from the root box; a quarter with a bound of 2"""
    nodes, prims, (p, q, md), want = lattice_case()
    g = renderer(hip, nodes, prims)
    got = ask(g, p, q, md)
    same(got, want, "lattice")
    assert len(np.unique(got[3])) == 6 and len(np.unique(got[4])) == 7 and (got[1] < 0).any() and (got[0] == 0).any()
    same(ask(g, p[:2178], q[:2178]), ref.segment(p[:2178], q[:2178], prims), "max_dist NULL")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_exact_ties_resolve_to_the_lower_index(hip):
    """a scene concatenated with itself: every winner is the lower of the two copies' build-order indices; and 40 identical
    triangles (an over-long leaf behind synthetic records), alone and next to the Cornell box"""
    from tyrant_amd import scenes

    nodes, prims, (p, q), want = duplicated_case()
    twin = duplicated(22, 2048)[3]
    g = renderer(hip, nodes, prims)
    got = ask(g, p, q)
    same(got, want, "duplicated")
    prim = got[1]
    assert (prim >= 0).all() and (prim < twin[prim]).all()
    for tris in (stack40(), np.concatenate([scenes.cornell_box().triangles, stack40()])):
        nodes, prims = build(tris)
        g.upload(nodes, prims)
        sp, sq = aimed(np.random.default_rng(53), prims, 1500)
        (_, prim, _, _, _, _, _), _ = check(g, prims, sp, sq, what="stack40")
        stack = np.nonzero((np.ascontiguousarray(prims).view(np.uint8).reshape(len(prims), -1) == np.ascontiguousarray(stack40()[:1]).view(np.uint8)).all(axis=1))[0]
        on_stack = np.isin(prim, stack)
        assert stack.size == 40 and on_stack.any() and (prim[on_stack] == stack.min()).all()  # the first of the identical records
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slivers", [False, True])
def test_scale_and_slack(hip, slivers):
    """a soup moved by (4096, -4096, 8192), without and with slivers: segments from within 1e-3 of the surface, from the root box
    and from half way to the origin; a quarter of them parallel to an axis, some of zero length, some with a bound"""
    nodes, prims = offset_soup(slivers)
    rng = np.random.default_rng(54)
    p = np.concatenate([surface_points(rng, prims, 384, 1e-3), box_points(rng, prims, 512), (box_points(rng, prims, 128) - OFFSET * F(0.5)).astype(F)])
    n = len(p)
    d = ((surface_points(rng, prims, n, 0.5) - p) * rng.uniform(0.3, 1.7, (n, 1))).astype(F)
    d[:384] = (rng.normal(size=(384, 3)) * rng.choice([0.01, 1.0, 20.0], (384, 1))).astype(F)
    axis = rng.integers(0, 12, n)
    for k in range(3):
        d[(axis != k) & (axis < 3), k] = 0
    d[axis == 3] = 0
    q = (p + d).astype(F)
    md = rng.choice(np.array([np.inf, np.inf, 1.0, 0.05], F), n).astype(F)
    g = renderer(hip, nodes, prims)
    (dist2, prim, _, _, _, _, _), _ = check(g, prims, p, q, md, what=f"offset soup, slivers={slivers}")
    assert (prim >= 0).sum() >= n // 2 and (prim < 0).sum() >= n // 20 and ((dist2 == 0) & (prim >= 0)).sum() >= 20
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_bounds_hostile_input_and_batch_sizes(hip):
    """the Cornell box: segments from whole-number corners, axis-parallel, of zero length and longer than the room; max_dist from 0
    to larger than the room, per segment, one number and NULL; NaN / infinite / negative input; n = 0 .. 4097; a scene without
    triangles; every combination of the optional outputs"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    g = renderer(hip, nodes, prims)
    rng = np.random.default_rng(55)
    n = 6000
    lo, hi = nodes[0]["bounds"][0].astype(F), nodes[0]["bounds"][1].astype(F)
    p = (lo - 5 + (hi - lo + 10) * rng.random((n, 3))).astype(F)
    d = (rng.normal(size=(n, 3)) * rng.choice([1.0, 20.0, 400.0], (n, 1))).astype(F)
    md = rng.choice(np.array([0.0, 0.5, 3.0, 20.0, 500.0, np.inf, np.inf], F), n).astype(F)
    kind = rng.integers(0, 30, n)
    p[kind < 6] = np.round(p[kind < 6])  # whole numbers, some of them on the walls' planes
    for k in range(3):
        d[(kind < 6) & (kind % 3 != k), k] = 0  # parallel to an axis
    d[kind == 6] = 0
    q = (p + d).astype(F)
    corner = np.nonzero(kind == 7)[0]  # from one whole-number corner of the room to another
    p[corner] = np.where(rng.random((corner.size, 3)) < 0.5, lo, hi)
    q[corner] = np.where(rng.random((corner.size, 3)) < 0.5, lo, hi)
    bad = np.array([np.nan, np.inf, -np.inf], F)
    for code, arr in ((8, p), (9, q)):
        w = np.nonzero(kind == code)[0]
        arr[w, rng.integers(0, 3, w.size)] = bad[rng.integers(0, 3, w.size)]
    md[kind == 10] = rng.choice(np.array([np.nan, -1.0, -np.inf, -0.0], F), (kind == 10).sum())
    want = ref.segment(p, q, prims, md)
    invalid = np.isposinf(want[0]) & ~np.isposinf(md)
    assert invalid.sum() >= n // 15 and (want[1] < 0).sum() >= n // 6 and (want[1][corner] >= 0).sum() >= corner.size // 2
    got = ask(g, p, q, md)
    same(got, want, "cornell")
    same(ask(g, p[:1500], q[:1500]), ref.segment(p[:1500], q[:1500], prims), "max_dist NULL")
    same(ask(g, p[:1500], q[:1500], 3.0), ref.segment(p[:1500], q[:1500], prims, F(3.0)), "one number as max_dist")
    for m in (0, 1, 63, 64, 65, 4097):  # every prefix answers as the whole batch did
        same(ask(g, p[:m], q[:m], md[:m]), tuple(a[:m] for a in want), f"n = {m}")
    # optional outputs NULL, in every combination, through the C call; the arrays not passed stay untouched
    m = 1000
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a[:m])).cuda()  # noqa: E731
    tp, tq, tm = on(p), on(q), on(md)
    P = C.c_void_p
    kinds = (((), torch.float32), ((), torch.int32), ((), torch.float32), ((), torch.uint8), ((), torch.uint8), ((3,), torch.float32), ((3,), torch.float32))
    for use in itertools.product((False, True), repeat=5):
        outs = [torch.full((m, *shape), 7, dtype=dtype).cuda() for shape, dtype in kinds]
        torch.cuda.synchronize()
        used = (True, True) + use
        out = hip.SegmentOut(*[x.data_ptr() if u else None for x, u in zip(outs, used)])
        assert hip.lib().tyr_query_segment(g.h, m, P(tp.data_ptr()), P(tq.data_ptr()), P(tm.data_ptr()), 0, C.byref(out), None) == 0
        assert g.query_error() == 0
        res = [x.cpu().numpy() for x in outs]
        same_outputs([nm for nm, u in zip(NAMES, used) if u], [x for x, u in zip(res, used) if u], [w[:m] for w, u in zip(want, used) if u], f"outputs {use}")
        assert all((x == 7).all() for x, u in zip(res, used) if not u), use
    # a scene without triangles: every valid segment "none"
    g.upload(*no_triangles())
    same(ask(g, p, q, md), ref.segment(p, q, prims[:0], md), "empty scene")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_segment_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with segment queries between its tyr_render calls: the same accumulation buffer and
    counters as without them"""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    rng = np.random.default_rng(56)
    n = 20000
    p = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(5, 80, n)], axis=1).astype(F)
    q = (p + rng.normal(size=(n, 3)) * 20).astype(F)
    want = ref.segment(p, q, prims)

    def between(g):
        same(ask(g, p, q), want, "between two renders")
        ask(g, p, q, 0.5)

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the answers to the refitted scene's; a torch side stream and the ctx's stream work; bad
    arguments are refused before any launch; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(16))
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    rng = np.random.default_rng(57)
    n = 1000
    p, q = aimed(rng, prims, n, reach=(0.3, 0.9))
    check(g, prims, p, q, what="before the refit")
    moved = deformed(prims, 4.0)
    g.refit(moved)
    got, want = check(g, moved, p, q, what="after the refit")
    assert not np.array_equal(want[1], ref.segment(p, q, prims)[1])
    # a side stream, device tensors taken in place; then the ctx's own stream (NULL) through the C call
    tp, tq = (torch.from_numpy(a).cuda() for a in (p, q))
    tm = torch.full((n,), 1.5).cuda()
    res, side = on_side_stream(lambda side: (g.query_segment(tp, tq, tm, stream=side), side))
    near = ref.segment(p, q, moved, np.full(n, 1.5, F))
    same(tuple(x.cpu().numpy() for x in res), near, "side stream")
    # a number as max_dist on a side stream named from outside its context: the tensor it becomes is filled on the current
    # stream, behind work that keeps it busy, and the query on `side` has to wait for that fill
    busy = torch.randn(2048, 2048, device="cuda")
    for _ in range(8):
        busy = busy @ busy * 1e-3
    res = g.query_segment(tp, tq, 1.5, stream=side)
    side.synchronize()
    same(tuple(x.cpu().numpy() for x in res), near, "one number as max_dist on a side stream")
    del busy

    L, h, P = hip.lib(), g.h, C.c_void_p
    dist2, prim = torch.full((n,), 7.0).cuda(), torch.full((n,), 7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    none5 = (None,) * 5
    ok = hip.SegmentOut(dist2.data_ptr(), prim.data_ptr(), *none5)
    pp, pq, pm = P(tp.data_ptr()), P(tq.data_ptr()), P(tm.data_ptr())
    assert L.tyr_query_segment(h, n, pp, pq, pm, 0, C.byref(ok), None) == 0
    assert g.query_error() == 0  # (waits for the ctx's stream)
    same((dist2.cpu().numpy(), prim.cpu().numpy()), near[:2], "the ctx's stream")
    before = prim.cpu().numpy().copy()
    inv = hip.TYR_ERR_INVALID
    assert L.tyr_query_segment(None, 4, pp, pq, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_segment(h, 4, None, pq, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_segment(h, 4, pp, None, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_segment(h, 4, pp, pq, None, 0, None, None) == inv
    assert L.tyr_query_segment(h, 4, pp, pq, None, 0, C.byref(hip.SegmentOut(None, prim.data_ptr(), *none5)), None) == inv
    assert L.tyr_query_segment(h, 4, pp, pq, None, 0, C.byref(hip.SegmentOut(dist2.data_ptr(), None, *none5)), None) == inv
    assert L.tyr_query_segment(h, 4, pp, pq, None, 1, C.byref(ok), None) == inv  # flags must be 0
    assert L.tyr_query_segment(h, 1 << 31, pp, pq, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_segment(h, 0, None, None, None, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_segment(empty.h, 4, pp, pq, None, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_segment(tp.double(), tq)
    with pytest.raises(ValueError):
        g.query_segment(tp, tq[:, :2].contiguous())
    with pytest.raises(ValueError):
        g.query_segment(tp, tq[:5])
    with pytest.raises(ValueError):
        g.query_segment(tp, tq, tm[:5])
    assert np.array_equal(prim.cpu().numpy(), before)  # the refused calls wrote nothing
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_c3_tree(hip):
    """one pass on C3's 1 M-triangle tree: the 256 segments of tests/golden/segment_c3.npz (p within 1.5 of the surface, lengths from
    0 to tens of cells, every fourth with a bound) against the seven answers tools/segment_c3_golden.py recorded from the
    restatement's brute force.  Every run checks that the file belongs to these triangles, recomputes one segment by brute force
    and evaluates the winners' pairs from the restatement."""
    sc, nodes, prims = built_scene("mesh706")
    z = np.load(C3_ANSWERS)
    assert str(z["digest"]) == hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest(), "the recorded answers belong to other triangles"
    p, q, md = z["p"], z["q"], z["max_dist"]
    want = tuple(z[k] for k in NAMES)
    arg = want[1].astype(np.int64)
    assert len(p) == 256 and (arg >= 0).sum() >= 128 and (arg < 0).sum() >= 16 and (want[0][arg >= 0] == 0).sum() >= 16
    live = int(np.random.default_rng(58).integers(0, 256))
    lb, la, _ = ref.brute_values(p[live:live + 1], q[live:live + 1], ref.bound2(md[live:live + 1], 1), prims, cull=False)
    assert int(la[0]) == int(arg[live]) and (la[0] < 0 or bits(lb)[0] == bits(want[0])[live])
    same(ref.answers(p, q, ref.bound2(md, 256), ref.valid_inputs(p, q, md), arg, prims), want, "the recorded answers against the restatement")
    g = renderer(hip, nodes, prims)
    same(ask(g, p, q, md), want, "C3")
    assert g.query_error() == 0
    g.close()
