"""Batched closest-triangle distance queries on the uploaded scene (tyr_query_tri_distance, hip/tri_distance.hip;
Renderer.query_tri_distance): the least distance between a caller's triangle and the mesh of include/tyr_c.h "Closest-triangle
queries" as an argmin over all triangles, bit for bit against its numpy restatement (tests/tri_distance_ref.py) by brute force --
the definition has no traversal order in it, so nothing else is needed as an oracle.

CPU: the restatement by hand, the restatement against a binary64 truth (a nested ternary search, and exact integer arithmetic
for contact), the pruning key against the value, what the fixtures are for, the degenerate query against tyr_query_segment's
restatement, what the compiler made of the kernel, the ABI.  GPU: lattices with shared edges and vertices, exact ties by index,
over-long leaves, offset scenes and slivers, scene shapes and tuning profiles, bounds, hostile input, batch sizes, optional
outputs, skip_shared on the mesh's own triangles, isolation from the render, refit, streams, argument checks, and one pass on
C3's 1 M-triangle tree.

Code 5 (the scene edge B -> C crosses the query) decides only through rounding: in exact arithmetic a query's cut through the
scene triangle's plane that enters through B -> C leaves through A -> B or A -> C (code 3 or 4, also F = 0, offered first) or
ends in the scene triangle, where a query edge crosses it (codes 0-2; an edge that lies in the plane has h0 == h1 and is seen by
no crossing rule, but the edges beside it start in the plane and cross at s = 0 or 1).  In the contract's binary64 the crossing
point rounds, and a query whose rim passes through a point of B -> C can fail codes 0-4 by one rounding and pass code 5: a hand
case with whole-number corners and the lattice fixture's through_edges queries have it as the decider."""
import ctypes as C
import functools
import hashlib
import itertools
import os
import re

import numpy as np
import pytest

import nearest_ref
import segment_ref
import tri_distance_ref as ref
from conftest import GOLDEN, ROOT, bits, built_scene
from query_support import (OFFSET, assert_kernel_budget, assert_query_abi, assert_render_undisturbed, build, deformed, duplicated, lattice, launch_bounds_blocks, no_triangles,
                           offset_soup, on_side_stream, query_exists, renderer, stack40, surface_points, tri)
from query_support import same as same_outputs

F = np.float32
D = np.float64
C3_ANSWERS = os.path.join(GOLDEN, "tri_distance_c3.npz")
NAMES = ref.NAMES
CODES = set(range(21))
# |sqrt(F) - truth| of the restatement on the committed seeds, per family, rounded up to two digits (test_restatement_against_truth
# prints the figure and holds it to these; DESIGN.md "Closest-triangle queries" has the same table); ERROR_BOUND, which other seeds
# are held to: the maximum times 4, rounded up to a power of ten
WORST_ERROR = {"lattice": 1.5e-14, "soup": 1.7e-14, "offset soup": 2.4e-12, "offset slivers": 1.6e-12}
ERROR_BOUND = 1e-11

_the_query_exists = query_exists("tyr_query_tri_distance")


# ---- fixtures (numpy only) --------------------------------------------------------------------------------------------
def around(rng, centre, size):
    """seeded triangles whose corners lie within about `size` (a number or one per triangle) of the points `centre`"""
    n = len(centre)
    size = np.broadcast_to(np.asarray(size, D), (n,))[:, None]
    return tuple((centre + rng.normal(size=(n, 3)) * size * 0.5).astype(F) for _ in range(3))


def own_triangles(prims):
    vert, e1, e2 = ref.records(prims)
    return vert.copy(), (vert + e1).astype(F), (vert + e2).astype(F)


def through_edges(rng, prims, n):
    """seeded triangles whose edge a -> b has its midpoint at the binary32 point t / 8 (t = 1 .. 7) along a seeded scene triangle's
    edge B -> C, the corners quarter and half steps from it.  In exact arithmetic a rim that meets B -> C also meets A -> B or
    A -> C, or the scene triangle's face, at F = 0 (codes 0-4); in the contract's binary64 the crossing point s = h0 / (h0 - h1)
    rounds, codes 0-4 can fail their closed tests by one rounding while code 5 passes, and then code 5 decides: on these queries
    for about one pair in a hundred."""
    vert, e1, e2 = ref.records(prims)
    B, Cc = (vert + e1).astype(F), (vert + e2).astype(F)
    i = rng.integers(0, len(vert), n)
    t = rng.integers(1, 8, n)[:, None] / 8.0
    m = (B[i].astype(D) + t * (Cc[i].astype(D) - B[i])).astype(F)
    d = rng.integers(-8, 9, (n, 3)).astype(F) * F(0.25)
    return (m + d).astype(F), (m - d).astype(F), (m + rng.integers(-8, 9, (n, 3)).astype(F) * F(0.5)).astype(F)


@functools.lru_cache(maxsize=None)
def lattice_case():
    """heightfield(16), cells 6.25 across: 1536 seeded triangles about one cell edge across around points within 3 of the surface,
    256 of a tenth of that, 256 four cells across, 256 flat ones at a whole-number height over grid cells (equally near to
    several triangles), and 1024 whose edge a -> b has its midpoint on a lattice edge B -> C (through_edges: where code 5
    decides); a quarter of all with a bound of 2 -- (nodes, prims, queries, answers)"""
    nodes, prims, grid, _ = lattice(16, 31)
    rng = np.random.default_rng(61)
    a, b, c = around(rng, surface_points(rng, prims, 2048, 3.0), np.r_[np.full(1536, 6.25), np.full(256, 0.6), np.full(256, 25.0)])
    g = grid[rng.integers(0, len(grid), 256)] + np.array([0, 0, 2], F)
    flat = [(g + np.array(o, F)).astype(F) for o in ((0, 0, 0), (6.25, 0, 0), (0, 6.25, 0))]
    a, b, c = (np.concatenate([x, y, z]) for x, y, z in zip((a, b, c), flat, through_edges(np.random.default_rng(71), prims, 1024)))
    md = rng.choice(np.array([np.inf, np.inf, np.inf, 2.0], F), len(a)).astype(F)
    q = tuple(np.ascontiguousarray(x) for x in (a, b, c, md))
    return nodes, prims, q, ref.tri_distance(a, b, c, prims, md)


@functools.lru_cache(maxsize=None)
def duplicated_case():
    nodes, prims, pts, _ = duplicated(32, 256)
    rng = np.random.default_rng(62)
    q = around(rng, pts[:512], 6.25)
    return nodes, prims, q, ref.tri_distance(*q, prims)


@functools.lru_cache(maxsize=None)
def self_case():
    """the lattice's own triangles as queries, with a bound of 5: (nodes, prims, queries, answers without the flag, with it)"""
    nodes, prims, _, _ = lattice(16, 31)
    q = own_triangles(prims)
    return nodes, prims, q, ref.tri_distance(*q, prims, F(5.0)), ref.tri_distance(*q, prims, F(5.0), skip_shared=True)


@functools.lru_cache(maxsize=None)
def soup_case(slivers):
    """offset_soup: 2048 triangles around points within 2 of the surface, sizes log-uniform from 1e-3 to the scene's diagonal; a
    quarter with a bound of 1, some with 0.05"""
    nodes, prims = offset_soup(slivers)
    rng = np.random.default_rng(63 + int(slivers))
    vert = np.concatenate(own_triangles(prims))
    diag = float(np.linalg.norm(vert.max(0).astype(D) - vert.min(0)))
    n = 2048
    a, b, c = around(rng, surface_points(rng, prims, n, 2.0), 10.0 ** rng.uniform(-3, np.log10(diag), n))
    md = rng.choice(np.array([np.inf, np.inf, 1.0, 0.05], F), n).astype(F)
    return nodes, prims, (a, b, c, md), ref.tri_distance(a, b, c, prims, md)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
V0, V1, FAR0, FAR1, FAR2 = (0.5, -1, -1), (0.5, -1, 1), (0.5, -5, 0), (-5, 0.5, 0), (4, 4, 0)
W0, W1, H0, H1 = (-1, 0.5, -1), (-1, 0.5, 1), (1.5, 1.5, -1), (1.5, 1.5, 1)
HAND = [  # the scene triangle A (0,0,0), B (1,0,0), C (0,1,0): a, b, c, F, code, region, on_query, on_triangle
    ((0.25, 0.25, 1), (0.25, 0.25, -1), (5, 5, 1), 0.0, 0, 0, (0.25, 0.25, 0), (0.25, 0.25, 0)),  # a query edge through the face
    ((5, 5, 1), (0.25, 0.25, 1), (0.25, 0.25, -1), 0.0, 1, 0, (0.25, 0.25, 0), (0.25, 0.25, 0)),
    ((0.25, 0.25, -1), (5, 5, 1), (0.25, 0.25, 1), 0.0, 2, 0, (0.25, 0.25, 0), (0.25, 0.25, 0)),
    # A -> B pierces the query's interior and no query edge touches the scene triangle (B -> C pierces it too: code 3 stays)
    ((0.5, -1, -1), (0.5, 1, -1), (0.5, 0, 2), 0.0, 3, 4, (0.5, 0, 0), (0.5, 0, 0)),
    ((-1, 0.5, -1), (1, 0.5, -1), (0, 0.5, 2), 0.0, 4, 5, (0, 0.5, 0), (0, 0.5, 0)),  # A -> C, and B -> C beside it
    ((0.25, 0.25, 1), (1.25, 0.25, 2), (0.25, 1.25, 2), 1.0, 6, 0, (0.25, 0.25, 1), (0.25, 0.25, 0)),  # a query corner over the face
    ((0.25, 1.25, 2), (0.25, 0.25, 1), (1.25, 0.25, 2), 1.0, 7, 0, (0.25, 0.25, 1), (0.25, 0.25, 0)),
    ((1.25, 0.25, 2), (0.25, 1.25, 2), (0.25, 0.25, 1), 1.0, 8, 0, (0.25, 0.25, 1), (0.25, 0.25, 0)),
    # a large query in the parallel plane z = 1: the three scene corners face its interior at the same F, the lowest code stays
    ((-2, -2, 1), (4, -2, 1), (-2, 4, 1), 1.0, 9, 1, (0, 0, 1), (0, 0, 0)),
    ((-2, -4, 4), (4, -4, -2), (1, 6, 1), 0.5, 10, 2, (1.5, 0, 0.5), (1, 0, 0)),  # the plane x + z = 2: B faces the interior
    ((-4, -2, 4), (6, 1, 1), (-4, 4, -2), 0.5, 11, 3, (0, 1.5, 0.5), (0, 1, 0)),  # the plane y + z = 2: C
    (V0, V1, FAR0, 1.0, 12, 4, (0.5, -1, 0), (0.5, 0, 0)),  # the edge pairs: a query edge across a scene edge, outside it
    (W0, W1, FAR1, 1.0, 13, 5, (-1, 0.5, 0), (0, 0.5, 0)),
    (H0, H1, FAR2, 2.0, 14, 6, (1.5, 1.5, 0), (0.5, 0.5, 0)),
    (FAR0, V0, V1, 1.0, 15, 4, (0.5, -1, 0), (0.5, 0, 0)),
    (FAR1, W0, W1, 1.0, 16, 5, (-1, 0.5, 0), (0, 0.5, 0)),
    (FAR2, H0, H1, 2.0, 17, 6, (1.5, 1.5, 0), (0.5, 0.5, 0)),
    (V1, FAR0, V0, 1.0, 18, 4, (0.5, -1, 0), (0.5, 0, 0)),
    (W1, FAR1, W0, 1.0, 19, 5, (-1, 0.5, 0), (0, 0.5, 0)),
    (H1, FAR2, H0, 2.0, 20, 6, (1.5, 1.5, 0), (0.5, 0.5, 0)),
    ((2, 0, 0), (3, 0, 0), (2, 1, 0), 1.0, 6, 2, (2, 0, 0), (1, 0, 0)),  # coplanar and apart: corner to corner, codes 6 10 12.. tie
    ((0.25, 0.25, 0), (3, 0.25, 0), (0.25, 3, 0), 0.0, 6, 0, (0.25, 0.25, 0), (0.25, 0.25, 0)),  # coplanar and overlapping: no crossing in a plane
    ((0.5, -1, 1), (0.5, -1, 2), (0.5, -3, 1), 2.0, 6, 4, (0.5, -1, 1), (0.5, 0, 0)),  # a corner nearest to an edge: 6 ties with 12, 13..
    ((0.25, 0.25, 1), (0.25, 0.25, 1), (0.25, 0.25, 1), 1.0, 6, 0, (0.25, 0.25, 1), (0.25, 0.25, 0)),  # a point
    ((0.25, 0.25, 1), (0.25, 0.25, -1), (0.25, 0.25, -1), 0.0, 0, 0, (0.25, 0.25, 0), (0.25, 0.25, 0)),  # a segment through the face
    ((-1, 0.5, 1), (-1, 0.5, -1), (-1, 0.5, 1), 1.0, 13, 5, (-1, 0.5, 0), (0, 0.5, 0)),  # a segment across A -> C
    # code 5, on the scene triangle A (-6,5,-7), B (-7,8,-11), C (-11,6,-13): the query edge a -> b passes through (-9,7,-12), the
    # midpoint of B -> C, at s = 1/2.  In exact arithmetic code 0 has it (on the rim: bv + bw == nn); in binary64 h0 / (h0 - h1) and
    # the point built from it round, codes 0-4 fail their closed tests, and B -> C against the query -- whose crossing at s = 1/2
    # is exact -- decides
    ((-7, -3, 0), (-11, 17, -24), (-15, 13, -12), 0.0, 5, 6, (-9, 7, -12), (-9, 7, -12), ((-6, 5, -7), (-1, 3, -4), (-5, 1, -6))),
]


def one(a, b, c, md=None, prims=None, **kw):
    prims = tri((0, 0, 0), (1, 0, 0), (0, 1, 0)) if prims is None else prims
    res = ref.tri_distance(np.array([a], F), np.array([b], F), np.array([c], F), prims, None if md is None else np.array([md], F), **kw)
    return tuple(x[0] for x in res)


def test_hand_cases():
    """exactly representable numbers on the unit right triangle: every one of the 21 codes as the decider, parallel and coplanar pairs, a mesh
    edge through the query's interior and a mesh vertex facing it (what queries on the corners and the edges get wrong), queries
    and scene triangles of zero area, equal F between codes; the argmin; the strict bound; every invalid input; rule 0"""
    codes = set()
    for a, b, c, dist2, feature, region, x, y, *scene in HAND:
        got = one(a, b, c, prims=tri(*scene[0]) if scene else None)
        assert (int(got[1]), int(got[2]), int(got[3])) == (0, feature, region), (a, b, c, got)
        assert float(got[0]) == dist2 and got[4].tolist() == list(map(float, x)) and got[5].tolist() == list(map(float, y)), (a, b, c, got)
        codes.add(feature)
    assert codes == CODES
    unit = tri((0, 0, 0), (1, 0, 0), (0, 1, 0))
    # the mesh edge through the interior: tyr_query_segment on the three edges does not see it; the mesh vertex facing the interior:
    # neither do tyr_query_nearest on the corners nor the segments
    for k, least in ((3, 0.01), (8, 1.5)):
        P = [np.array([v], F) for v in HAND[k][:3]]
        seg = min(float(segment_ref.segment(P[i], P[(i + 1) % 3], unit)[0][0]) for i in range(3))
        pts = min(float(nearest_ref.nearest(P[i], unit)[0][0]) for i in range(3))
        assert seg >= least > HAND[k][3] and pts >= seg, (k, seg, pts)
    # scene triangles of zero area: e2 = 2 e1 (a piece of a line) under a query corner, and the zero triangle (its one point, which
    # faces the interior of a query above it: the three corner codes tie)
    got = one((1.5, 0.5, 1), (1.5, 1.5, 2), (2.5, 0.5, 2), prims=tri((0, 0, 0), (1, 0, 0), (2, 0, 0)))
    assert (float(got[0]), int(got[1]), int(got[2]), int(got[3]), got[5].tolist()) == (1.25, 0, 6, 5, [1.5, 0, 0])
    got = one((-1, -1, 1), (2, -1, 1), (-1, 2, 1), prims=tri((0, 0, 0), (0, 0, 0), (0, 0, 0)))
    assert (float(got[0]), int(got[1]), int(got[2]), int(got[3]), got[4].tolist(), got[5].tolist()) == (1.0, 0, 9, 1, [0, 0, 1], [0, 0, 0])
    # the bound is strict: at exactly max_dist "none" (dist2 = bound2, both points a), one binary32 step more: found
    q = HAND[5][:3]
    got = one(*q, 1.0)
    assert (float(got[0]), int(got[1]), int(got[2]), int(got[3])) == (1.0, -1, 0, 0) and got[4].tolist() == got[5].tolist() == [0.25, 0.25, 1]
    assert int(one(*q, np.nextafter(F(1), F(2)))[1]) == 0
    assert (float(one(*q, 0.5)[0]), int(one(*HAND[0][:3], 0.0)[1])) == (0.25, -1)  # F = 0 is not < 0
    # the argmin: the lowest index of equal F32; every invalid input; max_dist = +inf and -0 are valid
    three = np.concatenate([tri((0, 0, 5), (1, 0, 0), (0, 1, 0)), unit, unit])
    nan, inf = np.nan, np.inf
    a, b, c = (np.array([v] * 10, F) for v in q)
    md = np.full(10, 8.0, F)
    a[1, 0], a[2, 2], b[3, 1], b[4, 0], c[5, 2], md[6], md[7], md[8], md[9] = nan, -inf, nan, inf, nan, nan, -1.0, inf, -0.0
    got = ref.tri_distance(a, b, c, three, md)
    assert got[1].tolist() == [1] + [-1] * 7 + [1, -1] and float(got[0][0]) == 1.0 and np.isposinf(got[0][1:8]).all() and float(got[0][9]) == 0.0
    assert np.array_equal(bits(got[4][1:8]), bits(a[1:8])) and np.array_equal(bits(got[5][1:8]), bits(a[1:8])) and not got[2][1:8].any() and not got[3][1:8].any()
    none = ref.tri_distance(a[:1], b[:1], c[:1], three[:0])
    assert none[1].tolist() == [-1] and np.isposinf(none[0]).all()  # no triangles: none
    # rule 0: a query that shares a corner with the nearer triangle answers with the other one, -0 equals +0
    two = np.concatenate([unit, tri((0, 0, 3), (1, 0, 0), (0, 1, 0))])
    for corner in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (1.0, 0.0, 0.0)):
        P = (np.array([corner], F), np.array([[5, 5, 1]], F), np.array([[5, 6, 1]], F))
        assert ref.tri_distance(*P, two)[1].tolist() == [0] and ref.tri_distance(*P, two, skip_shared=True)[1].tolist() == [1]
    assert ref.tri_distance(*P, unit, skip_shared=True)[1].tolist() == [-1]


def _families(n):
    """(name, scale, a, b, c, vert, e1, e2) of seeded pairs on the GPU tests' scenes: every query with the triangle the
    restatement answers (the near pairs: contacts and small gaps) and with a seeded other one"""
    from tyrant_amd import scenes

    rng = np.random.default_rng(19)
    soup = build(scenes.random_soup(2000))
    for name, (nodes, prims), size in (("lattice", lattice(16, 31)[:2], 6.25), ("soup", soup, 1.0), ("offset soup", offset_soup(False), 1.0), ("offset slivers", offset_soup(True), 1.0)):
        half = n // 2
        a, b, c = around(rng, surface_points(rng, prims, half, 0.3), size * 10.0 ** rng.uniform(-1.5, 1.0, half))
        near = ref.tri_distance(a, b, c, prims)[1].astype(np.int64)
        pick = np.concatenate([near, rng.integers(0, len(prims), half)])
        if name == "offset slivers":
            pick[half:] = rng.integers(0, len(prims) // 10, half) * 10  # the slivers themselves
        vert, e1, e2 = (x[pick] for x in ref.records(prims))
        vertex = np.concatenate(own_triangles(prims))
        yield (name, float(np.linalg.norm(vertex.max(0).astype(D) - vertex.min(0))), np.tile(a, (2, 1)), np.tile(b, (2, 1)), np.tile(c, (2, 1)), vert, e1, e2)


def test_restatement_against_truth():
    """the restatement against the least distance of a point of the query to the scene triangle (a nested ternary search over the
    query's barycentrics of nearest_ref.true_dist2: the function is convex) and against tri_ref.pair_exact (the overlap rules in
    exact integer arithmetic): a pair that touches has truth 0, and F below (1e-9 of the scene's diagonal)^2; a pair farther
    apart than 1e-9 of the diagonal has F > 0 and sqrt(F) within ERROR_BOUND of the truth.  x and y belong to F."""
    worst, counts, codes = {}, {}, set()
    for name, scale, a, b, c, vert, e1, e2 in _families(400):
        Fv, feature, region, x, y = ref.pair_value(a, b, c, vert, e1, e2)
        touch = ref.touching(a, b, c, vert, e1, e2)
        dist = np.where(touch, 0.0, ref.truth(a, b, c, vert, e1, e2))
        clear = ~touch & (dist > 1e-9 * scale)
        assert (np.sqrt(Fv[touch]) <= 1e-9 * scale).all(), (name, float(np.sqrt(Fv[touch]).max()))
        assert (Fv[clear] > 0).all() and (feature[clear] >= 6).all(), name
        counts[name] = (int(touch.sum()), int(clear.sum()))
        assert touch.sum() >= 20 and clear.sum() >= 200, (name, counts)
        worst[name] = float(np.abs(np.sqrt(Fv[clear]) - dist[clear]).max())
        # x is a point of the query and y one of the scene triangle (their distances to them are rounding), and F is their distance
        P0 = a.astype(D)
        A, B, Cc = ref.corners(vert, e1, e2)
        room = 1e-9 * (scale + np.abs(P0).max())
        assert ref.true_dist(x, P0, b.astype(D), c.astype(D)).max() <= room and ref.true_dist(y, A, B, Cc).max() <= room
        assert np.abs(np.sqrt(Fv) - np.linalg.norm(x - y, axis=1)).max() <= 1e-12 * scale
        codes |= set(np.unique(feature).tolist())
    print("worst |sqrt(F) - truth| per family:", worst, "(touching, clear) pairs:", counts, "codes:", sorted(codes))
    assert set(worst) == set(WORST_ERROR)
    assert ERROR_BOUND == 10.0 ** np.ceil(np.log10(4 * max(WORST_ERROR.values())))
    for name in worst:
        assert worst[name] <= WORST_ERROR[name] <= ERROR_BOUND, (name, worst)


def test_shortlist_keeps_every_winner():
    """tri_distance_ref.brute_values evaluates only the pairs its triangle-inequality shortlist keeps: the same values, winners and
    tie counts as all pairs, on lattice queries small and large, with and without a bound, and with skip_shared on the mesh's own"""
    nodes, prims, (a, b, c, md), _ = lattice_case()
    pick = np.r_[0:48, 1536:1560, 1792:1816, 2048:2072]
    for b2 in (ref.bound2(None, len(pick)), ref.bound2(md[pick], len(pick))):
        x = ref.brute_values(a[pick], b[pick], c[pick], b2, prims, cull=True)
        y = ref.brute_values(a[pick], b[pick], c[pick], b2, prims, cull=False)
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    qa, qb, qc = (v[:64] for v in own_triangles(prims))
    x = ref.brute_values(qa, qb, qc, ref.bound2(None, 64), prims, skip_shared=True, cull=True)
    y = ref.brute_values(qa, qb, qc, ref.bound2(None, 64), prims, skip_shared=True, cull=False)
    assert all(np.array_equal(u, v) for u, v in zip(x, y))


def test_fixtures_reach_what_they_are_for():
    """on the restatement's answers for the fixtures the GPU tests use: every one of the 21 codes (5 on the through_edges queries, see the
    head of this module) and every region win somewhere; bit-equal F32 ties exist (the duplicated scene: all of them); "none" by the bound
    exists; skip_shared removes a would-be winner for every one of the mesh's own triangles; the lattice's tree needs more stack
    than the 12 LDS entries; stack40 has an over-long leaf"""
    from tyrant_amd import binding

    nodes, prims, (a, b, c, md), (dist2, prim, feature, region, _, _) = lattice_case()
    hit = prim >= 0
    codes = set(np.unique(feature[hit]).tolist())
    for slivers in (False, True):
        s = soup_case(slivers)[3]
        codes |= set(np.unique(s[2][s[1] >= 0]).tolist())
        assert (s[1] < 0).sum() >= 100 and (s[1] >= 0).sum() >= 1000 and ((s[0] == 0) & (s[1] >= 0)).sum() >= 100
    assert codes >= CODES, sorted(CODES - codes)
    assert set(np.unique(region[hit]).tolist()) == set(range(7))
    assert (~hit & np.isfinite(dist2)).sum() >= 50 and ((dist2 == 0) & hit).sum() >= 300
    _, arg, ties = ref.brute_values(a[2048:2304], b[2048:2304], c[2048:2304], ref.bound2(None, 256), prims)
    assert (ties >= 2).sum() >= 64  # a flat triangle at a whole-number height over the grid is equally near to several triangles
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    nodes, prims, q, _ = duplicated_case()
    _, arg, ties = ref.brute_values(*q, ref.bound2(None, len(q[0])), prims)
    assert (arg >= 0).all() and (ties >= 2).all()
    nodes, prims, q, plain, skipped = self_case()
    assert (plain[0] == 0).all() and (plain[1] >= 0).all()  # itself or a neighbour, at distance 0
    assert (skipped[1] != plain[1]).all() and (skipped[1] >= 0).sum() >= 100 and (skipped[1] < 0).sum() >= 1
    nodes, prims = build(stack40())
    assert nodes["primitiveCount"].max() == 40  # an over-long leaf: synthetic records


def test_pruning_key_never_passes_the_value_of_a_triangle_in_the_box():
    """hip/tri_distance.hip skips a box when its key -- the distance between the box and the query's own box, reduced by
    kTdSlack * M + kTdFloor, squared -- is above `best`.  On a triangle's own three-corner box, and on boxes inflated around it,
    no pair may be skipped with best = its F32, for the soup at the origin and moved by 4096 and 65536, with slivers, small and
    large queries, a quarter of them flat in a coordinate plane or thin along an axis, and for the GPU tests' lattice, offset soup
    and offset sliver fixtures.  What the unreduced bound would have
    needed, over what the reduction gives, stays below one half (DESIGN.md "Closest-triangle queries": 3.2x by derivation)."""
    src = open(os.path.join(ROOT, "tyrant_amd", "csrc", "hip", "tri_distance.hip")).read()
    slack = float(re.search(r"kTdSlack = ([0-9.]+)f \* kTdUlp;", src).group(1)) * float(re.search(r"kTdUlp = ([0-9.e-]+)f;", src).group(1))
    floor = float(re.search(r"kTdFloor = ([0-9.e-]+)f;", src).group(1))
    assert 2.0 ** -24 <= slack <= 2.0 ** -16 and floor == 2.0 ** -70
    rng = np.random.default_rng(20)
    n = 20000
    worst, pairs, pruned = {}, 0, 0
    for off in (0.0, 4096.0, 65536.0):
        for large in (False, True):
            vert = (rng.uniform(-50, 50, (n, 3)) + off).astype(F)
            e1, e2 = (rng.uniform(-1.5, 1.5, (n, 3)).astype(F) for _ in range(2))
            e1[::8], e2[::8] = 0, 0  # a point
            e2[1::8] = (F(0.75) * e1[1::8] + (1e-5 * rng.normal(size=e1[1::8].shape)).astype(F)).astype(F)  # a sliver
            centre = vert + rng.normal(size=(n, 3)) * rng.choice([0.5, 3.0, 40.0], (n, 1))
            a, b, c = around(rng, centre, 60.0 if large else 2.0)
            axis = rng.integers(0, 12, n)
            for k in range(3):  # flat in a coordinate plane: an axis on which the two boxes' gap is the whole distance
                b[axis == k, k], c[axis == k, k] = a[axis == k, k], a[axis == k, k]
            Fv = ref.pair_value(a, b, c, vert, e1, e2)[0]
            F32 = Fv.astype(F)
            vb, vc = (vert + e1).astype(F), (vert + e2).astype(F)
            lo, hi = np.minimum(np.minimum(vert, vb), vc), np.maximum(np.maximum(vert, vb), vc)
            for grow in (0.0, 0.7, 25.0):  # the triangle's own box, and larger boxes around it, off centre
                pad = (rng.random((n, 3)) * grow).astype(F), (rng.random((n, 3)) * grow).astype(F)
                blo, bhi = (lo - pad[0]).astype(F), (hi + pad[1]).astype(F)
                key, Dv, E = ref.key32(a, b, c, blo, bhi, slack, floor)
                assert not (key > F32).any(), (off, large, grow, int((key > F32).sum()))
                need = (Dv.astype(D) - np.sqrt(F32.astype(D))) / E.astype(D)
                worst[(off, large, grow)] = float(need.max())
                pairs += n
                pruned += int((key > F32 * F(0.25)).sum())
    # the GPU tests' own families: every fixture query against the triangle it answers with and a seeded other one
    for name, (nodes, prims, q, want) in (("lattice", lattice_case()), ("offset soup", soup_case(False)), ("offset slivers", soup_case(True))):
        a, b, c = q[:3]
        vert, e1, e2 = ref.records(prims)
        for j in (np.where(want[1] >= 0, want[1], 0).astype(np.int64), rng.integers(0, len(prims), len(a))):
            F32 = ref.pair_value(a, b, c, vert[j], e1[j], e2[j])[0].astype(F)
            vb, vc = (vert[j] + e1[j]).astype(F), (vert[j] + e2[j]).astype(F)
            lo, hi = np.minimum(np.minimum(vert[j], vb), vc), np.maximum(np.maximum(vert[j], vb), vc)
            for grow in (0.0, 5.0):
                pad = (rng.random((len(a), 3)) * grow).astype(F)
                key, Dv, E = ref.key32(a, b, c, (lo - pad).astype(F), (hi + pad).astype(F), slack, floor)
                assert not (key > F32).any(), (name, grow, int((key > F32).sum()))
                worst[(name, grow)] = max(worst.get((name, grow), 0.0), float(((Dv.astype(D) - np.sqrt(F32.astype(D))) / E.astype(D)).max()))
                pairs += len(a)
    print("needed reduction / reduction:", worst, "largest:", max(worst.values()), "pairs:", pairs, "keys above a quarter of the value:", pruned / pairs)
    assert pairs >= 300000 and max(worst.values()) <= 0.5, worst
    assert pruned / pairs >= 0.1


def test_a_point_as_a_query_against_the_segment_restatement():
    """a == b == c: codes 0-5 are ruled out (h0 == h1, mm == 0), 6-8 are tyr_query_segment's endpoint rule at p, 12-20 its edge
    rule with a == 0, and 9-11 add the three corners' own distances dot(V - p, V - p), which the segment block reaches only
    through its clamped edge parameters.  In binary64 these can differ in the last bit, so equality of dist2 and prim with
    segment_ref.segment(p, p) is a property of the inputs, not of the contract (include/tyr_c.h says so); on the families here
    -- 4096 points on each GPU scene, a quarter of them nearest to a vertex -- the two agree bit for bit, and that is asserted."""
    rng = np.random.default_rng(21)
    for name, (nodes, prims) in (("lattice", lattice(16, 31)[:2]), ("offset soup", offset_soup(False)), ("offset slivers", offset_soup(True))):
        p = surface_points(rng, prims, 3072, 1.0)
        corner = np.concatenate(own_triangles(prims))
        p = np.concatenate([p, (corner[rng.integers(0, len(corner), 1024)] + rng.normal(size=(1024, 3)) * 0.05).astype(F)])
        got = ref.tri_distance(p, p, p, prims)
        want = segment_ref.segment(p, p, prims)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), (name, int((bits(got[0]) != bits(want[0])).sum()), int((got[1] != want[1]).sum()))
        assert (got[2] >= 6).all()


def test_tri_distance_kernel_keeps_registers_and_lds_in_budget():
    """exactly one k_query_tri_distance; no vector spills; scratch no larger than the LdsStack's private spill arrays (52 entries of
    8 bytes, plus the frame's alignment); LDS (24,576 + 7,168 bytes) and an occupancy that admit the blocks per CU the launch
    bounds plan for (DESIGN.md "Closest-triangle queries" records the number and why)."""
    planned = launch_bounds_blocks("tri_distance", "k_query_tri_distance")
    assert 2 <= planned <= 3
    assert_kernel_budget("tri_distance", "k_query_tri_distance", 1, (64 - 12) * 8 + 16, 24576 + 7168, planned=planned)


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_tri_distance", "tyr_tri_distance_out", hip.TriDistanceOut, 6, defines=("TYR_QUERY_TRI_SKIP_SHARED",))


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, a, b, c, md=None, **kw):
    md = md if md is None or np.isscalar(md) else np.array(md)
    return tuple(x.cpu().numpy() for x in g.query_tri_distance(np.array(a), np.array(b), np.array(c), md, feature=True, region=True, points=True, **kw))


same = functools.partial(same_outputs, NAMES)


def check(g, prims, a, b, c, md=None, what="", **kw):
    got = ask(g, a, b, c, md, **kw)
    want = ref.tri_distance(a, b, c, prims, md, **kw)
    same(got, want, what)
    return got, want


def probes(rng, prims, n, size):
    return around(rng, surface_points(rng, prims, n, 0.5 * size), size)


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lattice_and_ties(hip):
    """heightfield(16): triangles a cell edge across around the surface, small and large ones, flat ones over the grid that are
    equally near to several triangles; a quarter with a bound of 2"""
    nodes, prims, (a, b, c, md), want = lattice_case()
    g = renderer(hip, nodes, prims)
    got = ask(g, a, b, c, md)
    same(got, want, "lattice")
    assert (got[2][got[1] >= 0] == 5).any() and len(np.unique(got[2])) >= 15 and len(np.unique(got[3])) == 7 and (got[1] < 0).any() and (got[0] == 0).any()
    same(ask(g, a[:1024], b[:1024], c[:1024]), ref.tri_distance(a[:1024], b[:1024], c[:1024], prims), "max_dist NULL")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_exact_ties_resolve_to_the_lower_index(hip):
    """a scene concatenated with itself: every winner is the lower of the two copies' build-order indices"""
    nodes, prims, (a, b, c), want = duplicated_case()
    twin = duplicated(32, 256)[3]
    g = renderer(hip, nodes, prims)
    got = ask(g, a, b, c)
    same(got, want, "duplicated")
    prim = got[1]
    assert (prim >= 0).all() and (prim < twin[prim]).all()
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slivers", [False, True])
def test_scale_and_slack(hip, slivers):
    """a soup moved by (4096, -4096, 8192), without and with slivers: 2048 triangles from 1e-3 across to the scene's diagonal
    (the unbounded walk, and the weak key of a query whose own box is most of the scene), some with a bound"""
    nodes, prims, (a, b, c, md), want = soup_case(slivers)
    g = renderer(hip, nodes, prims)
    got = ask(g, a, b, c, md)
    same(got, want, f"offset soup, slivers={slivers}")
    assert g.query_error() == 0
    g.close()


SHAPES = {"default": {}, "staged0": dict(staged_nodes=0), "staged7": dict(staged_nodes=7), "layout_host": dict(layout_on_device=0), "layout_device": dict(layout_on_device=1),
          "counting": dict(flags=4)}  # (TYR_FLAG_COUNT_VISITS)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scene_shapes(hip, shape):
    """no triangles, one triangle, and 40 identical ones (an over-long leaf behind synthetic records) alone and beside the Cornell
    box, on the default ctx and on each other make of scene a ctx can be given (as test_query_shapes: the staged-node counts,
    the host and the device layout pass, the counting upload)"""
    from tyrant_amd import scenes

    kw = dict(SHAPES[shape])
    flags = kw.pop("flags", 0)
    one_tri = build(scenes.make_triangles(np.array([[-30, 0, 10]], F), np.array([[30, 0, 10]], F), np.array([[0, 0, 70]], F)))
    forty = build(stack40())
    beside = build(np.concatenate([scenes.cornell_box().triangles, stack40()]))
    rng = np.random.default_rng(64)
    g = None
    for name, (nodes, prims) in (("none", no_triangles()), ("one", one_tri), ("stack40", forty), ("cornell + stack40", beside)):
        if g is None:
            g = renderer(hip, nodes, prims, flags=flags, **kw)
        else:
            g.upload(nodes, prims)
        src = prims if len(prims) else forty[1]
        a, b, c = (np.concatenate(x) for x in zip(probes(rng, src, 200, 8.0), probes(rng, src, 100, 60.0)))
        md = rng.choice(np.array([np.inf, np.inf, 5.0], F), len(a)).astype(F)
        (_, prim, _, _, _, _), _ = check(g, prims, a, b, c, md, what=f"{name}, {shape}")
        if name == "none":
            assert (prim < 0).all()
        if "stack40" in name:
            stack = np.nonzero((np.ascontiguousarray(prims).view(np.uint8).reshape(len(prims), -1) == np.ascontiguousarray(stack40()[:1]).view(np.uint8)).all(axis=1))[0]
            on_stack = np.isin(prim, stack)
            assert stack.size == 40 and on_stack.any() and (prim[on_stack] == stack.min()).all()  # the first of the identical records
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_bounds_hostile_input_and_batch_sizes(hip):
    """the Cornell box: triangles with whole-number corners, of zero area and larger than the room; max_dist of 0, tiny, larger than
    the room and +inf, per query, one number and NULL; NaN / infinite / negative input; n = 1 .. one past a feed chunk; every
    optional output NULL in turn (all combinations)"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    g = renderer(hip, nodes, prims)
    rng = np.random.default_rng(65)
    n = 4200
    lo, hi = nodes[0]["bounds"][0].astype(F), nodes[0]["bounds"][1].astype(F)
    centre = lo - 5 + (hi - lo + 10) * rng.random((n, 3))
    a, b, c = around(rng, centre, rng.choice([1.0, 20.0, 400.0], n))
    md = rng.choice(np.array([0.0, 1e-30, 1e-3, 0.5, 3.0, 500.0, np.inf, np.inf], F), n).astype(F)
    kind = rng.integers(0, 30, n)
    for x in (a, b, c):
        x[kind < 6] = np.round(x[kind < 6])  # whole numbers, some of them on the walls' planes
    b[kind == 6], c[kind == 6] = a[kind == 6], a[kind == 6]  # a point
    c[kind == 7] = b[kind == 7]  # a segment
    bad = np.array([np.nan, np.inf, -np.inf], F)
    for code, arr in ((8, a), (9, b), (10, c)):
        w = np.nonzero(kind == code)[0]
        arr[w, rng.integers(0, 3, w.size)] = bad[rng.integers(0, 3, w.size)]
    md[kind == 11] = rng.choice(np.array([np.nan, -1.0, -np.inf, -0.0], F), (kind == 11).sum())
    want = ref.tri_distance(a, b, c, prims, md)
    invalid = np.isposinf(want[0]) & ~np.isposinf(md)
    assert invalid.sum() >= n // 15 and (want[1] < 0).sum() >= n // 6 and (want[1] >= 0).sum() >= n // 3
    got = ask(g, a, b, c, md)
    same(got, want, "cornell")
    same(ask(g, a[:1000], b[:1000], c[:1000]), ref.tri_distance(a[:1000], b[:1000], c[:1000], prims), "max_dist NULL")
    same(ask(g, a[:1000], b[:1000], c[:1000], 3.0), ref.tri_distance(a[:1000], b[:1000], c[:1000], prims, F(3.0)), "one number as max_dist")
    for m in (0, 1, 63, 64, 65, 4097):  # every prefix answers as the whole batch did
        same(ask(g, a[:m], b[:m], c[:m], md[:m]), tuple(x[:m] for x in want), f"n = {m}")
    # the outputs asked for through the binding, in its order
    res = g.query_tri_distance(a[:100], b[:100], c[:100], md[:100], region=True)
    assert len(res) == 3 and np.array_equal(res[2].cpu().numpy(), want[3][:100])
    # optional outputs NULL, in every combination, through the C call; the arrays not passed stay untouched
    m = 1000
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x[:m])).cuda()  # noqa: E731
    ta, tb, tc, tm = on(a), on(b), on(c), on(md)
    P = C.c_void_p
    kinds = (((), torch.float32), ((), torch.int32), ((), torch.uint8), ((), torch.uint8), ((3,), torch.float32), ((3,), torch.float32))
    for use in itertools.product((False, True), repeat=4):
        outs = [torch.full((m, *shape), 7, dtype=dtype).cuda() for shape, dtype in kinds]
        torch.cuda.synchronize()
        used = (True, True) + use
        out = hip.TriDistanceOut(*[x.data_ptr() if u else None for x, u in zip(outs, used)])
        assert hip.lib().tyr_query_tri_distance(g.h, m, P(ta.data_ptr()), P(tb.data_ptr()), P(tc.data_ptr()), P(tm.data_ptr()), 0, C.byref(out), None) == 0
        assert g.query_error() == 0
        res = [x.cpu().numpy() for x in outs]
        same_outputs([nm for nm, u in zip(NAMES, used) if u], [x for x, u in zip(res, used) if u], [w[:m] for w, u in zip(want, used) if u], f"outputs {use}")
        assert all((x == 7).all() for x, u in zip(res, used) if not u), use
    g.close()


@pytest.mark.gpu
def test_skip_shared_on_the_meshs_own_triangles(hip):
    """the lattice's own triangles as queries with a bound of 5: without the flag every answer is dist2 0 on a neighbour or itself;
    with it the answers are the restatement's -- the nearest triangle that shares no corner, or none"""
    nodes, prims, (a, b, c), plain, skipped = self_case()
    g = renderer(hip, nodes, prims)
    got = ask(g, a, b, c, 5.0)
    same(got, plain, "own triangles")
    assert (got[0] == 0).all() and (got[1] >= 0).all()
    same(ask(g, a, b, c, 5.0, skip_shared=True), skipped, "own triangles, skip_shared")
    rng = np.random.default_rng(66)
    qa, qb, qc = probes(rng, prims, 500, 6.25)
    qa[::2] = a[rng.integers(0, len(a), 250)]  # strangers that share one corner with the mesh
    check(g, prims, qa, qb, qc, what="one shared corner", skip_shared=True)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_tri_distance_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with triangle-distance queries between its tyr_render calls: the same accumulation
    buffer and counters as without them"""
    from tyrant_amd import binding, scenes

    nodes, prims = binding.bvh_build(scenes.cornell_box().triangles)
    rng = np.random.default_rng(67)
    n = 4000
    centre = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(5, 80, n)], axis=1)
    q = around(rng, centre, 15.0)
    want = ref.tri_distance(*q, prims)

    def between(g):
        same(ask(g, *q), want, "between two renders")
        ask(g, *q, 0.5, skip_shared=True)

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the answers to the refitted scene's; a torch side stream and the ctx's stream work; bad
    arguments are refused before any launch; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(16))
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    rng = np.random.default_rng(68)
    n = 1000
    a, b, c = probes(rng, prims, n, 6.25)
    check(g, prims, a, b, c, what="before the refit")
    moved = deformed(prims, 4.0)
    g.refit(moved)
    got, want = check(g, moved, a, b, c, what="after the refit")
    assert not np.array_equal(want[1], ref.tri_distance(a, b, c, prims)[1])
    # a side stream, device tensors taken in place; then the ctx's own stream (NULL) through the C call
    ta, tb, tc = (torch.from_numpy(x).cuda() for x in (a, b, c))
    tm = torch.full((n,), 1.5).cuda()
    res, side = on_side_stream(lambda side: (g.query_tri_distance(ta, tb, tc, tm, feature=True, region=True, points=True, stream=side), side))
    near = ref.tri_distance(a, b, c, moved, np.full(n, 1.5, F))
    same(tuple(x.cpu().numpy() for x in res), near, "side stream")
    res = g.query_tri_distance(ta, tb, tc, 1.5, feature=True, region=True, points=True, stream=side)  # the number is filled on the current stream
    side.synchronize()
    same(tuple(x.cpu().numpy() for x in res), near, "one number as max_dist on a side stream")

    L, h, P = hip.lib(), g.h, C.c_void_p
    dist2, prim = torch.full((n,), 7.0).cuda(), torch.full((n,), 7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    none4 = (None,) * 4
    ok = hip.TriDistanceOut(dist2.data_ptr(), prim.data_ptr(), *none4)
    pa, pb, pc, pm = P(ta.data_ptr()), P(tb.data_ptr()), P(tc.data_ptr()), P(tm.data_ptr())
    fn = L.tyr_query_tri_distance
    assert fn(h, n, pa, pb, pc, pm, 0, C.byref(ok), None) == 0
    assert g.query_error() == 0  # (waits for the ctx's stream)
    same((dist2.cpu().numpy(), prim.cpu().numpy()), near[:2], "the ctx's stream")
    before = prim.cpu().numpy().copy()
    inv = hip.TYR_ERR_INVALID
    assert fn(None, 4, pa, pb, pc, None, 0, C.byref(ok), None) == inv
    assert fn(h, 4, None, pb, pc, None, 0, C.byref(ok), None) == inv
    assert fn(h, 4, pa, None, pc, None, 0, C.byref(ok), None) == inv
    assert fn(h, 4, pa, pb, None, None, 0, C.byref(ok), None) == inv
    assert fn(h, 4, pa, pb, pc, None, 0, None, None) == inv
    assert fn(h, 4, pa, pb, pc, None, 0, C.byref(hip.TriDistanceOut(None, prim.data_ptr(), *none4)), None) == inv
    assert fn(h, 4, pa, pb, pc, None, 0, C.byref(hip.TriDistanceOut(dist2.data_ptr(), None, *none4)), None) == inv
    for flags in (1, 2, 4, 16, 8 | 4):  # TYR_QUERY_TRI_SKIP_SHARED (8) is the only legal flag
        assert fn(h, 4, pa, pb, pc, None, flags, C.byref(ok), None) == inv
    assert fn(h, 1 << 31, pa, pb, pc, None, 0, C.byref(ok), None) == inv
    assert fn(h, 0, None, None, None, None, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert fn(empty.h, 4, pa, pb, pc, None, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_tri_distance(ta.double(), tb, tc)
    with pytest.raises(ValueError):
        g.query_tri_distance(ta, tb[:, :2].contiguous(), tc)
    with pytest.raises(ValueError):
        g.query_tri_distance(ta, tb, tc[:5])
    with pytest.raises(ValueError):
        g.query_tri_distance(ta, tb, tc, tm[:5])
    assert np.array_equal(prim.cpu().numpy(), before)  # the refused calls wrote nothing
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_c3_tree(hip):
    """one pass on C3's 1 M-triangle tree: the 256 triangles of tests/golden/tri_distance_c3.npz (around points within 1.5 of the
    surface, from a tenth of a cell to tens of cells across, every fourth with a bound) against the six answers
    tools/tri_distance_c3_golden.py recorded from the restatement's brute force.  Every run checks that the file belongs to
    these triangles and evaluates the winners' pairs from the restatement."""
    sc, nodes, prims = built_scene("mesh706")
    z = np.load(C3_ANSWERS)
    assert str(z["digest"]) == hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest(), "the recorded answers belong to other triangles"
    a, b, c, md = z["a"], z["b"], z["c"], z["max_dist"]
    want = tuple(z[k] for k in NAMES)
    arg = want[1].astype(np.int64)
    assert len(a) == 256 and (arg >= 0).sum() >= 128 and (arg < 0).sum() >= 8 and (want[0][arg >= 0] == 0).sum() >= 16
    same(ref.answers(a, b, c, ref.bound2(md, 256), ref.valid_inputs(a, b, c, md), arg, prims), want, "the recorded answers against the restatement")
    g = renderer(hip, nodes, prims)
    same(ask(g, a, b, c, md), want, "C3")
    assert g.query_error() == 0
    g.close()
