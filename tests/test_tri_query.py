"""Batched triangle-overlap queries on the uploaded scene (tyr_query_tri, hip/tri.hip; Renderer.query_tri): the member set of
include/tyr_c.h "Triangle-overlap queries" over all triangles, bit for bit against its numpy restatement (tests/tri_ref.py) by
brute force -- the definition has no traversal order in it, so nothing else is needed as an oracle.

CPU: the restatement by hand, the restatement against the same rules in exact integer arithmetic, what the fixtures are for, the
pruning argument on the fixtures' trees, what the compiler made of the kernels, the ABI.  GPU: a lattice asked about its own
triangles, the seeded pair families as one scene, duplicated triangles, an over-long leaf, offset scenes and slivers, row
lengths and the flags, batch sizes, hostile input, isolation from the render, refit, streams, argument checks, and one pass on
C3's 1 M-triangle tree."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest

import tri_ref as ref
from conftest import GOLDEN, built_scene
from query_support import (OFFSET, assert_kernel_budget, assert_query_abi, assert_render_undisturbed, box_points, build, deformed, duplicated, lattice, launch_bounds_blocks,
                           no_triangles, offset_soup, on_side_stream, renderer, stack40, surface_points, tri)
from query_support import same as same_outputs

F = np.float32
D = np.float64
C3_ANSWERS = os.path.join(GOLDEN, "tri_c3.npz")
INF = F(np.inf)
KMAX = 32


def up(x):
    return np.nextafter(F(x), INF)


def down(x):
    return np.nextafter(F(x), -INF)


# ---- fixtures (numpy only) --------------------------------------------------------------------------------------------
def scene_corners(prims):
    """the binary32 corners Q0, Q1, Q2 of every record"""
    return tuple(np.ascontiguousarray(x.astype(F)) for x in ref.corners(*ref.records(prims)))


def triangles_round(rng, centres, lo_exp, hi_exp):
    """seeded triangles round `centres`: every corner within 10^lo_exp .. 10^hi_exp (one size per triangle) of its centre"""
    size = 10.0 ** rng.uniform(lo_exp, hi_exp, (len(centres), 1))
    return tuple(np.ascontiguousarray((centres + rng.uniform(-1, 1, centres.shape) * size).astype(F)) for _ in range(3))


@functools.lru_cache(maxsize=None)
def lattice_case():
    """heightfield(32), grid step 3.125: (nodes, prims, (a, b, c), the parts' slices, (count, prim) for 32)"""
    nodes, prims, _, _ = lattice(32, 21)
    rng = np.random.default_rng(71)
    A, B, Cc = scene_corners(prims)
    parts, cols = {}, ([], [], [])

    def add(name, a, b, c):
        at = sum(len(x) for x in cols[0])
        parts[name] = slice(at, at + len(a))
        for col, x in zip(cols, (a, b, c)):
            col.append(np.asarray(x, F).reshape(-1, 3))

    add("own", A, B, Cc)  # every triangle finds itself and the triangles that share a corner with it
    w = rng.permutation(len(prims))[:256]
    lifted = [x[w].copy() for x in (A, B, Cc)]
    for x in lifted:
        x[:, 2] = up(x[:, 2])  # one binary32 step above the surface: whatever still touches, touches by rounding
    add("lifted", *lifted)
    w = rng.permutation(len(prims))[:256]
    add("tilted", A[w] + np.array([0, 0, 2.5], F), B[w] - np.array([0, 0, 2.5], F), Cc[w])  # through the surface
    add("seeded", *triangles_round(rng, surface_points(rng, prims, 448, 0.5), -6.0, 0.8))  # from a step across to larger than a cell
    # 48 triangles of circumradius 20 .. 40, nearly level at the field's mean height: each cuts the surface along many cells
    centre, radius, turn = rng.uniform(-30, 30, (48, 2)), rng.uniform(20, 40, 48), rng.uniform(0, 2 * np.pi, 48)
    add("large", *(np.stack([centre[:, 0] + radius * np.cos(turn + k * 2.1), centre[:, 1] + radius * np.sin(turn + k * 2.1), 22 + rng.uniform(-2, 2, 48)], axis=1) for k in range(3)))
    add("everything", [[-60, -60, 0]], [[60, -60, 0]], [[0, 200, 50]])  # its bounding box holds the whole field
    a, b, c = (np.ascontiguousarray(np.concatenate(col)) for col in cols)
    return nodes, prims, (a, b, c), parts, ref.tri(a, b, c, prims, KMAX)


@functools.lru_cache(maxsize=None)
def pair_families():
    """seeded (query, scene triangle) pairs: name -> (a, b, c, vert, e1, e2)"""
    rng = np.random.default_rng(72)

    def soup(n, off=0.0):
        vert = (rng.uniform(-4, 4, (n, 3)) + off).astype(F)
        return vert, rng.uniform(-1, 1, (n, 3)).astype(F), rng.uniform(-1, 1, (n, 3)).astype(F)

    def near(vert, e1, e2, spread=0.5, lo_exp=-1.0, hi_exp=0.2):
        """query triangles round a point of their scene triangle plus noise, sized relative to it"""
        n = len(vert)
        u = rng.random((n, 1))
        v = rng.random((n, 1)) * (1 - u)
        scale = np.maximum(np.abs(e1).max(1, keepdims=True), np.abs(e2).max(1, keepdims=True)).astype(D)
        centre = vert.astype(D) + u * e1 + v * e2 + rng.normal(size=(n, 3)) * spread * scale
        size = 10.0 ** rng.uniform(lo_exp, hi_exp, (n, 1)) * scale
        return tuple((centre + rng.uniform(-1, 1, (n, 3)) * size).astype(F) for _ in range(3))

    fam = {}
    t = soup(9000)
    fam["unit"] = near(*t) + t
    t = soup(5000, OFFSET.astype(D))
    fam["offset"] = near(*t) + t
    _, prims = offset_soup(True)
    w = np.concatenate([np.arange(0, 2000, 10), rng.integers(0, 2000, 1800)])  # every sliver, and seeded others
    t = tuple(x[w] for x in ref.records(prims))
    fam["slivers"] = near(*t, spread=0.3) + t
    # one and two corners of the query are corners of the scene triangle, bit for bit
    for name, n, k in (("shared_corner", 2000, 1), ("shared_edge", 2000, 2)):
        t = soup(n)
        P = np.stack(near(*t), axis=1)  # (n, 3 corners, 3)
        Q = np.stack([x.astype(F) for x in ref.corners(*t)], axis=1)
        pi, qi = np.argsort(rng.random((n, 3)), axis=1), np.argsort(rng.random((n, 3)), axis=1)
        rows = np.arange(n)
        for j in range(k):
            P[rows, pi[:, j]] = Q[rows, qi[:, j]]
        fam[name] = (P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy()) + t
    # exactly coplanar: all six corners o + i u + j v with u, v and o multiples of 1/64 and i, j multiples of 1/16 -- exact in
    # binary32, and so are vert + e1 and vert + e2
    n = 4000
    o, u, v = (rng.integers(-64, 65, (n, 1, 3)) / 64.0 for _ in range(3))
    ij = rng.integers(-24, 25, (n, 6, 2)) / 16.0
    ij[:, 3:] = ij[:, 3:] * 0.5 + rng.integers(-1, 2, (n, 1, 2))  # the query: smaller, next to the scene triangle or on it
    pts = o + ij[:, :, :1] * u + ij[:, :, 1:] * v
    assert np.array_equal(pts.astype(F).astype(D), pts)
    pts = pts.astype(F)
    fam["coplanar"] = (pts[:, 3], pts[:, 4], pts[:, 5], pts[:, 0], pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0])
    # a corner of the query exactly in the scene triangle's face: Q0 + s f + t g with dyadic s, t, s + t <= 1, on corners that
    # are multiples of 1/64
    n = 2000
    Q = rng.integers(-256, 257, (n, 3, 3)) / 64.0
    s = rng.integers(0, 9, (n, 1)) / 8.0
    tt = np.floor(rng.random((n, 1)) * (9 - s * 8)) / 8.0
    inface = Q[:, 0] + s * (Q[:, 1] - Q[:, 0]) + tt * (Q[:, 2] - Q[:, 0])
    assert np.array_equal(inface.astype(F).astype(D), inface) and (s + tt <= 1).all()
    Q = Q.astype(F)
    t = (Q[:, 0], Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0])
    P = np.stack(near(*t, spread=1.0), axis=1)
    P[np.arange(n), rng.integers(0, 3, n)] = inface.astype(F)
    fam["corner_in_face"] = (P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy()) + t
    return fam


def tree_facts(nodes, prims):
    """of a depth-first node array (left child i + 1, right child `offset`; a leaf holds offset .. offset + primitiveCount - 1):
    (every child's box lies in its parent's, every corner Q0, Q1, Q2 of a leaf's triangles lies in the leaf's box)"""
    Q0, Q1, Q2 = scene_corners(prims)
    cmin, cmax = np.minimum(np.minimum(Q0, Q1), Q2), np.maximum(np.maximum(Q0, Q1), Q2)
    lo, hi = nodes["bounds"][:, 0], nodes["bounds"][:, 1]
    leaf = nodes["primitiveCount"] > 0
    inner = np.nonzero(~leaf)[0]
    nested = True
    for child in (inner + 1, nodes["offset"][inner]):
        nested = nested and bool((lo[child] >= lo[inner]).all() and (hi[child] <= hi[inner]).all())
    holds = True
    for n in np.nonzero(leaf)[0]:
        s = slice(int(nodes["offset"][n]), int(nodes["offset"][n]) + int(nodes["primitiveCount"][n]))
        holds = holds and bool((cmin[s] >= lo[n]).all() and (cmax[s] <= hi[n]).all())
    return nested, holds


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0))    # the unit right triangle in z = 0: Q0, Q1 = (1, 0, 0), Q2 = (0, 1, 0)
TILTED = ((0, 0, 0), (1, 0, 1), (0, 1, 1))  # in the plane z = x + y: Q1 = (1, 0, 1), Q2 = (0, 1, 1)
# scene triangle, the query's corners, the first separating axis (0: a member), whether that axis is the only one that separates
HAND = [
    (UNIT, ((2, 0, -1), (3, 0, 1), (2, 1, 0)), 1, False),  # the coordinate axes x, y, z
    (UNIT, ((0, 2, -1), (1, 3, 1), (0, 2, 1)), 2, False),
    (UNIT, ((0, 0, 1), (1, 0, 2), (0, 1, 1)), 3, False),
    # one axis of rule 2 alone separates: the scene triangle's normal, the query's, each of the nine edge crosses
    (TILTED, ((0.5, 0.5, 0.75), (1.75, -0.5, 0.25), (1.5, 1.75, -0.25)), 4, True),
    (TILTED, ((-1, 0.25, 1.25), (1, -0.5, -0.5), (-0.25, 0.25, -0.75)), 5, True),
    (TILTED, ((-0.25, 0.75, 0.25), (0.75, -0.75, 0), (1, 1.25, 0)), 6, True),
    (TILTED, ((1, 1, 1.5), (0.5, -0.25, 0.75), (-0.5, 0.75, 1.25)), 7, True),
    (TILTED, ((-1, 0.25, 0.5), (1, 0.75, 0.25), (-0.5, 0.75, 0.25)), 8, True),
    (TILTED, ((1.5, 2, 1.25), (1.25, 1.5, 1.5), (0.5, -0.75, 0.25)), 9, True),
    (TILTED, ((0.25, 1.25, -0.75), (-0.25, 0.75, 0.25), (1, 0.25, 1.25)), 10, True),
    (TILTED, ((0.25, 2, 0.75), (0.75, 1, 0.25), (-0.25, 0.5, 0.25)), 11, True),
    (TILTED, ((-1, -0.5, 1.75), (0.75, -0.25, 0.5), (2, 0.25, -1)), 12, True),
    (TILTED, ((1, -0.75, -0.25), (0, 1.25, 0.25), (0, 1.75, 2)), 13, True),
    (TILTED, ((0, 2, 0.25), (-1, 0.75, -0.5), (-0.5, -0.5, 0.5)), 14, True),
    # coplanar and disjoint: the normals and every edge cross are parallel to z and separate nothing -- only an in-plane axis
    # does, an edge normal of the query (15-17) or of the scene triangle (19: the hypotenuse's)
    (UNIT, ((1.75, 1.5, 0), (1, -0.75, 0), (2, 1, 0)), 15, True),
    (UNIT, ((1.75, 0.5, 0), (0.25, 2, 0), (1.75, -1, 0)), 16, True),
    (UNIT, ((0.5, 0.75, 0), (1.5, 0.25, 0), (1.75, -0.75, 0)), 17, True),
    (UNIT, ((0.75, 0.75, 0), (1, 0.75, 0), (1, 1, 0)), 19, True),
    # touching, and the same one binary32 step apart
    (UNIT, ((1, 0, 0), (2, -1, 1), (2, 1, -1)), 0, False),  # corner on corner: P0 = Q1
    (UNIT, ((up(1), 0, 0), (2, -1, 1), (2, 1, -1)), 1, False),
    (TILTED, ((1, 0, 1), (0.5, -1, 1), (1.5, -1, 1)), 0, False),  # corner on corner where the boxes overlap: P0 = Q1
    (TILTED, ((1, down(0), 1), (0.5, -1, 1), (1.5, -1, 1)), 2, False),
    (UNIT, ((0.5, 0.5, 0), (1, 1, 1), (1, 1, -1)), 0, False),  # corner on edge: P0 on the hypotenuse, the query in the plane x = y
    (UNIT, ((up(0.5), up(0.5), 0), (1, 1, 1), (1, 1, -1)), 7, False),  # cross(P1 - P0, the hypotenuse) comes first of seven
    (TILTED, ((0.25, 0.25, 0.5), (0, 0.5, 2), (0.5, 0, 2)), 0, False),  # corner in face: P0 in the face's interior, the rest above
    (TILTED, ((0.25, 0.25, up(0.5)), (0, 0.5, 2), (0.5, 0, 2)), 4, False),
    (UNIT, ((0.5, -1, -1), (0.5, 1, 1), (0.5, -1, 1)), 0, False),  # edges crossing at a point: P0 P1 through (0.5, 0, 0) on Q0 Q1
    (UNIT, ((0.5, -1, -1), (0.5, 1, up(1)), (0.5, -1, 1)), 6, False),
    (UNIT, ((0.25, 0.25, 0), (2, 0.25, 0), (0.25, 2, 0)), 0, False),  # coplanar overlap
    (UNIT, ((1, 0, 0), (2, 0, 0), (1, 1, 0)), 0, False),  # coplanar, touching at Q1; a step apart
    (UNIT, ((up(1), 0, 0), (2, 0, 0), (up(1), 1, 0)), 1, False),
    (UNIT, ((0.5, 0.5, 0), (1, 0.5, 0), (1, 1, 0)), 0, False),  # coplanar, a corner on the hypotenuse; a step apart
    (UNIT, ((up(0.5), 0.5, 0), (1, 0.5, 0), (1, 1, 0)), 19, False),
    (UNIT, ((0.125, 0.125, 0), (0.25, 0.125, 0), (0.125, 0.25, 0)), 0, False),  # a small triangle inside a large coplanar one
    (((0.125, 0.125, 0), (0.125, 0, 0), (0, 0.125, 0)), ((0, 0, 0), (1, 0, 0), (0, 1, 0)), 0, False),  # and a large one round a small one
    (UNIT, ((0.25, 0.125, -1), (0.25, 0.125, 1), (0.125, 0.25, 5)), 0, False),  # pierced by an edge of the query, no corner inside
    (UNIT, ((0.25, -5, -5), (0.25, 5, -5), (0.25, 0, 5)), 0, False),  # the scene triangle's edges pierce the query: none of the query's reaches it
    # zero area, the contract's conservative clause: the segment (1.5, 0.25) -> (0.75, -0.5) passes the corner Q1 outside the
    # triangle, but its normal is 0 and no edge line of the scene triangle has it on one side
    (UNIT, ((1.5, 0.25, 0), (0.75, -0.5, 0), (1.125, -0.125, 0)), 0, False),
    (UNIT, ((1.5, 0.25, 0), (0.75, -0.5, 0), (1.5, -0.5, 0)), 15, True),  # the same edge in a triangle with area: its normal separates
]


def test_hand_cases():
    """exactly representable numbers on the unit right triangle and a tilted one: an axis of each class that separates, of rule 2
    alone; corner on corner, corner on edge, corner in face, edges crossing at a point, coplanar pairs, and the same one binary32
    step apart; a triangle inside a coplanar one; a triangle pierced with no corner inside the other; rule 0 with +0 against
    -0; a segment that pins the conservative answer; every invalid input.  The exact test agrees on each."""
    for (vert, e1, e2), (a, b, c), axis, alone in HAND:
        args = [np.array(x, F) for x in (a, b, c, vert, e1, e2)]
        got = int(ref.pair(*args))
        assert got == axis, (vert, e1, e2, a, b, c, got)
        assert ref.pair_exact(a, b, c, vert, e1, e2) == axis, (a, b, c)
        if alone:
            assert np.nonzero(ref.separating(*args)[0])[0].tolist() == [axis - 1]
        cnt, prim = ref.tri(*([x] for x in args[:3]), tri(vert, e1, e2), 2)
        assert (cnt.tolist(), prim.tolist()) == ([int(axis == 0)], [[0 if axis == 0 else -1, -1]])
    # the eleven classic axes call the coplanar disjoint pairs members: the in-plane axes are required
    for (vert, e1, e2), (a, b, c), axis, alone in HAND:
        if axis >= 15:
            assert not ref.separating(*(np.array(x, F) for x in (a, b, c, vert, e1, e2)))[0][:14].any()
    # rule 0: -0 equals +0; without the flag the pair touches at that corner
    a, b, c = np.array([[-0.0, 0, -0.0]], F), np.array([[-1, 0, 1]], F), np.array([[-1, -1, -1]], F)
    assert int(ref.pair(a, b, c, *(np.array(x, F) for x in UNIT))[0]) == 0 and ref.pair_exact(a[0], b[0], c[0], *UNIT) == 0
    assert int(ref.pair(a, b, c, *(np.array(x, F) for x in UNIT), skip_shared=True)[0]) == ref.SHARED == ref.pair_exact(a[0], b[0], c[0], *UNIT, skip_shared=True)
    assert ref.tri(a, b, c, tri(*UNIT), 1)[0].tolist() == [1] and ref.tri(a, b, c, tri(*UNIT), 1, skip_shared=True)[0].tolist() == [0]
    # the set, its count beyond the row, the row ascending, ANY, skip_shared; every invalid input
    four = np.concatenate([tri((0, 0, 5), (1, 0, 0), (0, 1, 0)), tri(*UNIT), tri(*TILTED), tri(*UNIT)])
    nan, inf = np.nan, np.inf
    a, b, c = (np.array([p] * 11, F) for p in ((0.25, 0.25, -1), (0.5, 0.25, 1), (0.25, 0.5, 1)))
    for i, (arr, comp, bad) in enumerate(((a, 0, nan), (a, 2, inf), (a, 1, -inf), (b, 0, nan), (b, 1, inf), (b, 2, -inf), (c, 2, nan), (c, 0, inf), (c, 1, -inf)), start=1):
        arr[i, comp] = bad
    a[10], b[10], c[10] = (0.25, 0.25, 3), (0.5, 0.25, 4), (0.25, 0.5, 4)
    cnt, prim = ref.tri(a, b, c, four, 2)
    assert cnt.tolist() == [3] + [0] * 10 and prim.tolist() == [[1, 2]] + [[-1, -1]] * 10
    assert ref.tri(a, b, c, four, 0)[0].tolist() == cnt.tolist() and ref.tri(a, b, c, four, 0)[1].shape == (11, 0)
    assert ref.tri(a, b, c, four, 32)[1][0].tolist() == [1, 2, 3] + [-1] * 29
    assert ref.tri(a, b, c, four, any=True).tolist() == [True] + [False] * 10
    c[0] = (0, 1, 1)  # Q2 of the tilted triangle: with skip_shared it is no member, the two others stay
    assert ref.tri(a, b, c, four, 4)[1][0].tolist() == [1, 2, 3, -1] and ref.tri(a, b, c, four, 4, skip_shared=True)[1][0].tolist() == [1, 3, -1, -1]
    assert ref.tri(a[:1], b[:1], c[:1], four[:0], 2)[0].tolist() == [0]  # no triangles: nothing


def moved(p, comp, direction):
    q = np.array(p, F)
    q[comp] = np.nextafter(q[comp], INF if direction > 0 else -INF)
    return q


def test_restatement_against_exact_arithmetic():
    """the binary64 rules against the same rules in exact integer arithmetic on the same binary32 inputs, 24,000 seeded pairs:
    unit scale, moved by OFFSET, slivers, a shared corner, a shared edge, exactly coplanar, a corner exactly in the other's face.
    A pair may disagree only if its exact answer flips when one component of one of the query's corners moves by one binary32
    step; the count is printed, and the seeded families have none.  Every pair that shares a corner or an edge is a member
    without rule 0 and none is with it."""
    total, wrong = 0, {}
    for name, f in pair_families().items():
        got = ref.pair(*f)
        exact = np.array([ref.pair_exact(*(x[i] for x in f)) for i in range(len(got))])
        agree = (got == 0) == (exact == 0)
        for i in np.nonzero(~agree)[0]:  # allowed only next to a flip
            P, T = [x[i] for x in f[:3]], [x[i] for x in f[3:]]
            flips = False
            for corner in range(3):
                for comp in range(3):
                    for direction in (-1, 1):
                        Pm = list(P)
                        Pm[corner] = moved(P[corner], comp, direction)
                        flips = flips or (ref.pair_exact(*Pm, *T) == 0) != (exact[i] == 0)
            assert flips, (name, int(i), int(got[i]), int(exact[i]))
        wrong[name] = int((~agree).sum())
        assert np.array_equal(got[agree], exact[agree]), name  # and the same first axis
        if name.startswith("shared"):
            assert (got == 0).all() and (exact == 0).all(), name
            assert (ref.pair(*f, skip_shared=True) == ref.SHARED).all() and ref.pair_exact(*(x[0] for x in f), skip_shared=True) == ref.SHARED
        total += len(got)
    print("pairs:", total, "disagreements with the exact answer per family:", wrong)
    assert total >= 20000 and not any(wrong.values()), wrong


def test_pruning_argument_holds_on_the_fixtures_trees():
    """every triangle's corners Q0, Q1, Q2 lie in its leaf's box and every box in its parent's, so in every ancestor's: a node
    whose box misses the query's bounding box on an axis holds only triangles that rule 1 separates on that axis"""
    from tyrant_amd import scenes

    trees = [lattice(32, 21)[:2], duplicated(22, 2048)[:2], build(stack40()), offset_soup(False), offset_soup(True), build(scenes.heightfield(16)), build(scenes.cornell_box().triangles),
             build(np.concatenate([scenes.cornell_box().triangles, stack40()]))]
    for nodes, prims in trees:
        assert tree_facts(nodes, prims) == (True, True)


def test_fixtures_reach_what_they_are_for():
    """each of the 20 axes is the first separator of at least 10 seeded pairs and none of at least 200; the lattice's queries
    have empty answers, rows of 5 partly filled (1 to 4 members), rows of 5 full (5 to 32) and rows of 32 overflowing, at least
    20 each; an
    interior triangle of the lattice touches itself and the 12 that share a corner with it, none with skip_shared; the
    lattice's tree needs more stack than the 12 LDS entries; stack40 has an over-long leaf"""
    from tyrant_amd import binding

    first = np.concatenate([ref.pair(*f) for f in pair_families().values()])
    hist = np.bincount(first, minlength=21)
    print("first separating axis, 0 = member:", hist.tolist())
    assert len(hist) == 21 and hist[0] >= 200 and (hist[1:] >= 10).all(), hist.tolist()
    nodes, prims, (a, b, c), parts, (cnt, prim) = lattice_case()
    print("members per query:", np.bincount(np.minimum(cnt, 40)).tolist())
    assert (cnt == 0).sum() >= 20 and ((cnt > 0) & (cnt < 5)).sum() >= 20 and ((cnt >= 5) & (cnt <= KMAX)).sum() >= 20 and (cnt > KMAX).sum() >= 20
    own = cnt[parts["own"]]
    Q0, Q1, Q2 = scene_corners(prims)
    interior = (np.abs(np.concatenate([Q0[:, :2], Q1[:, :2], Q2[:, :2]], axis=1)) < 50).all(axis=1)
    assert interior.sum() == 2 * 30 * 30 and (own[interior] == 13).all() and (own[~interior] < 13).all() and (own >= 4).all()
    assert not ref.tri(Q0, Q1, Q2, prims, skip_shared=True)[0].any()
    assert (np.diff(prim[parts["own"]][interior][:, :13], axis=1) > 0).all()
    assert cnt[parts["everything"]][0] > KMAX
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    nodes, prims = build(stack40())
    assert nodes["primitiveCount"].max() == 40  # an over-long leaf: synthetic records


def test_tri_kernels_keep_registers_and_lds_in_budget():
    """exactly two k_query_tri kernels (with and without ANY); no vector spills; scratch no larger than the LdsStack's private
    spill array (52 entries of 4 bytes, plus the frame's alignment); LDS as the box kernels' (12,288 + 7,168 bytes), which admits
    the blocks per CU the launch bounds plan for.  The registers and the occupancy reached are printed (DESIGN.md
    "Triangle-overlap queries" records them), not prescribed."""
    assert_kernel_budget("tri", "k_query_tri", 2, (64 - 12) * 4 + 16, 12288 + 7168, planned=launch_bounds_blocks("tri", "k_query_tri"))


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_tri", "tyr_tri_out", hip.TriOut, 2, (r"TYR_QUERY_TRI_ANY\s+4u\b", r"TYR_QUERY_TRI_SKIP_SHARED\s+8u\b", r"TYR_QUERY_TRI_MAX\s+32\b"))
    assert (hip.TYR_QUERY_TRI_ANY, hip.TYR_QUERY_TRI_SKIP_SHARED, hip.TYR_QUERY_TRI_MAX) == (4, 8, KMAX)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, q, k=0, **kw):
    """(count, prim) as numpy arrays for the queries q = (a, b, c); prim of shape (n, 0) for a count alone"""
    res = g.query_tri(*(np.array(x) for x in q), max_prims=k, **kw)
    cnt, prim = res if k else (res, None)
    cnt = cnt.cpu().numpy()
    return cnt, (prim.cpu().numpy() if k else np.zeros((len(cnt), 0), np.int32))


def hit(g, q, **kw):
    return g.query_tri(*q, any=True, **kw).cpu().numpy()


same = functools.partial(same_outputs, ("count", "prim"))


def check(g, prims, q, k, what="", **kw):
    got = ask(g, q, k, **kw)
    same(got, ref.tri(*q, prims, k, **kw), what)
    return got


def prefix(want, k, rows=slice(None)):
    """the answer for a row of k from the answer for a longer one"""
    return want[0][rows], np.ascontiguousarray(want[1][rows, :k])


def rows_of(q, rows):
    return tuple(np.ascontiguousarray(x[rows]) for x in q)


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lattice_and_its_own_triangles(hip):
    """heightfield(32) asked about its own triangles (each finds itself and every triangle that shares a corner, 13 in the
    interior, ascending; none with skip_shared), about them lifted by one binary32 step and tilted through the surface, about
    448 seeded triangles from a step across to larger than a cell, and about one triangle whose box holds everything (more stack
    than the LDS part holds)"""
    nodes, prims, q, parts, want = lattice_case()
    g = renderer(hip, nodes, prims)
    got = ask(g, q, KMAX)
    same(got, want, "lattice")
    own = got[0][parts["own"]]
    assert (own == 13).sum() == 1800 and own.max() == 13
    assert (np.diff(got[1][parts["own"]][own == 13][:, :13], axis=1) > 0).all()
    same(ask(g, q, 0), prefix(want, 0), "a count alone")
    assert np.array_equal(hit(g, q), want[0] > 0)
    skipped = check(g, prims, q, KMAX, "skip_shared", skip_shared=True)
    assert not skipped[0][parts["own"]].any() and (skipped[1][parts["own"]] == -1).all() and skipped[0][parts["tilted"]].any()
    assert np.array_equal(hit(g, q, skip_shared=True), skipped[0] > 0)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_pair_families_as_a_scene(hip):
    """the first 300 pairs of every seeded family, their scene triangles uploaded as one scene and their queries asked against
    all of it: the pairs that share a corner or an edge, the exactly coplanar ones and the corners exactly in a face reach the
    device's seventeen axes too.  At least 50 of the coplanar pairs are separated by an in-plane axis alone of rule 2: a kernel
    without those six axes counts them."""
    from tyrant_amd import scenes

    take = {name: tuple(x[:300] for x in f) for name, f in pair_families().items()}
    tris = np.zeros(300 * len(take), dtype=scenes.TRIANGLE_DTYPE)
    for key, col in (("vert", 3), ("e1", 4), ("e2", 5)):
        tris[key] = np.concatenate([f[col] for f in take.values()])
    q = tuple(np.ascontiguousarray(np.concatenate([f[col] for f in take.values()])) for col in range(3))
    sep, _ = ref.separating(*take["coplanar"])
    assert (sep[14:].any(axis=0) & ~sep[:14].any(axis=0)).sum() >= 50
    nodes, prims = build(tris)
    g = renderer(hip, nodes, prims)
    cnt, _ = check(g, prims, q, KMAX, "the families")
    assert (cnt[900:1500] >= 1).all()  # the shared corners and edges
    skipped, _ = check(g, prims, q, KMAX, "the families, skip_shared", skip_shared=True)
    assert (skipped[900:1500] < cnt[900:1500]).all()
    assert np.array_equal(hit(g, q), cnt > 0) and np.array_equal(hit(g, q, skip_shared=True), skipped > 0)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_duplicated_triangles_and_the_over_long_leaf(hip):
    """a scene concatenated with itself: both copies of every member are listed, the lower index first, and a scene triangle as
    the query skips both of its copies with skip_shared; 40 identical triangles (an over-long leaf behind synthetic records),
    alone and next to the Cornell box, with rows of 1, 5 and 32"""
    from tyrant_amd import scenes

    nodes, prims, _, twin = duplicated(22, 2048)
    rng = np.random.default_rng(73)
    Q = scene_corners(prims)
    w = rng.permutation(len(prims))[:320]
    seeded = triangles_round(rng, surface_points(rng, prims, 320, 1.0), -1.0, 0.8)
    q = tuple(np.ascontiguousarray(np.concatenate([x[w], y])) for x, y in zip(Q, seeded))
    g = renderer(hip, nodes, prims)
    cnt, prim = check(g, prims, q, KMAX, "duplicated")
    whole = (cnt > 0) & (cnt <= KMAX)
    assert whole.sum() >= 200 and (cnt[whole] % 2 == 0).all()
    for row, n in zip(prim[whole], cnt[whole]):
        assert set(twin[row[:n]].tolist()) == set(row[:n].tolist())
    for i, row in zip(w, prim[:320]):  # a scene triangle finds itself and its twin
        assert i in row and twin[i] in row
    cnt, prim = check(g, prims, q, KMAX, "duplicated, skip_shared", skip_shared=True)
    assert not cnt[:320].any() and cnt[320:].any()
    for tris in (stack40(), np.concatenate([scenes.cornell_box().triangles, stack40()])):
        nodes, prims = build(tris)
        g.upload(nodes, prims)
        q = triangles_round(rng, np.concatenate([surface_points(rng, prims, 600, 3.0), box_points(rng, prims, 200)]), -1.0, 1.3)
        want = ref.tri(*q, prims, KMAX)
        assert (want[0] >= 40).sum() >= 50
        for k in (1, 5, KMAX):
            same(ask(g, q, k), prefix(want, k), f"stack40, a row of {k}")
        assert np.array_equal(hit(g, q), want[0] > 0)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slivers", [False, True])
def test_offset_scenes(hip, slivers):
    """a soup moved by (4096, -4096, 8192), without and with slivers: triangles round points of the surface from a binary32 step
    across to larger than a scene triangle, some with a corner of a scene triangle as their own, and triangles anywhere in the
    root box"""
    nodes, prims = offset_soup(slivers)
    rng = np.random.default_rng(74)
    small = triangles_round(rng, np.concatenate([surface_points(rng, prims, 640, 0.05), box_points(rng, prims, 256)]), -3.5, 1.4)
    large = triangles_round(rng, surface_points(rng, prims, 128, 0.05), 0.8, 1.4)  # several scene triangles across: more than two members
    a, b, c = (np.ascontiguousarray(np.concatenate(x)) for x in zip(small, large))
    Q = scene_corners(prims)
    w = rng.integers(0, len(prims), 128)
    a[:128], b[128:256] = Q[1][w], Q[2][w]  # a corner of a scene triangle, bit for bit
    q = (a, b, c)
    g = renderer(hip, nodes, prims)
    cnt, _ = check(g, prims, q, 2, f"offset soup, slivers={slivers}")
    assert (cnt == 0).sum() >= 50 and (cnt > 0).sum() >= 300 and (cnt > 2).sum() >= 20
    skipped, _ = check(g, prims, q, 2, f"offset soup, slivers={slivers}, skip_shared", skip_shared=True)
    assert (skipped[:256] < cnt[:256]).all() and np.array_equal(skipped[256:], cnt[256:])
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_shapes_flags_hostile_input_and_batch_sizes(hip):
    """the lattice: rows of 0, 1, 5 and 32 are prefixes of each other; ANY equals count > 0; n = 1 .. 4097; the same queries
    shuffled answer the same; queries with a NaN or infinite component among good ones touch nothing and disturb nothing; a
    scene without triangles"""
    nodes, prims, q, parts, want32 = lattice_case()
    rng = np.random.default_rng(75)
    pick = rng.integers(0, len(q[0]), 4097)
    q = rows_of(q, pick)
    kind = rng.integers(0, 24, 4097)
    bad = np.array([np.nan, np.inf, -np.inf], F)
    for code, arr in enumerate(q):
        w = np.nonzero(kind == code)[0]
        arr[w, rng.integers(0, 3, w.size)] = bad[rng.integers(0, 3, w.size)]
    want = ref.tri(*q, prims, KMAX)
    invalid = ~ref.valid_queries(*q)
    assert invalid.sum() >= 300 and not want[0][invalid].any() and (want[1][invalid] == -1).all()
    ok = ~invalid
    assert np.array_equal(want[0][ok], want32[0][pick][ok]) and np.array_equal(want[1][ok], want32[1][pick][ok])
    g = renderer(hip, nodes, prims)
    for k in (0, 1, 5, KMAX):
        same(ask(g, q, k), prefix(want, k), f"a row of {k}")
    assert np.array_equal(hit(g, q), want[0] > 0)
    for m in (1, 63, 64, 65, 257):  # every prefix answers as the whole batch did
        same(ask(g, rows_of(q, slice(0, m)), 5), prefix(want, 5, slice(0, m)), f"n = {m}")
        assert np.array_equal(hit(g, rows_of(q, slice(0, m))), want[0][:m] > 0)
    order = rng.permutation(4097)
    same(ask(g, rows_of(q, order), 5), prefix(want, 5, order), "shuffled")
    with pytest.raises(ValueError):
        g.query_tri(*q, max_prims=KMAX + 1)
    with pytest.raises(ValueError):
        g.query_tri(*q, max_prims=1, any=True)
    g.upload(*no_triangles())
    same(ask(g, q, 5), ref.tri(*q, prims[:0], 5), "empty scene")
    assert not hit(g, q).any() and not hit(g, q, skip_shared=True).any()
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_tri_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with triangle queries between its tyr_render calls: the same accumulation buffer and
    counters as without them"""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    rng = np.random.default_rng(76)
    q = triangles_round(rng, box_points(rng, prims, 20000), -1.0, 1.3)
    want = ref.tri(*q, prims, 4)

    def between(g):
        same(ask(g, q, 4), want, "between two renders")
        g.query_tri(*q, any=True, skip_shared=True)

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the answers to the refitted scene's; a torch side stream and the ctx's stream work; bad
    arguments are refused before any launch and write nothing; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(16))
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    rng = np.random.default_rng(77)
    n = 1000
    q = triangles_round(rng, surface_points(rng, prims, n, 2.0), -0.5, 0.8)
    check(g, prims, q, 8, "before the refit")
    moved_prims = deformed(prims, 4.0)
    g.refit(moved_prims)
    check(g, moved_prims, q, 8, "after the refit")
    want = ref.tri(*q, moved_prims, 8)
    assert not np.array_equal(want[0], ref.tri(*q, prims, 8)[0])
    # a side stream, device tensors taken in place; then the ctx's own stream (NULL) through the C call
    ta, tb, tc = (torch.from_numpy(x).cuda() for x in q)
    (cnt, prim), anyhit = on_side_stream(lambda side: (g.query_tri(ta, tb, tc, max_prims=8, stream=side), g.query_tri(ta, tb, tc, any=True, stream=side)))
    same((cnt.cpu().numpy(), prim.cpu().numpy()), want, "side stream")
    assert np.array_equal(anyhit.cpu().numpy(), want[0] > 0)

    L, h, P = hip.lib(), g.h, C.c_void_p
    cnt, prim = torch.full((n,), 7, dtype=torch.int32).cuda(), torch.full((n, 8), 7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    ok = hip.TriOut(cnt.data_ptr(), prim.data_ptr())
    counts = hip.TriOut(cnt.data_ptr(), None)
    pa, pb, pc = P(ta.data_ptr()), P(tb.data_ptr()), P(tc.data_ptr())
    ANY, SKIP = hip.TYR_QUERY_TRI_ANY, hip.TYR_QUERY_TRI_SKIP_SHARED
    assert L.tyr_query_tri(h, n, pa, pb, pc, 8, 0, C.byref(ok), None) == 0
    assert g.query_error() == 0  # (waits for the ctx's stream)
    same((cnt.cpu().numpy(), prim.cpu().numpy()), want, "the ctx's stream")
    assert L.tyr_query_tri(h, n, pa, pb, pc, 0, ANY | SKIP, C.byref(counts), None) == 0  # out->prim is ignored with max_prims == 0
    assert g.query_error() == 0
    assert np.array_equal(cnt.cpu().numpy(), ref.tri(*q, moved_prims, any=True, skip_shared=True).astype(np.int32)) and np.array_equal(prim.cpu().numpy(), want[1])
    before = cnt.cpu().numpy().copy()
    inv = hip.TYR_ERR_INVALID
    assert L.tyr_query_tri(None, 4, pa, pb, pc, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_tri(h, 4, None, pb, pc, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_tri(h, 4, pa, None, pc, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_tri(h, 4, pa, pb, None, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_tri(h, 4, pa, pb, pc, 8, 0, None, None) == inv
    assert L.tyr_query_tri(h, 4, pa, pb, pc, 8, 0, C.byref(hip.TriOut(None, prim.data_ptr())), None) == inv
    assert L.tyr_query_tri(h, 4, pa, pb, pc, 8, 0, C.byref(counts), None) == inv  # out->prim NULL with max_prims > 0
    assert L.tyr_query_tri(h, 1 << 31, pa, pb, pc, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_tri(h, 4, pa, pb, pc, KMAX + 1, 0, C.byref(ok), None) == inv
    for flags in (1, 2, 16, ANY | 1, SKIP | 2, 1 << 31):  # TYR_QUERY_SPHERES and TYR_QUERY_TWO_SIDED included
        assert L.tyr_query_tri(h, 4, pa, pb, pc, 0, flags, C.byref(ok), None) == inv
    assert L.tyr_query_tri(h, 4, pa, pb, pc, 1, ANY, C.byref(ok), None) == inv  # ANY answers without indices
    assert L.tyr_query_tri(h, 4, pa, pb, pc, 1, ANY | SKIP, C.byref(ok), None) == inv
    assert L.tyr_query_tri(h, 0, None, None, None, 0, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_tri(empty.h, 4, pa, pb, pc, 8, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_tri(ta.double(), tb, tc)
    with pytest.raises(ValueError):
        g.query_tri(ta, tb[:, :2].contiguous(), tc)
    with pytest.raises(ValueError):
        g.query_tri(ta, tb, tc[:5])
    with pytest.raises(ValueError):
        g.query_tri(ta, tb[:5], tc)
    assert np.array_equal(cnt.cpu().numpy(), before) and np.array_equal(prim.cpu().numpy(), want[1])  # the refused calls wrote nothing
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_c3_tree(hip):
    """one pass on C3's 1 M-triangle tree: the 256 triangles of tests/golden/tri_c3.npz against the counts and first 32 indices
    tools/tri_c3_golden.py recorded by brute force.  Every run checks that the file belongs to these triangles and recomputes
    one query by brute force."""
    sc, nodes, prims = built_scene("mesh706")
    z = np.load(C3_ANSWERS)
    assert str(z["digest"]) == hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest(), "the recorded answers belong to other triangles"
    a, b, c, cnt, prim = (z[k] for k in ("a", "b", "c", "count", "prim"))
    assert len(a) == 256 and prim.shape == (256, KMAX) and (cnt == 0).sum() >= 16 and (cnt > KMAX).sum() >= 16 and ((cnt > 0) & (cnt <= KMAX)).sum() >= 16
    live = int(np.random.default_rng(78).integers(0, 256))
    same(ref.tri(a[live:live + 1], b[live:live + 1], c[live:live + 1], prims, KMAX), (cnt[live:live + 1], prim[live:live + 1]), "the recorded answer")
    g = renderer(hip, nodes, prims)
    same(ask(g, (a, b, c), KMAX), (cnt, prim), "C3")
    assert np.array_equal(hit(g, (a, b, c)), cnt > 0)
    assert g.query_error() == 0
    g.close()
