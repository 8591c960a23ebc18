"""Batched box-overlap queries on the uploaded scene (tyr_query_box, hip/box.hip; Renderer.query_box): the member set of
include/tyr_c.h "Box-overlap queries" over all triangles, bit for bit against its numpy restatement (tests/box_ref.py) by brute
force -- the definition has no traversal order in it, so nothing else is needed as an oracle.

CPU: the restatement by hand, the restatement against the same 13 axes in exact rational arithmetic, the pruning argument on the
fixtures' trees, what the fixtures are for, what the compiler made of the kernels, the ABI.  GPU: a lattice with boxes on its
grid lines, duplicated triangles, an over-long leaf, offset scenes and slivers, row lengths and the ANY flag, batch sizes, hostile
input, isolation from the render, refit, streams, argument checks, and one pass on C3's 1 M-triangle tree."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest

import box_ref as ref
from conftest import GOLDEN, built_scene
from query_support import (OFFSET, assert_kernel_budget, assert_query_abi, assert_render_undisturbed, box_points, build, deformed, duplicated, lattice, launch_bounds_blocks,
                           no_triangles, offset_soup, on_side_stream, renderer, stack40, surface_points, tri)
from query_support import same as same_outputs

F = np.float32
D = np.float64
C3_ANSWERS = os.path.join(GOLDEN, "box_c3.npz")
INF = F(np.inf)
KMAX = 32


def up(x):
    return np.nextafter(F(x), INF)


def down(x):
    return np.nextafter(F(x), -INF)


# ---- fixtures (numpy only) --------------------------------------------------------------------------------------------
def cubes(rng, centres, lo_exp=-1.0, hi_exp=1.2):
    """boxes round `centres` with seeded half extents of 10^lo_exp .. 10^hi_exp per axis"""
    half = (10.0 ** rng.uniform(lo_exp, hi_exp, centres.shape)).astype(F)
    return (centres - half).astype(F), (centres + half).astype(F)


@functools.lru_cache(maxsize=None)
def lattice_case():
    """heightfield(32), grid step 3.125 (exact in binary32): (nodes, prims, (lo, hi), the parts' slices, (count, prim) for 32)"""
    nodes, prims, grid, _ = lattice(32, 21)
    rng = np.random.default_rng(61)
    xs = np.linspace(-50.0, 50.0, 33).astype(F)
    step = F(3.125)
    parts, los, his = {}, [], []

    def add(name, lo, hi):
        at = sum(len(a) for a in los)
        parts[name] = slice(at, at + len(lo))
        los.append(np.asarray(lo, F).reshape(-1, 3))
        his.append(np.asarray(hi, F).reshape(-1, 3))

    # faces exactly on grid lines: 1 x 1 to 3 x 2 cells, the whole height
    i, j = rng.integers(0, 30, 96), rng.integers(0, 30, 96)
    w, h = rng.integers(1, 4, 96), rng.integers(1, 3, 96)
    add("grid", np.stack([xs[i], xs[j], np.full(96, -100, F)], 1), np.stack([xs[i + w], xs[j + h], np.full(96, 100, F)], 1))
    # round single vertices: the six triangles that meet there (fewer on the rim)
    v = grid[rng.permutation(len(grid))[:128]]
    add("vertex", v - np.array([0.5, 0.5, 140], F), v + np.array([0.5, 0.5, 60], F))
    # zero extent on one axis (a rectangle in a grid plane), on two (a vertical segment through a vertex, and a seeded one)
    # and on three (corners of triangles as points, and seeded points)
    i, j = rng.integers(0, 31, 64), rng.integers(0, 31, 64)
    add("rectangle", np.stack([xs[i], xs[j], np.full(64, -100, F)], 1), np.stack([xs[i], xs[j] + step * F(2), np.full(64, 100, F)], 1))
    seg = np.concatenate([grid[rng.permutation(len(grid))[:48], :2], box_points(rng, prims, 48)[:, :2]])
    add("segment", np.concatenate([seg, np.full((96, 1), -100, F)], 1), np.concatenate([seg, np.full((96, 1), 100, F)], 1))
    pts = np.concatenate([prims["vert"][rng.permutation(len(prims))[:48]], surface_points(rng, prims, 16, 0.0)])
    add("point", pts, pts)
    # mixed sizes: half of them round points near the surface, half anywhere in the inflated root box
    c = np.concatenate([surface_points(rng, prims, 224, 2.0), box_points(rng, prims, 224)])
    add("seeded", *cubes(rng, c, -1.0, 1.1))
    add("everything", [[-1000, -1000, -1000]], [[1000, 1000, 1000]])
    lo, hi = np.ascontiguousarray(np.concatenate(los)), np.ascontiguousarray(np.concatenate(his))
    return nodes, prims, (lo, hi), parts, ref.box(lo, hi, prims, KMAX)


@functools.lru_cache(maxsize=None)
def pair_families():
    """seeded (box, triangle) pairs, every box built round a point of its triangle: name -> (lo, hi, vert, e1, e2)"""
    rng = np.random.default_rng(62)

    def soup(n, off=0.0):
        vert = (rng.uniform(-4, 4, (n, 3)) + off).astype(F)
        return vert, rng.uniform(-1, 1, (n, 3)).astype(F), rng.uniform(-1, 1, (n, 3)).astype(F)

    def boxes(vert, e1, e2, spread=0.6, lo_exp=-2.0, hi_exp=-0.2):
        n = len(vert)
        u = rng.random((n, 1))
        v = rng.random((n, 1)) * (1 - u)
        scale = np.maximum(np.abs(e1).max(1, keepdims=True), np.abs(e2).max(1, keepdims=True)).astype(D)
        c = vert.astype(D) + u * e1 + v * e2 + rng.normal(size=(n, 3)) * spread * scale
        half = 10.0 ** rng.uniform(lo_exp, hi_exp, (n, 3)) * scale
        half[rng.random((n, 3)) < 0.05] = 0  # some boxes flat on an axis
        return (c - half).astype(F), (c + half).astype(F)

    fam = {}
    t = soup(6000)
    fam["unit"] = boxes(*t) + t
    t = soup(5000, OFFSET.astype(D))
    fam["offset"] = boxes(*t) + t
    _, prims = offset_soup(True)
    w = np.concatenate([np.arange(0, 2000, 10), rng.integers(0, 2000, 3800)])  # every sliver, and seeded others
    t = tuple(a[w] for a in ref.records(prims))
    fam["slivers"] = boxes(*t, spread=0.3) + t
    # a face of the box exactly through a corner of the triangle: on one or two axes (a face or an edge of the box through the
    # corner), and on all three (a corner of the box on it)
    for name, n, axes in (("faces", 5000, (1, 3)), ("corner_on_corner", 2000, (3, 4))):
        t = soup(n)
        lo, hi = boxes(*t)
        A, B, Cc = (a.astype(F) for a in ref.corners(*t))
        corner = np.choose(rng.integers(0, 3, (n, 1)), [A, B, Cc])
        through = np.argsort(rng.random((n, 3)), axis=1) < rng.integers(*axes, (n, 1))  # that many axes of each pair
        side = np.where(through, rng.integers(1, 3, (n, 3)), 0)  # 0: keep, 1: lo through the corner, 2: hi through it
        ext = (hi - lo).astype(F)
        lo = np.where(side == 1, corner, np.where(side == 2, (corner - ext).astype(F), lo))
        hi = np.where(side == 2, corner, np.where(side == 1, (corner + ext).astype(F), hi))
        fam[name] = (lo.astype(F), hi.astype(F)) + t
    return fam


def tree_facts(nodes, prims):
    """of a depth-first node array (left child i + 1, right child `offset`; a leaf holds offset .. offset + primitiveCount - 1):
    (every child's box lies in its parent's, every corner of a leaf's triangles lies in the leaf's box, the leaves' offsets in
    node order)"""
    A, B, Cc = (a.astype(F) for a in ref.corners(*ref.records(prims)))
    cmin, cmax = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
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
    return nested, holds, nodes["offset"][leaf].astype(np.int64), nodes["primitiveCount"][leaf].astype(np.int64)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0))    # the unit right triangle in z = 0
TILTED = ((0, 0, 0), (1, 0, 1), (0, 1, 1))  # in the plane z = x + y
TILTX = ((0, 0, 0), (1, 0, 0), (0, 1, 1))   # in the plane z = y
HAND = [  # triangle, lo, hi, the first separating axis (0: a member)
    (UNIT, (2, 0, -1), (3, 1, 1), 1),  # a box axis alone separates: x, y, z
    (UNIT, (0, 2, -1), (1, 3, 1), 2),
    (UNIT, (0, 0, 1), (1, 1, 2), 3),
    (TILTED, (0.5, 0.5, 0), (1, 1, 0.25), 4),  # inside the bounding box, below the plane: the plane alone
    (UNIT, (0.75, 0.75, -1), (1, 1, 1), 12),  # inside the bounding box, beyond the hypotenuse: cross(unit_z, e2' - e1') alone
    (UNIT, (1, -1, -1), (2, 1, 1), 0),  # a face through the vertex B; one binary32 step away
    (UNIT, (up(1), -1, -1), (2, 1, 1), 1),
    (UNIT, (1, 0, 0), (2, 1, 1), 0),  # a corner on the vertex B
    (UNIT, (up(1), 0, 0), (2, 1, 1), 1),
    (UNIT, (0.5, 0.5, -1), (1, 1, 1), 0),  # a vertical edge on the hypotenuse
    (UNIT, (up(0.5), 0.5, -1), (1, 1, 1), 12),
    (UNIT, (-1, 0.25, -1), (0, 0.75, 1), 0),  # a face along the edge A -> C
    (UNIT, (-1, 0.25, -1), (down(0), 0.75, 1), 1),
    (UNIT, (0.125, 0.125, 0), (0.25, 0.25, 1), 0),  # a face in the triangle's plane
    (UNIT, (0.125, 0.125, up(0)), (0.25, 0.25, 1), 3),
    (TILTX, (0.25, 0.5, -1), (0.5, 1, 0.5), 0),  # an edge of the box lying in the face: (0.25 .. 0.5, 0.5, 0.5)
    (TILTX, (0.25, 0.5, -1), (0.5, 1, down(0.5)), 4),
    (TILTED, (0.25, 0.25, -1), (1, 1, 0.5), 0),  # a corner in the face's interior: (0.25, 0.25, 0.5)
    (TILTED, (0.25, 0.25, -1), (1, 1, down(0.5)), 4),
    (TILTED, (up(0.25), 0.25, -1), (1, 1, 0.5), 4),
    (UNIT, (0.25, 0.25, 0), (0.25, 0.25, 0), 0),  # a point on the triangle, above it, beyond the hypotenuse
    (UNIT, (0.25, 0.25, 0.5), (0.25, 0.25, 0.5), 3),
    (UNIT, (0.75, 0.75, 0), (0.75, 0.75, 0), 12),
    (TILTED, (0.25, 0.5, 0.75), (0.25, 0.5, 0.75), 0),
    (TILTED, (0.25, 0.5, up(0.75)), (0.25, 0.5, up(0.75)), 4),
    (UNIT, (-1, -1, -1), (2, 2, 2), 0),  # the box holds the triangle
    (UNIT, (0.25, 0.25, -0.125), (0.375, 0.375, 0.125), 0),  # inside the face's outline, straddling the plane
    (((0, 0, 0), (0, 0, 0), (0, 0, 0)), (-1, -1, -1), (1, 1, 1), 0),  # the zero triangle: a point
    (((0, 0, 0), (0, 0, 0), (0, 0, 0)), (0, 0, 0), (0, 0, 0), 0),
    (((0, 0, 0), (0, 0, 0), (0, 0, 0)), (0.5, 0.5, 0.5), (1, 1, 1), 1),
    (((0, 0, 0), (1, 1, 0), (2, 2, 0)), (1, 0.5, -1), (1.5, 1.25, 1), 0),  # e2 = 2 e1: the segment (0, 0, 0) -> (2, 2, 0)
    (((0, 0, 0), (1, 1, 0), (2, 2, 0)), (1, 0, -1), (1.5, 0.5, 1), 11),  # inside its bounding box, off the segment
    (((0, 0, 0), (1, 1, 0), (2, 2, 0)), (1, 0, -1), (1.5, 1, 1), 0),  # a corner of the outline on it
]


def test_hand_cases():
    """exactly representable numbers on the unit right triangle and two tilted triangles: a box that each class of axis alone
    separates; boxes touching a vertex, an edge and the face with a face, an edge and a corner of their own, and the same boxes
    one binary32 step away; point boxes; a box round the triangle and one in the face's interior; the zero triangle and a segment;
    every invalid input.  The exact test agrees on each."""
    for (vert, e1, e2), lo, hi, axis in HAND:
        got = int(ref.pair(np.array(lo, F), np.array(hi, F), np.array(vert, F), np.array(e1, F), np.array(e2, F)))
        assert got == axis, (vert, e1, e2, lo, hi, got)
        assert ref.pair_exact(lo, hi, vert, e1, e2) == axis, (lo, hi)
        cnt, prim = ref.box(np.array([lo], F), np.array([hi], F), tri(vert, e1, e2), 2)
        assert (cnt.tolist(), prim.tolist()) == ([int(axis == 0)], [[0 if axis == 0 else -1, -1]])
    # the set, its count beyond the row, the row ascending, ANY; every invalid input
    three = np.concatenate([tri((0, 0, 5), (1, 0, 0), (0, 1, 0)), tri(*UNIT), tri(*TILTED), tri(*UNIT)])
    nan, inf = np.nan, np.inf
    lo = np.array([[0.25, 0.25, -1]] * 10, F)
    hi = np.array([[0.5, 0.5, 1]] * 10, F)
    lo[1, 0], lo[2, 2], hi[3, 1], hi[4, 0], lo[5, 1] = nan, -inf, nan, inf, inf
    lo[6, 0], lo[7, 1], lo[8, 2] = up(0.5), up(0.5), up(1)  # lo_k > hi_k on one axis only
    lo[9], hi[9] = (0.25, 0.25, 4), (0.5, 0.5, 4.5)
    cnt, prim = ref.box(lo, hi, three, 2)
    assert cnt.tolist() == [3] + [0] * 9 and prim.tolist() == [[1, 2]] + [[-1, -1]] * 9
    assert ref.box(lo, hi, three, 0)[0].tolist() == cnt.tolist() and ref.box(lo, hi, three, 0)[1].shape == (10, 0)
    assert ref.box(lo, hi, three, 32)[1][0].tolist() == [1, 2, 3] + [-1] * 29
    assert ref.box(lo, hi, three, any=True).tolist() == [True] + [False] * 9
    assert ref.box(lo[:1], hi[:1], three[:0], 2)[0].tolist() == [0]  # no triangles: nothing


def test_restatement_against_exact_arithmetic():
    """the binary64 test against the same 13 axes in exact rational arithmetic on the same binary32 inputs, 22,000 seeded pairs:
    unit scale, moved by OFFSET, slivers, and boxes with a face or an edge exactly through a triangle corner -- the same first
    separating axis on every pair.  The fifth family puts a CORNER of the box on a triangle corner: where that is B or C the
    plane's normal, rounded, is no longer exactly perpendicular to e1' or e2', and the binary64 test can see the touching box a
    rounding error off the plane.  Such a pair may disagree only if its exact answer flips when every box face moves by one
    binary32 step, and only by the plane axis; the count is printed."""
    total, wrong = 0, {}
    for name, (lo, hi, vert, e1, e2) in pair_families().items():
        got = ref.pair(lo, hi, vert, e1, e2)
        exact = np.array([ref.pair_exact(lo[i], hi[i], vert[i], e1[i], e2[i]) for i in range(len(lo))])
        agree = (got == 0) == (exact == 0)
        for i in np.nonzero(~agree)[0]:  # allowed only next to a flip: the exact answer with every face one step out, and one step in
            out = ref.pair_exact(down(lo[i]), up(hi[i]), vert[i], e1[i], e2[i]) == 0
            into = ref.pair_exact(np.minimum(up(lo[i]), hi[i]), np.maximum(down(hi[i]), lo[i]), vert[i], e1[i], e2[i]) == 0
            assert out != into and {int(got[i]), int(exact[i])} == {0, 4}, (name, int(i), int(got[i]), int(exact[i]))
        wrong[name] = int((~agree).sum())
        assert np.array_equal(got[agree], exact[agree]), name  # and the same first axis
        total += len(lo)
    print("pairs:", total, "disagreements with the exact answer per family:", wrong)
    assert total >= 20000 and all(v == 0 for k, v in wrong.items() if k != "corner_on_corner"), wrong


def test_pruning_argument_holds_on_the_fixtures_trees():
    """every triangle's corners A, B, C lie in its leaf's box and every box in its parent's, so in every ancestor's: a node whose
    box misses [lo, hi] holds no member.  And the observation hip/box.hip's insertion is fast for but does not rely on: the
    leaves' primitive ranges follow each other in node order, so members arrive ascending."""
    from tyrant_amd import scenes

    trees = [lattice(32, 21)[:2], duplicated(22, 2048)[:2], build(stack40()), offset_soup(False), offset_soup(True), build(scenes.heightfield(16)), build(scenes.cornell_box().triangles)]
    for nodes, prims in trees:
        nested, holds, offsets, counts = tree_facts(nodes, prims)
        assert nested and holds
        assert offsets[0] == 0 and np.array_equal(offsets[1:], (offsets + counts)[:-1]) and offsets[-1] + counts[-1] == len(prims)


def test_fixtures_reach_what_they_are_for():
    """each of the 13 axes is the first separator of at least 10 seeded pairs (the plane's and the edges' where every box axis
    passes) and none of at least 200; the lattice's boxes are empty, fit a row of 5 and overflow it, at least 20 each; the
    lattice's tree needs more stack than the 12 LDS entries; stack40 has an over-long leaf"""
    from tyrant_amd import binding

    first = np.concatenate([ref.pair(*f) for f in pair_families().values()])
    hist = np.bincount(first, minlength=14)
    print("first separating axis, 0 = member:", hist.tolist())
    assert hist[0] >= 200 and (hist[1:] >= 10).all(), hist.tolist()
    nodes, prims, (lo, hi), parts, (cnt, prim) = lattice_case()
    assert (cnt == 0).sum() >= 20 and ((cnt > 0) & (cnt <= 5)).sum() >= 20 and (cnt > 5).sum() >= 20 and (cnt > KMAX).sum() >= 20
    grid = lattice(32, 21)[2][:, :2]
    v = (lo[parts["vertex"]] + F(0.5))[:, :2]
    inner = (np.abs(v) < 49).all(axis=1)
    assert inner.sum() >= 64 and (cnt[parts["vertex"]][inner] == 6).all() and len(grid) == 33 * 33
    corners = cnt[parts["point"]][:48]  # a triangle's corner belongs to its neighbours too; a rounded point of a face is off it
    assert (corners >= 1).all() and (corners >= 2).sum() >= 32
    assert cnt[parts["everything"]].tolist() == [len(prims)] and prim[parts["everything"]][0].tolist() == list(range(KMAX))
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    nodes, prims = build(stack40())
    assert nodes["primitiveCount"].max() == 40  # an over-long leaf: synthetic records


def test_box_kernels_keep_registers_and_lds_in_budget():
    """exactly two k_query_box kernels (with and without ANY); no vector spills; scratch no larger than the LdsStack's private
    spill array (52 entries of 4 bytes, plus the frame's alignment); LDS (12,288 + 7,168 bytes) that admits the blocks per CU the
    launch bounds plan for.  The occupancy reached is printed (DESIGN.md "Box-overlap queries" records it), not prescribed."""
    assert_kernel_budget("box", "k_query_box", 2, (64 - 12) * 4 + 16, 12288 + 7168, planned=launch_bounds_blocks("box", "k_query_box"))


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_box", "tyr_box_out", hip.BoxOut, 2, (r"TYR_QUERY_BOX_ANY\s+4u\b", r"TYR_QUERY_BOX_MAX\s+32\b"))
    assert (hip.TYR_QUERY_BOX_ANY, hip.TYR_QUERY_BOX_MAX) == (4, KMAX)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, lo, hi, k=0, **kw):
    """(count, prim) as numpy arrays; prim of shape (n, 0) for a count alone"""
    res = g.query_box(np.array(lo), np.array(hi), max_prims=k, **kw)
    cnt, prim = res if k else (res, None)
    cnt = cnt.cpu().numpy()
    return cnt, (prim.cpu().numpy() if k else np.zeros((len(cnt), 0), np.int32))


same = functools.partial(same_outputs, ("count", "prim"))


def check(g, prims, lo, hi, k, what=""):
    got = ask(g, lo, hi, k)
    want = ref.box(lo, hi, prims, k)
    same(got, want, what)
    return got


def prefix(want, k, rows=slice(None)):
    """the answer for a row of k from the answer for a longer one"""
    return want[0][rows], np.ascontiguousarray(want[1][rows, :k])


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lattice_and_ties(hip):
    """heightfield(32): boxes whose faces lie exactly on grid lines (touching is exact), boxes round single vertices (the six
    triangles there, ascending), boxes of zero extent on one, two and three axes, 448 seeded boxes, and one box round everything
    (count = the number of triangles, the row 0 .. 31: more stack than the LDS part holds)"""
    nodes, prims, (lo, hi), parts, want = lattice_case()
    g = renderer(hip, nodes, prims)
    got = ask(g, lo, hi, KMAX)
    same(got, want, "lattice")
    assert got[0][parts["everything"]].tolist() == [len(prims)] and (got[0][parts["vertex"]] == 6).sum() >= 64
    rows = got[1][parts["vertex"]][got[0][parts["vertex"]] == 6][:, :6]
    assert (np.diff(rows, axis=1) > 0).all()
    same(ask(g, lo, hi, 0), prefix(want, 0), "a count alone")
    assert np.array_equal(g.query_box(lo, hi, any=True).cpu().numpy(), want[0] > 0)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_duplicated_triangles_and_the_over_long_leaf(hip):
    """a scene concatenated with itself: both copies of every member are listed, the lower index first; 40 identical triangles
    (an over-long leaf behind synthetic records), alone and next to the Cornell box, with rows of 1, 5 and 32"""
    from tyrant_amd import scenes

    nodes, prims, pts, twin = duplicated(22, 2048)
    rng = np.random.default_rng(63)
    lo, hi = cubes(rng, np.concatenate([pts[:289] - np.array([0, 0, 40], F), surface_points(rng, prims, 351, 1.0)]), -1.0, 0.8)
    g = renderer(hip, nodes, prims)
    cnt, prim = check(g, prims, lo, hi, KMAX, "duplicated")
    whole = (cnt > 0) & (cnt <= KMAX)
    assert whole.sum() >= 100 and (cnt[whole] % 2 == 0).all()
    for row, c in zip(prim[whole], cnt[whole]):
        assert set(twin[row[:c]].tolist()) == set(row[:c].tolist())
    for tris in (stack40(), np.concatenate([scenes.cornell_box().triangles, stack40()])):
        nodes, prims = build(tris)
        g.upload(nodes, prims)
        c = np.concatenate([surface_points(rng, prims, 300, 3.0), box_points(rng, prims, 200)])
        lo, hi = cubes(rng, c, -1.0, 1.3)
        want = ref.box(lo, hi, prims, KMAX)
        assert (want[0] >= 40).sum() >= 50
        for k in (1, 5, KMAX):
            same(ask(g, lo, hi, k), prefix(want, k), f"stack40, a row of {k}")
        assert np.array_equal(g.query_box(lo, hi, any=True).cpu().numpy(), want[0] > 0)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slivers", [False, True])
def test_offset_scenes(hip, slivers):
    """a soup moved by (4096, -4096, 8192), without and with slivers: boxes round points of the surface from a binary32 step
    across to larger than a triangle, some through triangle corners, and boxes anywhere in the root box"""
    nodes, prims = offset_soup(slivers)
    rng = np.random.default_rng(64)
    lo, hi = cubes(rng, np.concatenate([surface_points(rng, prims, 640, 0.05), box_points(rng, prims, 256)]), -3.5, 1.4)
    A, B, Cc = (a.astype(F) for a in ref.corners(*ref.records(prims)))
    w = rng.integers(0, len(prims), 128)
    lo[:128, 0], hi[128:256, 1] = B[w, 0], Cc[w, 1]  # (a face through a corner: of another triangle than the box was made for)
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    g = renderer(hip, nodes, prims)
    cnt, _ = check(g, prims, lo, hi, 2, f"offset soup, slivers={slivers}")
    assert (cnt == 0).sum() >= 50 and (cnt > 0).sum() >= 300 and (cnt > 2).sum() >= 20
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_shapes_flags_hostile_input_and_batch_sizes(hip):
    """the lattice: rows of 0, 1, 5 and 32 are prefixes of each other; ANY equals count > 0; n = 1 .. 4097; the same boxes
    shuffled answer the same; NaN, infinite and inverted boxes among good ones touch nothing and disturb nothing; a scene
    without triangles"""

    nodes, prims, (lo, hi), parts, want32 = lattice_case()
    rng = np.random.default_rng(65)
    pick = rng.integers(0, len(lo), 4097)
    lo, hi = np.ascontiguousarray(lo[pick]), np.ascontiguousarray(hi[pick])
    kind = rng.integers(0, 24, 4097)
    bad = np.array([np.nan, np.inf, -np.inf], F)
    for code, arr in ((0, lo), (1, hi)):
        w = np.nonzero(kind == code)[0]
        arr[w, rng.integers(0, 3, w.size)] = bad[rng.integers(0, 3, w.size)]
    w = np.nonzero(kind == 2)[0]
    ax = rng.integers(0, 3, w.size)
    lo[w, ax] = up(hi[w, ax])  # lo_k > hi_k by one step on one axis
    want = ref.box(lo, hi, prims, KMAX)
    invalid = ~ref.valid_boxes(lo, hi)
    assert invalid.sum() >= 300 and not want[0][invalid].any() and (want[1][invalid] == -1).all()
    ok = ~invalid
    assert np.array_equal(want[0][ok], want32[0][pick][ok]) and np.array_equal(want[1][ok], want32[1][pick][ok])
    g = renderer(hip, nodes, prims)
    for k in (0, 1, 5, KMAX):
        same(ask(g, lo, hi, k), prefix(want, k), f"a row of {k}")
    assert np.array_equal(g.query_box(lo, hi, any=True).cpu().numpy(), want[0] > 0)
    for m in (1, 63, 64, 65, 257):  # every prefix answers as the whole batch did
        same(ask(g, lo[:m], hi[:m], 5), prefix(want, 5, slice(0, m)), f"n = {m}")
        assert np.array_equal(g.query_box(lo[:m], hi[:m], any=True).cpu().numpy(), want[0][:m] > 0)
    order = rng.permutation(4097)
    same(ask(g, lo[order], hi[order], 5), prefix(want, 5, order), "shuffled")
    with pytest.raises(ValueError):
        g.query_box(lo, hi, max_prims=KMAX + 1)
    with pytest.raises(ValueError):
        g.query_box(lo, hi, max_prims=1, any=True)
    g.upload(*no_triangles())
    same(ask(g, lo, hi, 5), ref.box(lo, hi, prims[:0], 5), "empty scene")
    assert not g.query_box(lo, hi, any=True).any().item()
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_box_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with box queries between its tyr_render calls: the same accumulation buffer and
    counters as without them"""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    rng = np.random.default_rng(66)
    lo, hi = cubes(rng, box_points(rng, prims, 20000), -1.0, 1.3)
    want = ref.box(lo, hi, prims, 4)

    def between(g):
        same(ask(g, lo, hi, 4), want, "between two renders")
        g.query_box(lo, hi, any=True)

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the answers to the refitted scene's; a torch side stream and the ctx's stream work; bad
    arguments are refused before any launch; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(16))
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    rng = np.random.default_rng(67)
    n = 1000
    lo, hi = cubes(rng, surface_points(rng, prims, n, 2.0), -0.5, 0.8)
    check(g, prims, lo, hi, 8, "before the refit")
    moved = deformed(prims, 4.0)
    g.refit(moved)
    check(g, moved, lo, hi, 8, "after the refit")
    want = ref.box(lo, hi, moved, 8)
    assert not np.array_equal(want[0], ref.box(lo, hi, prims, 8)[0])
    # a side stream, device tensors taken in place; then the ctx's own stream (NULL) through the C call
    tl, th = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    (cnt, prim), hit = on_side_stream(lambda side: (g.query_box(tl, th, max_prims=8, stream=side), g.query_box(tl, th, any=True, stream=side)))
    same((cnt.cpu().numpy(), prim.cpu().numpy()), want, "side stream")
    assert np.array_equal(hit.cpu().numpy(), want[0] > 0)

    L, h, P = hip.lib(), g.h, C.c_void_p
    cnt, prim = torch.full((n,), 7, dtype=torch.int32).cuda(), torch.full((n, 8), 7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    ok = hip.BoxOut(cnt.data_ptr(), prim.data_ptr())
    counts = hip.BoxOut(cnt.data_ptr(), None)
    pl, ph = P(tl.data_ptr()), P(th.data_ptr())
    ANY = hip.TYR_QUERY_BOX_ANY
    assert L.tyr_query_box(h, n, pl, ph, 8, 0, C.byref(ok), None) == 0
    assert g.query_error() == 0  # (waits for the ctx's stream)
    same((cnt.cpu().numpy(), prim.cpu().numpy()), want, "the ctx's stream")
    assert L.tyr_query_box(h, n, pl, ph, 0, ANY, C.byref(counts), None) == 0  # out->prim is ignored with max_prims == 0
    assert g.query_error() == 0
    assert np.array_equal(cnt.cpu().numpy(), (want[0] > 0).astype(np.int32)) and np.array_equal(prim.cpu().numpy(), want[1])
    before = cnt.cpu().numpy().copy()
    inv = hip.TYR_ERR_INVALID
    assert L.tyr_query_box(None, 4, pl, ph, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_box(h, 4, None, ph, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_box(h, 4, pl, None, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_box(h, 4, pl, ph, 8, 0, None, None) == inv
    assert L.tyr_query_box(h, 4, pl, ph, 8, 0, C.byref(hip.BoxOut(None, prim.data_ptr())), None) == inv
    assert L.tyr_query_box(h, 4, pl, ph, 8, 0, C.byref(counts), None) == inv  # out->prim NULL with max_prims > 0
    assert L.tyr_query_box(h, 1 << 31, pl, ph, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_box(h, 4, pl, ph, KMAX + 1, 0, C.byref(ok), None) == inv
    for flags in (1, 2, 8, ANY | 1):  # TYR_QUERY_SPHERES and TYR_QUERY_TWO_SIDED included
        assert L.tyr_query_box(h, 4, pl, ph, 0, flags, C.byref(ok), None) == inv
    assert L.tyr_query_box(h, 4, pl, ph, 1, ANY, C.byref(ok), None) == inv  # ANY answers without indices
    assert L.tyr_query_box(h, 0, None, None, 0, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_box(empty.h, 4, pl, ph, 8, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_box(tl.double(), th)
    with pytest.raises(ValueError):
        g.query_box(tl, th[:, :2].contiguous())
    with pytest.raises(ValueError):
        g.query_box(tl, th[:5])
    assert np.array_equal(cnt.cpu().numpy(), before)  # the refused calls wrote nothing
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_c3_tree(hip):
    """one pass on C3's 1 M-triangle tree: the 256 boxes of tests/golden/box_c3.npz against the counts and first 32 indices
    tools/box_c3_golden.py recorded by brute force.  Every run checks that the file belongs to these triangles and recomputes
    one box by brute force."""
    sc, nodes, prims = built_scene("mesh706")
    z = np.load(C3_ANSWERS)
    assert str(z["digest"]) == hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest(), "the recorded answers belong to other triangles"
    lo, hi, cnt, prim = (z[k] for k in ("lo", "hi", "count", "prim"))
    assert len(lo) == 256 and prim.shape == (256, KMAX) and (cnt == 0).sum() >= 16 and (cnt > KMAX).sum() >= 16 and ((cnt > 0) & (cnt <= KMAX)).sum() >= 16
    live = int(np.random.default_rng(68).integers(0, 256))
    same(ref.box(lo[live:live + 1], hi[live:live + 1], prims, KMAX), (cnt[live:live + 1], prim[live:live + 1]), "the recorded answer")
    g = renderer(hip, nodes, prims)
    same(ask(g, lo, hi, KMAX), (cnt, prim), "C3")
    assert np.array_equal(g.query_box(lo, hi, any=True).cpu().numpy(), cnt > 0)
    assert g.query_error() == 0
    g.close()
