"""Batched k-nearest and within-radius triangle queries on the uploaded scene (tyr_query_nearest_k, hip/nearest_k.hip;
Renderer.query_nearest_k): the smallest pairs (value, index) of include/tyr_c.h "k-nearest queries" over all triangles, bit for
bit on every output against the numpy restatement (tests/nearest_k_ref.py) by brute force -- the definition has no traversal
order in it, so nothing else is needed as an oracle.

CPU: the restatement by hand and against nearest_ref, what the fixtures are for, what the compiler made of the kernel, the
ABI.  GPU: a lattice full of ties at every k with and without count and radius, exact ties across the cut by index, over-long
leaves, offset scenes and slivers, bounds and hostile input, batch sizes, optional outputs, isolation from the render, refit,
streams, argument checks, and one pass on C3's 1 M-triangle tree."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import nearest_k_ref as kref
import nearest_ref as ref
from conftest import GOLDEN, bits, built_scene
from query_support import (assert_kernel_budget, assert_query_abi, assert_render_undisturbed, box_points, build, deformed, duplicated, lattice, no_triangles, offset_soup,
                           on_side_stream, renderer, root_box, stack40, surface_points)
from query_support import same as same_outputs

F = np.float32
NAMES = ("dist2", "prim", "uv", "region", "point", "count")
K_MAX = 32


# ---- fixtures (numpy only; made once, never changed) ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup():
    """random_soup(2000) and 2048 seeded points in its root box (the box itself: with the 10 % pad of box_points three points
    in ten have no triangle within 8, and the fractions test_fixtures_reach_what_they_are_for asserts are not reached)"""
    from tyrant_amd import scenes

    nodes, prims = build(scenes.random_soup(2000))
    lo, hi = root_box(prims, inflate=0.0)
    return nodes, prims, (lo + (hi - lo) * np.random.default_rng(33).random((2048, 3))).astype(F)


def prefix(want, k):
    """the answer for k from the answer for a larger k: the definition's row for k is the first k entries"""
    return tuple(a[:, :k] for a in want[:5]) + (want[5],)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
def test_hand_cases_and_k1_is_the_nearest():
    """three coplanar copies of one triangle, one of them lifted: the order by (F, i), the strict bound, the unused entries,
    invalid input; and k = 1 is nearest_ref.nearest on a soup"""
    from tyrant_amd import scenes

    tri = scenes.make_triangles(np.array([[0, 0, 0]] * 3, F), np.array([[1, 0, 0]] * 3, F), np.array([[0, 1, 0]] * 3, F))
    tri["vert"][0] = (0, 0, 5)  # F = 16 from (0.25, 0.25, 1); the other two: F = 1
    p = [0.25, 0.25, 1.0]
    pts = np.array([p] * 6 + [[np.nan, 0, 0]], F)
    md = np.array([np.inf, 1.0, 1.5, 4.0, -1.0, np.nan, 9.0], F)
    d2, prim, uv, reg, pt, cnt = kref.nearest_k(pts, tri, 3, md)
    inf = np.inf
    assert prim.tolist() == [[1, 2, 0], [-1, -1, -1], [1, 2, -1], [1, 2, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    assert np.array_equal(bits(d2), bits(np.array([[1, 1, 16], [1, 1, 1], [1, 1, 2.25], [1, 1, 16], [inf] * 3, [inf] * 3, [inf] * 3], F)))
    assert cnt.tolist() == [3, 0, 2, 2, 0, 0, 0]  # max_dist 1: exactly the distance excludes; 4: exactly the lifted one's
    assert np.array_equal(uv[0], np.array([[0.25, 0.25]] * 3, F)) and not uv[1].any() and not uv[2, 2].any() and not reg.any()
    assert np.array_equal(pt[0], np.array([[0.25, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 5]], F))
    assert np.array_equal(pt[2, 2], pts[2]) and np.array_equal(bits(pt[6]), bits(np.repeat(pts[6:7], 3, axis=0)))
    # without max_dist, and the row for k is the first k entries of the row for a larger k
    free = kref.nearest_k(pts[:1], tri, 3)
    assert free[1].tolist() == [[1, 2, 0]] and free[5].tolist() == [3]
    two = kref.nearest_k(pts, tri, 2, md)
    for a, b in zip(two, prefix((d2, prim, uv, reg, pt, cnt), 2)):
        assert np.array_equal(a, b, equal_nan=True)
    # k = 1 against the closest-point restatement
    nodes, prims, pts = soup()
    md = np.full(len(pts), 8.0, F)
    for m in (None, md):
        one, want = kref.nearest_k(pts, prims, 1, m), ref.nearest(pts, prims, m)
        for name, a, b in zip(NAMES, one, want):
            assert np.array_equal(bits(a.reshape(b.shape)) if a.dtype == F else a.reshape(b.shape), bits(b) if b.dtype == F else b), name


def test_fixtures_reach_what_they_are_for():
    """ties inside a row and across its cut on the lattice, partly filled, full and empty rows on the soup, counts above the
    largest k, and a tree that needs more stack than the 12 LDS entries"""
    from tyrant_amd import binding

    nodes, prims, grid, _ = lattice(16, 31)
    d2, prim, _, _, _, cnt = kref.nearest_k(grid, prims, 9)
    assert (prim >= 0).all()
    eq = d2[:, :-1] == d2[:, 1:]
    tie4 = float(eq[:, :3].any(axis=1).mean())
    cut4, cut8 = float(eq[:, 3].mean()), float(eq[:, 7].mean())
    print("lattice(16): a tie inside the first 4 entries", tie4, "the 4th = the 5th value", cut4, "the 8th = the 9th", cut8)
    assert tie4 >= 0.8 and cut4 >= 0.5 and cut8 >= 0.4
    cnt25 = kref.nearest_k(grid, prims, 1, np.full(len(grid), 25.0, F))[5]
    print("lattice(16) at max_dist 25: count above 32 on", float((cnt25 > K_MAX).mean()))
    assert (cnt25 > K_MAX).mean() >= 0.5
    nodes, prims, pts = soup()
    cnt8 = kref.nearest_k(pts, prims, 1, np.full(len(pts), 8.0, F))[5]
    print("soup at max_dist 8: count above 4 on", float((cnt8 > 4).mean()), "above 8 on", float((cnt8 > 8).mean()), "none on", float((cnt8 == 0).mean()))
    assert (cnt8 > 4).mean() >= 0.4 and (cnt8 == 0).any() and ((cnt8 > 0) & (cnt8 < 8)).any() and (cnt8 > 8).any()
    nodes, prims, _, _ = lattice(32, 31)
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    nodes, prims = build(stack40())
    assert nodes["primitiveCount"].max() == 40  # an over-long leaf: synthetic records


def test_nearest_k_kernels_keep_registers_and_lds_in_budget():
    """both forms of the kernel within k_query_nearest's budget: no vector spills; scratch no larger than the LdsStack's
    private spill arrays (52 entries of 8 bytes, plus the frame's alignment); occupancy and LDS (24,576 + 7,168 bytes) that admit
    the five blocks per CU the launch bounds plan for"""
    assert_kernel_budget("nearest_k", "k_query_nearest_k", 2, (64 - 12) * 8 + 16, 24576 + 7168)


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_nearest_k", "tyr_nearest_k_out", hip.NearestKOut, 6, (r"TYR_QUERY_NEAREST_K_MAX\s+32\b",))
    assert hip.TYR_QUERY_NEAREST_K_MAX == K_MAX


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, points, k, max_dist=None, count=True, **kw):
    """the five or six outputs as numpy arrays (count as int64)"""
    out = tuple(x.cpu().numpy() for x in g.query_nearest_k(points, k, max_dist, count=count, **kw))
    return out[:5] + (out[5].astype(np.int64),) if count else out


def same(got, want, what=""):
    """every output of `got` (five, or six with the count) against `want`, bit for bit"""
    assert len(got) in (5, 6)
    same_outputs(NAMES, got, want, what)


def rows_hold_the_definition(got, points, prims, max_dist, what=""):
    """without brute force: every row sorted by (dist2, prim) with distinct triangles, the kept entries first, every kept
    entry's outputs those of pair_value for its (point, prim), every unused entry as the contract fills it"""
    d2, prim, uv, region, point = got[:5]
    n, k = prim.shape
    kept = prim >= 0
    assert (kept[:, :-1] | ~kept[:, 1:]).all(), what  # no kept entry behind an unused one
    both = kept[:, :-1] & kept[:, 1:]
    a, b, pa, pb = d2[:, :-1], d2[:, 1:], prim[:, :-1], prim[:, 1:]
    assert (~both | (a < b) | ((a == b) & (pa < pb))).all(), what
    vert, e1, e2 = ref.records(prims)
    i, j = np.nonzero(kept)
    w = prim[i, j]
    val, u2, v2, reg, c = ref.pair_value(points[i], vert[w], e1[w], e2[w])
    assert np.array_equal(bits(d2[i, j]), bits(val)) and np.array_equal(bits(uv[i, j]), bits(np.stack([u2, v2], axis=1))), what
    assert np.array_equal(region[i, j], reg) and np.array_equal(bits(point[i, j]), bits(c)), what
    ok = ref.valid_inputs(points, max_dist)
    with np.errstate(all="ignore"):
        bound2 = np.full(n, np.inf, F) if max_dist is None else (np.asarray(max_dist, F) * np.asarray(max_dist, F)).astype(F)
    bound2 = np.where(ok, bound2, F(np.inf)).astype(F)
    assert (val < bound2[i]).all(), what
    i, j = np.nonzero(~kept)
    assert np.array_equal(bits(d2[i, j]), bits(bound2[i])) and not uv[i, j].any() and not region[i, j].any(), what
    assert np.array_equal(bits(point[i, j]), bits(points[i])), what


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lattice_every_k_with_and_without_count_and_radius(hip):
    """heightfield(32): points above every grid vertex (equally near to several triangles, inside the row and across its cut)
    and seeded points; k = 1, 4, 8, 32, count off and on, unbounded and within 25"""
    nodes, prims, grid, rand = lattice(32, 31)
    pts = np.concatenate([grid, rand])
    g = renderer(hip, nodes, prims)
    for md in (None, np.full(len(pts), 25.0, F)):
        want = kref.nearest_k(pts, prims, K_MAX, md)
        assert (want[5] > K_MAX).any()
        rows = {}
        for k, count in itertools.product((1, 4, 8, 32), (False, True)):
            got = ask(g, pts, k, md, count=count)
            same(got, prefix(want, k), f"lattice, k = {k}, count = {count}, max_dist = {None if md is None else 25}")
            rows[k] = got
        one = tuple(x.cpu().numpy() for x in g.query_nearest(pts, md))
        for name, a, b in zip(NAMES, rows[1], one):
            assert np.array_equal(bits(a.reshape(b.shape)) if a.dtype == F else a.reshape(b.shape), bits(b) if b.dtype == F else b), name
        for a, b in zip(rows[4][:5], rows[32][:5]):
            assert np.array_equal(a, b[:, :4])
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_exact_ties_resolve_by_index(hip):
    """a scene concatenated with itself: every value occurs twice, so entries come in pairs of equal dist2, the lower copy's
    index first, and at an odd cut the index alone decides; and 40 identical triangles (an over-long leaf behind synthetic
    records): the row is the first 32 of them in order, the count all 40"""
    nodes, prims, pts, twin = duplicated(32, 1024)
    g = renderer(hip, nodes, prims)
    want = kref.nearest_k(pts, prims, 9)
    for k in (2, 8):
        got = ask(g, pts, k)
        same(got, prefix(want, k), f"duplicated, k = {k}")
        d2, prim = got[0], got[1]
        assert np.array_equal(bits(d2[:, 0::2]), bits(d2[:, 1::2])) and (prim[:, 0::2] < prim[:, 1::2]).all()
        whole = want[0][:, k - 1] != want[0][:, k]  # the cut does not go through a group of equal values: both copies of every entry
        assert whole.any() and not whole.all() and np.array_equal(np.sort(twin[prim[whole]], axis=1), np.sort(prim[whole], axis=1))
    got = ask(g, pts, 1)  # an odd cut through a pair: the lower copy
    same(got, prefix(want, 1), "duplicated, k = 1")
    assert (got[1][:, 0] < twin[got[1][:, 0]]).all()
    nodes, prims = build(stack40())
    g.upload(nodes, prims)
    pts = box_points(np.random.default_rng(34), prims, 1500)
    got = ask(g, pts, K_MAX)
    same(got, kref.nearest_k(pts, prims, K_MAX), "stack40")
    assert np.array_equal(got[1], np.tile(np.arange(K_MAX, dtype=np.int32), (len(pts), 1))) and (got[5] == 40).all()
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slivers", [False, True])
def test_scale_and_slack(hip, slivers):
    """a soup moved by (4096, -4096, 8192), without and with slivers: points within 1e-3 of the surface and in the root box, the
    8 nearest within 8 and their count"""
    nodes, prims = offset_soup(slivers)
    rng = np.random.default_rng(35)
    pts = np.concatenate([surface_points(rng, prims, 2048, 1e-3), box_points(rng, prims, 1024)])
    md = np.full(len(pts), 8.0, F)
    g = renderer(hip, nodes, prims)
    want = kref.nearest_k(pts, prims, 8, md)
    got = ask(g, pts, 8, md)
    same(got, want, f"offset soup, slivers={slivers}")
    assert (got[0][:2048, 0] < 1.0).all() and (got[5] > 8).any() and (got[5] < 8).any()
    same(ask(g, pts, 8, md, count=False), want, f"offset soup without count, slivers={slivers}")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_bounds_hostile_input_and_batch_sizes(hip):
    """max_dist of 0, exactly an entry's distance (strict <: that entry and what follows it are out), +inf, NaN, negative; NaN,
    infinite and 1e30 points; n = 0 .. 4097 and 400,003; every combination of the optional outputs; a scene without triangles"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    g = renderer(hip, nodes, prims)
    rng = np.random.default_rng(36)
    n, k = 400003, 8
    pts = np.stack([rng.uniform(-60, 60, n), rng.uniform(-60, 60, n), rng.uniform(-10, 110, n)], axis=1).astype(F)
    pts[:4096] = np.round(pts[:4096])  # whole numbers: distances to the axis-aligned walls whose squares are exact
    free = kref.nearest_k(pts[:4096], prims, k)
    same(ask(g, pts[:4096], k), free, "cornell, unbounded")
    third = free[0][:, 2]
    root = np.sqrt(third).astype(F)
    exact = np.nonzero(((root * root).astype(F) == third) & (third > free[0][:, 1]))[0]  # the third value, alone above the second
    assert exact.size > 500
    md = (rng.random(n) * 60).astype(F)
    md[exact] = root[exact]  # exactly the third entry's distance: two members
    kind = rng.integers(0, 40, n)
    kind[exact] = 99
    md[kind == 0] = 0.0
    md[kind == 1] = np.inf
    md[kind == 2] = np.nan
    md[kind == 3] = -1.0
    md[kind == 4] = -0.0
    bad = np.array([np.nan, np.inf, -np.inf], F)
    hostile = np.nonzero(kind == 5)[0]
    pts[hostile, rng.integers(0, 3, hostile.size)] = bad[rng.integers(0, 3, hostile.size)]
    huge = np.nonzero(kind == 6)[0]
    pts[huge, rng.integers(0, 3, huge.size)] = F(1e30)  # a valid point whose every value overflows: no member
    m = 4097
    want = kref.nearest_k(pts[:m], prims, k, md[:m])
    head = exact[exact < m]
    assert (want[5][head] == 2).all() and (want[1][head, 2] == -1).all() and np.array_equal(bits(want[0][head, 2]), bits(third[head]))
    for sel in (hostile, huge, np.nonzero((kind == 0) | (kind == 2) | (kind == 3) | (kind == 4))[0]):
        sel = sel[sel < m]
        assert sel.size and (want[5][sel] == 0).all() and (want[1][sel] == -1).all()
    got = ask(g, pts, k, md)
    same(tuple(a[:m] for a in got), want, "cornell, bounded, the first 4097")
    sample = np.random.default_rng(37).choice(n, 512, replace=False)
    same(tuple(a[sample] for a in got), kref.nearest_k(pts[sample], prims, k, md[sample]), "cornell, bounded, a sample of 400,003")
    rows_hold_the_definition(got, pts, prims, md, "cornell, bounded, n = 400,003")
    for b in (0, 1, 63, 64, 65, 4097):  # every prefix answers as the whole batch did
        same(ask(g, pts[:b], k, md[:b]), tuple(a[:b] for a in want), f"n = {b}")
    # optional outputs NULL, in every combination, through the C call; the arrays not passed stay untouched
    m = 1000
    tp, tm = torch.from_numpy(pts[:m]).cuda(), torch.from_numpy(md[:m]).cuda()
    P = C.c_void_p
    for use in itertools.product((False, True), repeat=4):  # uv, region, point, count
        outs = [torch.full((m, k), 7, dtype=torch.float32).cuda(), torch.full((m, k), 7, dtype=torch.int32).cuda(), torch.full((m, k, 2), 7, dtype=torch.float32).cuda(),
                torch.full((m, k), 7, dtype=torch.uint8).cuda(), torch.full((m, k, 3), 7, dtype=torch.float32).cuda(), torch.full((m,), 7, dtype=torch.int32).cuda()]
        torch.cuda.synchronize()
        ptr = [o.data_ptr() if u else None for o, u in zip(outs, (True, True) + use)]
        out = hip.NearestKOut(ptr[0], ptr[1], ptr[5], ptr[2], ptr[3], ptr[4])
        assert hip.lib().tyr_query_nearest_k(g.h, m, P(tp.data_ptr()), P(tm.data_ptr()), k, 0, C.byref(out), None) == 0
        assert g.query_error() == 0
        res = [o.cpu().numpy() for o in outs]
        res[5] = res[5].astype(np.int64)
        used = (True, True) + use
        for name, r, w, u in zip(NAMES, res, want, used):
            if u:
                assert np.array_equal(bits(r) if r.dtype == F else r, bits(w[:m]) if w.dtype == F else w[:m]), (use, name)
            else:
                assert (r == 7).all(), (use, name)
    # a scene without triangles: unused entries and no member
    g.upload(*no_triangles())
    same(ask(g, pts[:5000], k, md[:5000]), kref.nearest_k(pts[:5000], prims[:0], k, md[:5000]), "empty scene")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_nearest_k_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with k-nearest queries between its tyr_render calls: the same accumulation
    buffer and counters as without them"""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(-40, 40, 20000), rng.uniform(-40, 40, 20000), rng.uniform(5, 80, 20000)], axis=1).astype(F)
    md = np.full(20000, 30.0, F)
    want = kref.nearest_k(pts, prims, 8, md)

    def between(g):
        same(ask(g, pts, 8, md), want, "between two renders")
        ask(g, pts, K_MAX, count=False)

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the answers to the refitted scene's; a torch side stream works; bad arguments are
    refused before any launch and write nothing; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(24))
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    pts = box_points(np.random.default_rng(38), prims, 3000)
    md = np.full(3000, 12.0, F)
    before = kref.nearest_k(pts, prims, 8, md)
    same(ask(g, pts, 8, md), before, "before the refit")
    moved = deformed(prims, 4.0)
    g.refit(moved)
    after = kref.nearest_k(pts, moved, 8, md)
    same(ask(g, pts, 8, md), after, "after the refit")
    assert not np.array_equal(after[1], before[1]) and not np.array_equal(after[5], before[5])
    # a side stream, device tensors taken in place
    tp, tm = torch.from_numpy(pts).cuda(), torch.from_numpy(md).cuda()
    res = on_side_stream(lambda side: g.query_nearest_k(tp, 8, tm, count=True, stream=side))
    same(tuple(x.cpu().numpy() for x in res[:5]) + (res[5].cpu().numpy().astype(np.int64),), after, "side stream")

    L, h, P = hip.lib(), g.h, C.c_void_p
    d2, prim = res[0], res[1]
    kept = (d2.cpu().numpy().copy(), prim.cpu().numpy().copy())
    ok = hip.NearestKOut(d2.data_ptr(), prim.data_ptr(), None, None, None, None)
    pp = P(tp.data_ptr())
    inv = hip.TYR_ERR_INVALID
    assert L.tyr_query_nearest_k(None, 4, pp, None, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_nearest_k(h, 4, None, None, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_nearest_k(h, 4, pp, None, 8, 0, None, None) == inv
    assert L.tyr_query_nearest_k(h, 4, pp, None, 8, 0, C.byref(hip.NearestKOut(None, prim.data_ptr(), None, None, None, None)), None) == inv
    assert L.tyr_query_nearest_k(h, 4, pp, None, 8, 0, C.byref(hip.NearestKOut(d2.data_ptr(), None, None, None, None, None)), None) == inv
    assert L.tyr_query_nearest_k(h, 4, pp, None, 8, 1, C.byref(ok), None) == inv  # flags must be 0
    assert L.tyr_query_nearest_k(h, 4, pp, None, 0, 0, C.byref(ok), None) == inv  # k: 1 .. 32
    assert L.tyr_query_nearest_k(h, 4, pp, None, K_MAX + 1, 0, C.byref(ok), None) == inv
    assert L.tyr_query_nearest_k(h, 1 << 31, pp, None, 8, 0, C.byref(ok), None) == inv
    assert L.tyr_query_nearest_k(h, 0, None, None, 8, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_nearest_k(empty.h, 4, pp, None, 8, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    for bad in (lambda: g.query_nearest_k(tp.double(), 8), lambda: g.query_nearest_k(tp[:, :2].contiguous(), 8), lambda: g.query_nearest_k(tp, 8, tm[:5]),
                lambda: g.query_nearest_k(tp, 0), lambda: g.query_nearest_k(tp, K_MAX + 1)):
        with pytest.raises(ValueError):
            bad()
    assert np.array_equal(bits(d2.cpu().numpy()), bits(kept[0])) and np.array_equal(prim.cpu().numpy(), kept[1])  # the refused calls wrote nothing
    assert g.query_error() == 0
    g.close()


C3_RADIUS = 0.2


@pytest.mark.gpu
def test_c3_tree(hip):
    """one pass on C3's 1 M-triangle tree with the points of tests/golden/nearest_c3.npz (test_point_query.c3_points): k = 1
    against the recorded brute-force answers; the 8 nearest within a radius, with the count, held to the definition row by row
    and, for a seeded sample of 64 points, against brute force over the million triangles (64 M pair evaluations: some twenty
    seconds of numpy)"""
    import hashlib

    sc, nodes, prims = built_scene("mesh706")
    rng = np.random.default_rng(27)
    pts = np.concatenate([box_points(rng, prims, 2048), surface_points(rng, prims, 2048, 0.5)])
    z = np.load(os.path.join(GOLDEN, "nearest_c3.npz"))
    assert str(z["digest"]) == hashlib.sha256(np.ascontiguousarray(pts).tobytes() + np.ascontiguousarray(prims).tobytes()).hexdigest(), "the recorded answers belong to other points or triangles"
    best, arg = z["dist2"], z["prim"]
    vert, e1, e2 = ref.records(prims)
    val, u2, v2, reg, c = ref.pair_value(pts, vert[arg], e1[arg], e2[arg])
    assert np.array_equal(bits(val), bits(best))
    g = renderer(hip, nodes, prims)
    one = ask(g, pts, 1, count=False)
    same(one, (val[:, None], arg.astype(np.int32)[:, None], np.stack([u2, v2], axis=1)[:, None], reg[:, None], c[:, None]), "C3, k = 1")
    # a radius per point: that of its nearest triangle and C3_RADIUS more, so that every row has an entry; in the sample the
    # counts run from 1 to 160
    md = (np.sqrt(best) + F(C3_RADIUS)).astype(F)
    got = ask(g, pts, 8, md)
    rows_hold_the_definition(got, pts, prims, md, "C3, k = 8")
    for a, b in zip(got[:5], one):
        assert np.array_equal(a[:, :1], b)
    filled = (got[1] >= 0).sum(axis=1)
    assert (filled >= 1).all() and (filled == np.minimum(got[5], 8)).all()
    sample = np.random.default_rng(39).choice(len(pts), 64, replace=False)
    want = kref.nearest_k(pts[sample], prims, 8, md[sample])
    assert (want[5] == 1).any() and ((want[5] > 1) & (want[5] < 8)).any() and (want[5] > K_MAX).any()  # partly filled and full rows
    same(tuple(a[sample] for a in got), want, "C3, k = 8, brute force on a sample")
    assert g.query_error() == 0
    g.close()
