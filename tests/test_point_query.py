"""Batched closest-point queries on the uploaded scene (tyr_query_nearest, hip/nearest.hip; Renderer.query_nearest): the argmin
of include/tyr_c.h "Closest-point queries" over all triangles, bit for bit against its numpy restatement (tests/nearest_ref.py)
by brute force -- the definition has no traversal order in it, so nothing else is needed as an oracle.

CPU: the restatement by hand, its one-sided bound against float64, what the fixtures are for, what the compiler made of the
kernel, the ABI.  GPU: lattices with shared edges and vertices, exact ties by index, over-long leaves, offset scenes and slivers,
bounds and hostile input, batch sizes, optional outputs, isolation from the render, refit, streams, argument checks, and one
pass on C3's 1 M-triangle tree."""
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest

import nearest_ref as ref
from conftest import GOLDEN, ROOT, bits, built_scene
from query_support import (OFFSET, assert_kernel_budget, assert_query_abi, assert_render_undisturbed, box_points, build, deformed, duplicated, lattice, no_triangles,
                           offset_soup, on_side_stream, renderer, stack40, surface_points)
from query_support import same as same_outputs

F = np.float32
C3_ANSWERS = os.path.join(GOLDEN, "nearest_c3.npz")


# ---- fixtures (numpy only) --------------------------------------------------------------------------------------------
def tie_fraction(points, prims):
    _, _, ties = ref.brute_values(points, prims)
    return float((ties >= 2).mean())


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
HAND = [  # vert (0,0,0), e1 (1,0,0), e2 (0,1,0): p, dist2, (u, v), region
    ((0.25, 0.25, 1.0), 1.0, (0.25, 0.25), 0),
    ((-1.0, -1.0, 0.0), 2.0, (0.0, 0.0), 1),
    ((2.0, -1.0, 0.0), 2.0, (1.0, 0.0), 2),
    ((-1.0, 2.0, 0.0), 2.0, (0.0, 1.0), 3),
    ((0.5, -2.0, 0.0), 4.0, (0.5, 0.0), 4),
    ((-2.0, 0.5, 0.0), 4.0, (0.0, 0.5), 5),
    ((1.0, 1.0, 0.0), 0.5, (0.5, 0.5), 6),
]


def test_hand_cases_one_per_region():
    """exactly representable numbers: every region of Ericson's test, a degenerate triangle (e2 = 2 e1) and a zero triangle"""
    for p, d2, uv, region in HAND:
        val, u, v, reg, c = ref.pair_value(np.array(p, F), np.zeros(3, F), np.array([1, 0, 0], F), np.array([0, 1, 0], F))
        assert (float(val), (float(u), float(v)), int(reg)) == (d2, uv, region), p
        assert np.array_equal(c, np.array([uv[0], uv[1], 0.0], F)), p
    # e2 = 2 e1: the segment from (0,0,0) to (2,0,0); the point above its middle
    val, u, v, reg, c = ref.pair_value(np.array([1.0, 0.0, 3.0], F), np.zeros(3, F), np.array([1, 0, 0], F), np.array([2, 0, 0], F))
    assert np.isfinite(val) and float(val) >= 9.0 and 0 <= float(u) <= 1 and 0 <= float(v) <= 1 - float(u)
    assert float(val) == float(np.sum((np.array([1.0, 0.0, 3.0]) - c.astype(np.float64)) ** 2))
    # the zero triangle: its one point
    val, u, v, reg, c = ref.pair_value(np.array([1.0, 2.0, 2.0], F), np.array([0, 0, 0], F), np.zeros(3, F), np.zeros(3, F))
    assert (float(val), float(u), float(v), int(reg)) == (9.0, 0.0, 0.0, 1) and np.array_equal(c, np.zeros(3, F))
    # the argmin: the lowest index of equal values, strict bound, invalid input
    from tyrant_amd import scenes

    tri = scenes.make_triangles(np.array([[0, 0, 0]] * 3, F), np.array([[1, 0, 0]] * 3, F), np.array([[0, 1, 0]] * 3, F))
    tri["vert"][0] = (0, 0, 5)
    pts = np.array([[0.25, 0.25, 1.0]] * 5 + [[np.nan, 0, 0]], F)
    md = np.array([np.inf, 1.0, 1.5, -1.0, np.nan, 9.0], F)
    d2, prim, uv, reg, pt = ref.nearest(pts, tri, md)
    assert prim.tolist() == [1, -1, 1, -1, -1, -1]
    assert np.array_equal(bits(d2), bits(np.array([1.0, 1.0, 1.0, np.inf, np.inf, np.inf], F)))
    assert np.array_equal(bits(pt[1]), bits(pts[1])) and np.array_equal(bits(pt[5]), bits(pts[5])) and not uv[[1, 3, 4, 5]].any()


def _pair_families(rng, n):
    """(name, p, vert, e1, e2) of seeded pairs: soup, large triangles, an offset of 4096, slivers"""
    def soup(edge, spread, off=0.0):
        vert = (rng.uniform(-50, 50, (n, 3)) + off).astype(F)
        e1, e2 = (rng.uniform(-edge, edge, (n, 3)).astype(F) for _ in range(2))
        p = (vert + rng.normal(size=(n, 3)) * spread).astype(F)
        return p, vert, e1, e2

    yield ("soup",) + soup(1.5, 3.0)
    yield ("large",) + soup(200.0, 50.0)
    yield ("offset",) + soup(1.5, 3.0, off=4096.0)
    p, vert, e1, _ = soup(1.5, 1.0)
    perp = np.cross(e1.astype(np.float64), rng.normal(size=(n, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    thin = 10.0 ** rng.uniform(-6, -2, (n, 1))
    e2 = (rng.uniform(-1.5, 1.5, (n, 1)) * e1 + thin * np.linalg.norm(e1, axis=1, keepdims=True) * perp).astype(F)
    yield "slivers", p, vert, e1, e2


def test_value_never_undercuts_the_true_distance_by_more_than_rounding():
    """F >= true squared distance - 16 * 2^-24 * S^2 with S^2 = max(|ap|^2, |e1|^2, |e2|^2): the cap the pruning slack of
    hip/nearest.hip relies on (a property of the definition: 5.7 was measured on 10 M pairs)"""
    rng = np.random.default_rng(5)
    worst = {}
    for name, p, vert, e1, e2 in _pair_families(rng, 100000):
        val = ref.pair_value(p, vert, e1, e2)[0].astype(np.float64)
        true = ref.true_dist2(p, vert, e1, e2)
        ap = p.astype(np.float64) - vert
        S2 = np.maximum(np.maximum((ap * ap).sum(1), (e1.astype(np.float64) ** 2).sum(1)), (e2.astype(np.float64) ** 2).sum(1))
        assert np.isfinite(val).all(), name
        worst[name] = float(((true - val) / (2.0 ** -24 * S2)).max())
    print("undercut in units of 2^-24 S^2:", worst)
    assert max(worst.values()) <= 16.0, worst


def test_pruning_key_never_passes_the_value_of_a_triangle_in_the_box():
    """hip/nearest.hip skips a box when lb2 - (kSlackFar2 * far2 + kSlackCoord * max|p_k| * farInf) > best.  On a triangle's own
    box (tyr_triangle_bboxes' rule: vert, fl(vert + e1), fl(vert + e2)) that key must not exceed the triangle's value, for scenes
    at the origin and moved by 4096 and 65536, far points and points within 1e-3 of the triangle; every larger box has a smaller
    lb2 and a larger slack.  The slack's derivation (DESIGN.md "Closest-point queries") leaves 3.4x room; at least 2x is asserted.
    (The far2 term alone fails here by two orders of magnitude on the moved scenes: the boxes hold rounded sums.)"""
    src = open(os.path.join(ROOT, "tyrant_amd", "csrc", "hip", "nearest.hip")).read()
    k_far2 = float(re.search(r"kSlackFar2 = ([0-9.]+)f \* kUlpHalf", src).group(1))
    k_coord = float(re.search(r"kSlackCoord = ([0-9.]+)f \* kUlpHalf", src).group(1))
    u = F(2.0 ** -24)
    rng = np.random.default_rng(6)
    worst = {}
    for off in (0.0, 4096.0, 65536.0):
        for name, p, vert, e1, e2 in _pair_families(rng, 50000):
            vert, p = (vert + F(off)).astype(F), (p + F(off)).astype(F)
            close = (vert + F(0.3) * e1 + F(0.3) * e2 + rng.normal(size=p.shape) * 1e-3).astype(F)
            for pts in (p, close):
                val = ref.pair_value(pts, vert, e1, e2)[0].astype(np.float64)
                b, c = (vert + e1).astype(F), (vert + e2).astype(F)
                lo, hi = np.minimum(np.minimum(vert, b), c), np.maximum(np.maximum(vert, b), c)
                al, ah = (lo - pts).astype(F), (pts - hi).astype(F)
                d, f = np.maximum(np.maximum(al, ah), F(0)), np.maximum(np.abs(al), np.abs(ah))
                lb2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
                far2 = ((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]).astype(F)
                c1 = (F(k_coord) * u * np.abs(pts).max(axis=1)).astype(F)
                slack = ((F(k_far2) * u * far2).astype(F) + (c1 * f.max(axis=1)).astype(F)).astype(F)
                key = (lb2 - slack).astype(F)
                assert (key <= val).all(), (off, name)
                worst[(off, name)] = max(worst.get((off, name), 0.0), float(((lb2 - val) / slack).max()))
    print("needed slack / slack:", worst)
    assert max(worst.values()) <= 0.5, worst


def test_fixtures_reach_what_they_are_for():
    """the lattice has points with several triangles at a bit-equal minimal value, the duplicated scene only such points, and
    the lattice's tree needs more stack than the 12 LDS entries"""
    from tyrant_amd import binding

    nodes, prims, grid, _ = lattice(32, 21)
    frac = tie_fraction(grid, prims)
    print("lattice(32): fraction of the grid points with a tie", frac)
    assert frac >= 0.5
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    nodes, prims, pts, _ = duplicated(22, 2048)
    _, _, ties = ref.brute_values(pts, prims)
    assert (ties >= 2).all()
    nodes, prims = build(stack40())
    assert nodes["primitiveCount"].max() == 40  # an over-long leaf: synthetic records


def test_nearest_kernel_keeps_registers_and_lds_in_budget():
    """no vector spills; scratch no larger than the LdsStack's private spill arrays (52 entries of 8 bytes, plus the frame's
    alignment); occupancy and LDS (24,576 + 7,168 bytes) that admit the five blocks per CU the launch bounds plan for"""
    assert_kernel_budget("nearest", "k_query_nearest", 1, (64 - 12) * 8 + 16, 24576 + 7168)


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_nearest", "tyr_nearest_out", hip.NearestOut, 5)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
NAMES = ("dist2", "prim", "uv", "region", "point")


def ask(g, points, max_dist=None, **kw):
    return tuple(x.cpu().numpy() for x in g.query_nearest(points, max_dist, **kw))


same = functools.partial(same_outputs, NAMES)


def check(g, prims, points, max_dist=None, what=""):
    got = ask(g, points, max_dist)
    want = ref.nearest(points, prims, max_dist)
    same(got, want, what)
    return got, want


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lattice_and_ties(hip):
    """heightfield(32): points above every grid vertex (most of them equally near to several triangles) and seeded points"""
    nodes, prims, grid, rand = lattice(32, 21)
    g = renderer(hip, nodes, prims)
    (d2, prim, uv, region, _), _ = check(g, prims, np.concatenate([grid, rand]), what="lattice")
    assert (prim >= 0).all() and len(np.unique(region)) >= 4
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_exact_ties_resolve_to_the_lower_index(hip):
    """a scene concatenated with itself: every winner is the lower of the two copies' build-order indices; and 40 identical
    triangles (an over-long leaf behind synthetic records), alone and next to the Cornell box"""
    from tyrant_amd import scenes

    nodes, prims, pts, twin = duplicated(22, 2048)
    g = renderer(hip, nodes, prims)
    (_, prim, _, _, _), _ = check(g, prims, pts, what="duplicated")
    assert (prim < twin[prim]).all()
    for tris in (stack40(), np.concatenate([scenes.cornell_box().triangles, stack40()])):
        nodes, prims = build(tris)
        g.upload(nodes, prims)
        pts = box_points(np.random.default_rng(23), prims, 1500)
        (_, prim, _, _, _), _ = check(g, prims, pts, what="stack40")
        stack = np.nonzero((np.ascontiguousarray(prims).view(np.uint8).reshape(len(prims), -1) == np.ascontiguousarray(stack40()[:1]).view(np.uint8)).all(axis=1))[0]
        on_stack = np.isin(prim, stack)
        assert stack.size == 40 and on_stack.any() and (prim[on_stack] == stack.min()).all()  # the first of the identical records
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slivers", [False, True])
def test_scale_and_slack(hip, slivers):
    """a soup moved by (4096, -4096, 8192), without and with slivers: points within 1e-3 of the surface and far from it"""
    nodes, prims = offset_soup(slivers)
    rng = np.random.default_rng(24)
    pts = np.concatenate([surface_points(rng, prims, 2048, 1e-3), box_points(rng, prims, 768), (box_points(rng, prims, 256) - OFFSET * F(0.5)).astype(F)])
    g = renderer(hip, nodes, prims)
    (d2, _, _, _, _), _ = check(g, prims, pts, what=f"offset soup, slivers={slivers}")
    assert (d2[:2048] < 1.0).all()
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_bounds_hostile_input_and_batch_sizes(hip):
    """max_dist of 0, exactly the distance (strict <: a miss), +inf, NaN, negative; NaN / infinite points; n = 0 .. 4097 and
    400,003; a scene without triangles; every combination of the optional outputs"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    g = renderer(hip, nodes, prims)
    rng = np.random.default_rng(25)
    n = 400003
    pts = np.stack([rng.uniform(-60, 60, n), rng.uniform(-60, 60, n), rng.uniform(-10, 110, n)], axis=1).astype(F)
    pts[:4096] = np.round(pts[:4096])  # whole numbers: distances to the axis-aligned walls whose squares are exact
    free = ref.nearest(pts[:4096], prims)
    same(ask(g, pts[:4096]), free, "cornell, unbounded")
    root = np.sqrt(free[0]).astype(F)
    exact = np.nonzero(((root * root).astype(F) == free[0]) & (free[0] > 0))[0]
    assert exact.size > 1000
    md = (rng.random(n) * 60).astype(F)
    md[exact[0::2]] = root[exact[0::2]]  # exactly the distance: a miss
    above = np.nextafter(root[exact[1::2]], F(np.inf))
    for _ in range(4):  # the next bound whose square is above the distance's
        above = np.where((above * above).astype(F) > free[0][exact[1::2]], above, np.nextafter(above, F(np.inf)))
    md[exact[1::2]] = above
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
    want = ref.nearest(pts, prims, md)
    assert (want[1][exact[0::2]] == -1).all() and (want[1][exact[1::2]] >= 0).all()
    assert np.isinf(want[0][hostile]).all() and np.isinf(want[0][kind == 2]).all() and np.isinf(want[0][kind == 3]).all()
    got = ask(g, pts, md)
    same(got, want, "cornell, bounded")
    for m in (0, 1, 63, 64, 65, 4097):  # every prefix answers as the whole batch did
        part = ask(g, pts[:m], md[:m])
        same(part, tuple(a[:m] for a in want), f"n = {m}")
    # optional outputs NULL, in every combination, through the C call; the arrays not passed stay untouched
    m = 1000
    tp, tm = torch.from_numpy(pts[:m]).cuda(), torch.from_numpy(md[:m]).cuda()
    P = C.c_void_p
    for use in itertools.product((False, True), repeat=3):
        outs = [torch.full((m,), 7, dtype=torch.float32).cuda(), torch.full((m,), 7, dtype=torch.int32).cuda(), torch.full((m, 2), 7, dtype=torch.float32).cuda(),
                torch.full((m,), 7, dtype=torch.uint8).cuda(), torch.full((m, 3), 7, dtype=torch.float32).cuda()]
        torch.cuda.synchronize()
        ptrs = [outs[0].data_ptr(), outs[1].data_ptr()] + [outs[2 + k].data_ptr() if use[k] else None for k in range(3)]
        out = hip.NearestOut(*ptrs)
        assert hip.lib().tyr_query_nearest(g.h, m, P(tp.data_ptr()), P(tm.data_ptr()), 0, C.byref(out), None) == 0
        assert g.query_error() == 0
        res = [o.cpu().numpy() for o in outs]
        used = (True, True) + use
        same_outputs([nm for nm, u in zip(NAMES, used) if u], [r for r, u in zip(res, used) if u], [w[:m] for w, u in zip(want, used) if u], f"outputs {use}")
        assert all((r == 7).all() for r, u in zip(res, used) if not u), use
    # a scene without triangles: every point a miss
    g.upload(*no_triangles())
    same(ask(g, pts[:5000], md[:5000]), ref.nearest(pts[:5000], prims[:0], md[:5000]), "empty scene")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_nearest_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with closest-point queries between its tyr_render calls: the same accumulation
    buffer and counters as without them"""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(-40, 40, 20000), rng.uniform(-40, 40, 20000), rng.uniform(5, 80, 20000)], axis=1).astype(F)
    want = ref.nearest(pts, prims)

    def between(g):
        same(ask(g, pts), want, "between two renders")
        ask(g, pts, np.full(20000, 5.0, F))

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the answers to the refitted scene's; a torch side stream works; bad arguments are
    refused before any launch; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(24))
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    rng = np.random.default_rng(26)
    pts = box_points(rng, prims, 3000)
    check(g, prims, pts, what="before the refit")
    moved = deformed(prims, 4.0)
    g.refit(moved)
    got, want = check(g, moved, pts, what="after the refit")
    assert not np.array_equal(want[1], ref.nearest(pts, prims)[1])
    # a side stream, device tensors taken in place
    tp, tm = torch.from_numpy(pts).cuda(), torch.full((3000,), 6.0).cuda()
    res = on_side_stream(lambda side: g.query_nearest(tp, tm, stream=side))
    same(tuple(x.cpu().numpy() for x in res), ref.nearest(pts, moved, np.full(3000, 6.0, F)), "side stream")

    L, h, P = hip.lib(), g.h, C.c_void_p
    d2, prim = res[0], res[1]
    before = prim.cpu().numpy().copy()
    ok = hip.NearestOut(d2.data_ptr(), prim.data_ptr(), None, None, None)
    pp = P(tp.data_ptr())
    inv = hip.TYR_ERR_INVALID
    assert L.tyr_query_nearest(None, 4, pp, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_nearest(h, 4, None, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_nearest(h, 4, pp, None, 0, None, None) == inv
    assert L.tyr_query_nearest(h, 4, pp, None, 0, C.byref(hip.NearestOut(None, prim.data_ptr(), None, None, None)), None) == inv
    assert L.tyr_query_nearest(h, 4, pp, None, 0, C.byref(hip.NearestOut(d2.data_ptr(), None, None, None, None)), None) == inv
    assert L.tyr_query_nearest(h, 4, pp, None, 1, C.byref(ok), None) == inv  # flags must be 0
    assert L.tyr_query_nearest(h, 1 << 31, pp, None, 0, C.byref(ok), None) == inv
    assert L.tyr_query_nearest(h, 0, None, None, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_nearest(empty.h, 4, pp, None, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_nearest(tp.double())
    with pytest.raises(ValueError):
        g.query_nearest(tp[:, :2].contiguous())
    with pytest.raises(ValueError):
        g.query_nearest(tp, tm[:5])
    assert np.array_equal(prim.cpu().numpy(), before)  # the refused calls wrote nothing
    assert g.query_error() == 0
    g.close()


def c3_points(prims):
    rng = np.random.default_rng(27)
    return np.concatenate([box_points(rng, prims, 2048), surface_points(rng, prims, 2048, 0.5)])


def c3_answers(pts, prims):
    """brute force over the million triangles for 4096 points is about 4 G pair evaluations -- a quarter of an hour of numpy.
    Its (dist2, prim) are recorded in tests/golden/nearest_c3.npz with a digest of the points and triangles they belong to
    (TYR_RECORD_NEAREST_C3=1 computes them again and rewrites the file); every run recomputes a seeded sample of the points
    by brute force and all the winners' values from the restatement."""
    import hashlib

    digest = hashlib.sha256(np.ascontiguousarray(pts).tobytes() + np.ascontiguousarray(prims).tobytes()).hexdigest()
    if os.environ.get("TYR_RECORD_NEAREST_C3") == "1":
        best, arg, _ = ref.brute_values(pts, prims)
        np.savez_compressed(C3_ANSWERS, digest=np.array(digest), dist2=best, prim=arg.astype(np.int32))
    z = np.load(C3_ANSWERS)
    assert str(z["digest"]) == digest, "the recorded answers belong to other points or triangles"
    return z["dist2"], z["prim"]


@pytest.mark.gpu
def test_c3_tree(hip):
    """one pass on C3's 1 M-triangle tree: 4096 points, uniform in the inflated root box and within 0.5 of the surface"""
    sc, nodes, prims = built_scene("mesh706")
    pts = c3_points(prims)
    best, arg = c3_answers(pts, prims)
    live = np.random.default_rng(28).choice(len(pts), 8, replace=False)
    lb, la, _ = ref.brute_values(pts[live], prims)
    assert np.array_equal(bits(lb), bits(best[live])) and np.array_equal(la, arg[live])
    vert, e1, e2 = ref.records(prims)
    val, u2, v2, reg, c = ref.pair_value(pts, vert[arg], e1[arg], e2[arg])
    assert np.array_equal(bits(val), bits(best))
    g = renderer(hip, nodes, prims)
    got = ask(g, pts)
    same(got, (val, arg.astype(np.int32), np.stack([u2, v2], axis=1), reg, c), "C3")
    assert g.query_error() == 0
    g.close()
