"""Batched multi-hit ray queries on the uploaded scene (tyr_query_hits, hip/hits.hip; Renderer.query_hits): how many surfaces a
segment goes through and the nearest max_hits of them in order -- include/tyr_c.h "Multi-hit queries", bit for bit against its
numpy restatement (tests/hits_ref.py), which is the only oracle: the definition is a set with no visit order in it.

CPU: the restatement by hand, its `count > 0` against the reference's own intersectSimple, what the fixtures are for, what the
compiler made of the kernel, the ABI.  GPU: exact ties and overflowing buffers at every max_hits, ray order and batch sizes, a
deep tree and a soup, the siblings' answers on the device, hostile input and optional outputs, isolation from the render,
streams, refit and argument checks."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import hits_ref as ref
from conftest import GOLDEN, bits
from query_support import (assert_kernel_budget, assert_query_abi, assert_render_undisturbed, build, deformed, no_triangles, on_side_stream, query_exists, renderer, stack40,
                           take, unit)
from query_support import same as same_outputs

F = np.float32
VERY_FAR = F(1e20)
NAMES = ("count", "t", "prim", "uv", "side", "back_count")
SOUP_EDGE = 16.0


_the_query_exists = query_exists("tyr_query_hits")  # nothing here means anything without the entry point


# ---- fixtures (numpy only; made once, never changed) ------------------------------------------------------------------
def quads48():
    """48 squares [-20, 20] x [10, 50] in the planes y = 0, 0.5, .. 23.5, two triangles each, facing -y"""
    from tyrant_amd import scenes

    y = 0.5 * np.arange(48)
    p = lambda x, z: np.stack([np.full(48, x), y, np.full(48, z)], axis=1)
    p0, p1, p2, p3 = p(-20.0, 10.0), p(20.0, 10.0), p(20.0, 50.0), p(-20.0, 50.0)
    return np.concatenate([scenes.make_triangles(p0, p1, p2), scenes.make_triangles(p0, p2, p3)])


def _axial_and_oblique(rng, xs, zs, n_oblique, target_lo, target_hi):
    """rays along +y from y = -100 and along -y from y = +100 through every (x, z) of the grid (box faces, triangle edges and
    corners among them), and oblique rays from both sides at seeded points of the target rectangle; tmax: VERY_FAR, +inf, and
    lengths that end inside, in front of and behind the geometry"""
    X, Z = np.meshgrid(np.asarray(xs, np.float64), np.asarray(zs, np.float64), indexing="ij")
    g = X.size
    o = np.concatenate([np.stack([X.reshape(-1), np.full(g, -100.0), Z.reshape(-1)], axis=1), np.stack([X.reshape(-1), np.full(g, 100.0), Z.reshape(-1)], axis=1)])
    d = np.concatenate([np.tile([0.0, 1.0, 0.0], (g, 1)), np.tile([0.0, -1.0, 0.0], (g, 1))])
    tgt = np.stack([rng.uniform(target_lo[0], target_hi[0], n_oblique), rng.uniform(0.0, 12.0, n_oblique), rng.uniform(target_lo[1], target_hi[1], n_oblique)], axis=1)
    oo = np.stack([rng.uniform(-60, 60, n_oblique), np.where(rng.random(n_oblique) < 0.5, -100.0, 100.0) + rng.uniform(-20, 20, n_oblique), rng.uniform(-10, 90, n_oblique)], axis=1)
    o = np.concatenate([o, oo]).astype(F)
    d = np.concatenate([d, unit(tgt - oo)]).astype(F)
    n = o.shape[0]
    kind = rng.integers(0, 6, n)
    tmax = np.select([kind == 0, kind == 1, kind == 2], [F(np.inf), (100.0 + rng.uniform(-2, 26, n)).astype(F), (rng.uniform(0, 250, n)).astype(F)], VERY_FAR).astype(F)
    return o, d, tmax


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(nodes, prims, origins, directions, tmax)"""
    from tyrant_amd import scenes

    if name == "stack40":
        nodes, prims = build(stack40())
        o, d, tmax = _axial_and_oblique(np.random.default_rng(51), np.arange(-35, 36, 5), np.arange(5, 76, 5), 300, (-30, 10), (30, 70))
    elif name == "quads48":
        nodes, prims = build(quads48())
        o, d, tmax = _axial_and_oblique(np.random.default_rng(52), np.arange(-25, 26, 5), np.arange(5, 56, 5), 400, (-20, 10), (20, 50))
    elif name == "layered":
        import layered_scenes as ls

        sc, nodes, prims = ls.built_layered("layered_mesh24")
        o, d = ls.ray_set(sc, nodes, 2048, 53)
        tmax = np.where(np.random.default_rng(53).random(2048) < 0.5, VERY_FAR, F(60.0)).astype(F)
    elif name in ("heightfield32", "heightfield128"):
        # grazing: from outside the field's -x edge, almost level, at the height the surface undulates about
        cells, n, seed = (32, 1024, 54) if name == "heightfield32" else (128, 4096, 55)
        nodes, prims = build(scenes.heightfield(cells))
        rng = np.random.default_rng(seed)
        o = np.stack([np.full(n, -60.0), rng.uniform(-45, 45, n), rng.uniform(21.0, 23.0, n)], axis=1).astype(F)
        d = unit(np.stack([np.ones(n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.004, 0.004, n)], axis=1))
        tmax = np.full(n, VERY_FAR, F)
    elif name == "soup":
        # (random_soup's default edge of 1.5 gives a ray through the box 0.1 triangles on average: no seed makes a quarter of
        # the rays meet more than four.  The same generator with edges up to SOUP_EDGE does.)
        nodes, prims = build(scenes.random_soup(2000, edge=SOUP_EDGE))
        rng = np.random.default_rng(56)
        lo, hi = nodes[0]["bounds"][0].astype(np.float64), nodes[0]["bounds"][1].astype(np.float64)
        a, b = lo + (hi - lo) * rng.random((4096, 3)), lo + (hi - lo) * rng.random((4096, 3))
        d = unit(b - a)
        o = (a - 200.0 * d).astype(F)
        tmax = np.where(rng.random(4096) < 0.5, VERY_FAR, rng.uniform(150, 400, 4096)).astype(F)
    else:
        raise KeyError(name)
    for a in (nodes, prims, o, d, tmax):
        a.setflags(write=False)
    return nodes, prims, o, d, tmax


@functools.lru_cache(maxsize=None)
def reference(name, two_sided):
    """the restatement's hit lists of a fixture's rays, computed once per process"""
    nodes, prims, o, d, tmax = fixture(name)
    return ref.Hits(o, d, nodes, prims, tmax, two_sided)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
def test_hand_cases():
    """one triangle (0,0,0), (1,0,0), (0,1,0), facing +z, in exactly representable numbers: front and back with and without
    the flag, t inside 1e-3 of the origin and of tmax, tmax of 0, negative, NaN and +inf, rays along the box's faces and the
    triangle's edges, and a ray that is none"""
    from tyrant_amd import scenes

    nodes, prims = build(scenes.make_triangles(np.array([[0, 0, 0]], F), np.array([[1, 0, 0]], F), np.array([[0, 1, 0]], F)))
    down, up = (0, 0, -1), (0, 0, 1)
    nan, inf = np.nan, np.inf
    cases = [  # origin, direction, tmax -> count one-sided, count two-sided, back_count two-sided, t of the hit
        ((0.25, 0.25, 1.0), down, 1e20, 1, 1, 0, 1.0),          # the front
        ((0.25, 0.25, -1.0), up, 1e20, 0, 1, 1, 1.0),           # the back: culled without the flag
        ((0.25, 0.25, 0.0005), down, 1e20, 0, 0, 0, None),      # t <= 1e-3
        ((0.25, 0.25, 0.0015), down, 1e20, 1, 1, 0, 0.0015),
        ((0.25, 0.25, 1.0), down, 1.0005, 0, 0, 0, None),       # tmax - t <= 1e-3
        ((0.25, 0.25, 1.0), down, 1.0015, 1, 1, 0, 1.0),
        ((0.25, 0.25, 1.0), down, 0.0, 0, 0, 0, None),
        ((0.25, 0.25, 1.0), down, -5.0, 0, 0, 0, None),
        ((0.25, 0.25, 1.0), down, nan, 0, 0, 0, None),
        ((0.25, 0.25, 1.0), down, inf, 1, 1, 0, 1.0),
        # along the box's faces 1 / d is infinite and (bound - origin) zero: Bbox.h:38-62 computes 0 * inf = NaN.  In x it becomes
        # tMin or tMax and fails the last comparison; in y it only loses the comparisons that would have taken it.
        ((0.0, 0.5, 1.0), down, 1e20, 0, 0, 0, None),           # the edge u = 0 in the box's face x = 0: the box is missed
        ((0.5, 0.0, 1.0), down, 1e20, 1, 1, 0, 1.0),            # the edge v = 0 in the box's face y = 0: entered
        ((0.5, 0.5, 1.0), down, 1e20, 1, 1, 0, 1.0),            # the edge u + v = 1, inside the box
        ((1.0, 0.0, 1.0), down, 1e20, 0, 0, 0, None),           # a corner: the face x = 1
        ((0.5, 0.25, 1.0), (0, 0, -2), 1e20, 1, 1, 0, 0.5),     # a direction that is no unit vector: t in its units
        ((1.0, 1.0, 1.0), down, 1e20, 0, 0, 0, None),           # the box's corner outside the triangle
        ((-1.0, 0.25, 0.0), (1, 0, 0), 1e20, 0, 0, 0, None),    # in the triangle's plane: det = 0
        ((0.25, 0.25, 1.0), (0, 0, 0), 1e20, 0, 0, 0, None),    # no direction
        ((nan, 0.25, 1.0), down, 1e20, 0, 0, 0, None),          # not a ray
        ((0.25, 0.25, 1.0), (0, inf, -1), 1e20, 0, 0, 0, None),
    ]
    o = np.array([c[0] for c in cases], F)
    d = np.array([c[1] for c in cases], F)
    tmax = np.array([c[2] for c in cases], F)
    for two in (False, True):
        count, t, prim, uv, side, back = ref.hits(o, d, nodes, prims, tmax, 2, two)
        for i, (oo, dd, tm, c1, c2, b2, th) in enumerate(cases):
            want = c2 if two else c1
            assert count[i] == want and back[i] == (b2 if two else 0), (i, two)
            assert np.array_equal(bits(t[i, want:]), bits(np.full(2 - want, tm, F))) and (prim[i, want:] == -1).all(), (i, two)
            assert not uv[i, want:].any() and not side[i, want:].any(), (i, two)
            if want:
                assert float(t[i, 0]) == float(F(th)) and prim[i, 0] == 0 and side[i, 0] == (1 if b2 and two else 0), (i, two)
                assert (float(uv[i, 0, 0]), float(uv[i, 0, 1])) == (float(F(oo[0])), float(F(oo[1]))), (i, two)
    # the order: equal t by index, and count beyond max_hits
    tri = scenes.make_triangles(np.array([[0, 0, 0], [0, 0, 0.5], [0, 0, 0], [0, 0, 0.25]], F), np.array([[1, 0, 0], [1, 0, 0.5], [1, 0, 0], [1, 0, 0.25]], F), np.array([[0, 1, 0], [0, 1, 0.5], [0, 1, 0], [0, 1, 0.25]], F))
    nodes, prims = build(tri)
    z = prims["vert"][:, 2]
    order = np.lexsort((np.arange(4), -z))  # from z = 1: the highest plane first, the two at z = 0 by index
    for k in (1, 3, 4, 6):
        count, t, prim, uv, side, back = ref.hits(np.array([[0.25, 0.25, 1.0]], F), np.array([down], F), nodes, prims, None, k, False)
        assert count[0] == 4 and prim[0, :min(k, 4)].tolist() == order[:k].tolist() and (prim[0, 4:] == -1).all()
        assert t[0, :min(k, 4)].tolist() == (1.0 - z[order[:k]]).tolist() and np.array_equal(bits(t[0, 4:]), bits(np.full(max(k - 4, 0), VERY_FAR, F)))


def _golden(name):
    from tyrant_amd import scenes

    z = np.load(os.path.join(GOLDEN, f"ref_traverse_{name}.npz"))
    nodes = np.ascontiguousarray(z["nodes"]).view(scenes.NODE_DTYPE).reshape(-1)
    prims = np.ascontiguousarray(z["prims"]).view(scenes.TRIANGLE_DTYPE).reshape(-1)
    return nodes, prims, z["origin"].astype(F), z["direction"].astype(F), z["closest"].astype(F), z["anyhit"].astype(bool)


def test_count_is_pinned_to_the_references_any_hit(orc):
    """over the reference's committed ray sets and every fixture of this module: the restatement's one-sided `count > 0` is
    intersectSimple(ray, tmax) -- the reference's own bvh.h where its harness is built (and its recorded answers for the
    committed sets everywhere), and the oracle's restatement of it -- exactly.  Prints how many pairs that pass the triangle
    test and the accept rule the reach filter removed (DESIGN.md "Multi-hit queries" reports it)."""
    from tyrant_amd import scenes

    R = orc.ref()
    f = orc.lib().orc_bvh_intersect_simple
    tested = removed = 0
    sets = [("golden " + n,) + _golden(n) for n in ("cornell36", "soup2k", "mesh32", "layered")]
    sets += [(n,) + fixture(n) + (None,) for n in ("stack40", "quads48", "layered", "heightfield32", "soup")]
    for name, nodes, prims, o, d, tmax, recorded in sets:
        ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
        h = reference(name, False) if recorded is None else ref.Hits(o, d, nodes, prims, tmax, False)
        tested, removed = tested + h.tested, removed + h.removed
        got = h.count > 0
        n = o.shape[0]
        s = np.zeros(n, dtype=scenes.SHADOW_DTYPE)
        s["origin"], s["direction"], s["closestDistance"] = o, d, tmax
        nn, pp = np.ascontiguousarray(nodes), np.ascontiguousarray(prims)
        want = np.array([f(nn.ctypes.data, pp.ctypes.data, s.ctypes.data + i * s.dtype.itemsize, float(tmax[i]), None) if ok[i] else 0 for i in range(n)]) != 0
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8].tolist())
        if recorded is not None:
            assert np.array_equal(got, recorded), name
        if R is not None:
            hit = np.zeros(n, dtype=np.int32)
            R.ref_bvh_intersect_simple(nn.ctypes.data, pp.ctypes.data, s.ctypes.data, n, hit.ctypes.data_as(C.POINTER(C.c_int)))
            assert np.array_equal(got[ok], hit[ok] != 0), name
        assert got.any() and (name == "heightfield32" or not got.all()), name  # (every grazing ray meets the field)
    print(f"reach filter: removed {removed} of {tested} pairs that pass the triangle test and the accept rule")


def test_fixtures_reach_what_they_are_for():
    """ties, overflow at every max_hits, hits closer together than the accept rule's 1e-3, a tree deeper than the LDS stack, and
    rays with more hits than a small buffer holds -- by the restatement alone"""
    from tyrant_amd import binding

    # 40 identical triangles in one leaf: 40 bit-equal t on every ray through them
    nodes, prims, o, d, tmax = fixture("stack40")
    assert nodes["primitiveCount"].max() == 40
    h = reference("stack40", True)
    through = h.count > 0
    assert through.sum() > 100 and (h.count[through] == 40).all()
    t = h.answer(32)[1][through]
    assert (bits(t) == bits(t[:, :1])).all() and (h.answer(32)[2][through] == np.arange(32)).all()
    assert (reference("stack40", False).count == 40).sum() > 50
    # 48 quads 0.5 apart: more hits than TYR_QUERY_HITS_MAX on the axial rays that go all the way through
    nodes, prims, o, d, tmax = fixture("quads48")
    axial = (d[:, 0] == 0) & (d[:, 2] == 0) & (np.abs(o[:, 0]) < 20) & (o[:, 2] > 10) & (o[:, 2] < 50) & (tmax > 200)  # (inside the squares)
    assert axial.sum() > 50
    assert (reference("quads48", True).count[axial] > 32).all() and (reference("quads48", True).count[axial] >= 48).all()
    fwd = axial & (d[:, 1] > 0)
    assert (reference("quads48", False).count[fwd] > 32).all() and (reference("quads48", True).back_count[axial & ~fwd] >= 48).all()
    # layers less than 1e-3 apart: pairs of listed hits that peeling with closest-hit calls cannot separate
    h = reference("layered", True)
    same_ray = h.ray[1:] == h.ray[:-1]
    close = same_ray & ((h.t[1:] - h.t[:-1]) < F(1e-3))
    print("layered: pairs of neighbouring hits closer than 1e-3:", int(close.sum()), "of", int(same_ray.sum()))
    assert close.sum() > 1000
    # heightfield(32): a tree that needs more stack than the 12 LDS entries, grazing rays through several of its hills
    nodes, prims, o, d, tmax = fixture("heightfield32")
    assert binding.layout_probe(nodes, prims, want_pairs=False)["quad_max_stack"] > 12
    assert (reference("heightfield32", True).count >= 4).all()
    # the soup: at least a quarter of the rays have more hits than a buffer of four holds
    h = reference("soup", True)
    print("soup: fraction of the rays with count > 4:", float((h.count > 4).mean()), "two-sided,", float((reference("soup", False).count > 4).mean()), "one-sided")
    assert (h.count > 4).mean() >= 0.25 and h.count.max() > 16


def test_hits_kernels_keep_registers_and_lds_in_budget():
    """both instantiations: no vector spills; scratch no larger than the LdsStack's private spill arrays plus alignment -- so
    the k-buffer is not in scratch; occupancy and LDS that admit the five blocks per CU the launch bounds name"""
    assert_kernel_budget("hits", r"k_query_hitsILb[01]E", 2, (64 - 12) * 8 + 16)


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_hits", "tyr_hits_out", hip.HitsOut, 6, (r"TYR_QUERY_TWO_SIDED\s+2u", r"TYR_QUERY_HITS_MAX\s+32\b"))
    assert hip.TYR_QUERY_TWO_SIDED == 2 and hip.TYR_QUERY_HITS_MAX == 32


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, o, d, tmax=None, max_hits=4, two_sided=False, **kw):
    o, d, tmax = np.array(o), np.array(d), None if tmax is None else np.array(tmax)  # (the fixtures' arrays are read-only: torch wants its own)
    res = tuple(x.cpu().numpy() for x in g.query_hits(o, d, tmax, max_hits=max_hits, two_sided=two_sided, **kw))
    return (res[0].view(np.uint32),) + res[1:5] + (res[5].view(np.uint32),)


same = functools.partial(same_outputs, NAMES)


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stack40", "quads48"])
def test_ties_and_overflow(hip, name):
    """bit-equal t resolved by index and buffers that overflow, at max_hits 1, 2, 3, 8 and 32, one- and two-sided; the answer
    does not depend on the order of the rays or on the batch size"""
    nodes, prims, o, d, tmax = fixture(name)
    g = renderer(hip, nodes, prims)
    n = o.shape[0]
    for two in (False, True):
        h = reference(name, two)
        for k in (1, 2, 3, 8, 32):
            same(ask(g, o, d, tmax, k, two), h.answer(k), f"{name}, max_hits {k}, two_sided {two}")
        perm = np.random.default_rng(57).permutation(n)
        same(ask(g, o[perm], d[perm], tmax[perm], 3, two), take(h.answer(3), perm), f"{name} shuffled")
        idx = np.arange(4097) % n
        for m in (1, 63, 64, 65, 4097):
            for k in (2, 32):
                same(ask(g, o[idx[:m]], d[idx[:m]], tmax[idx[:m]], k, two), take(h.answer(k), idx[:m]), f"{name}, n = {m}, max_hits {k}")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["heightfield32", "soup", "layered"])
def test_deep_tree_soup_and_layers(hip, name):
    """grazing rays over a tree deeper than the LDS stack, a soup whose rays overflow a buffer of four, and layers closer
    together than 1e-3: max_hits 4 and 32, both sidedness settings; no query error"""
    nodes, prims, o, d, tmax = fixture(name)
    g = renderer(hip, nodes, prims)
    for two in (False, True):
        for k in (4, 32):
            same(ask(g, o, d, tmax, k, two), reference(name, two).answer(k), f"{name}, max_hits {k}, two_sided {two}")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_larger_tree_live(hip):
    """heightfield(128), 32,768 triangles: 4096 grazing rays, checked live by the restatement"""
    nodes, prims, o, d, tmax = fixture("heightfield128")
    g = renderer(hip, nodes, prims)
    h = ref.Hits(o, d, nodes, prims, tmax, True)
    assert (h.count >= 4).mean() > 0.9 and (h.count > 5).mean() > 0.5 and h.count.max() <= 32
    same(ask(g, o, d, tmax, 32, True), h.answer(32), "heightfield128, two-sided")
    same(ask(g, o, d, tmax, 5, True), h.answer(5), "heightfield128, two-sided, max_hits 5")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["soup", "layered", "quads48"])
def test_consistent_with_the_sibling_queries(hip, name):
    """on the device alone: `count > 0` is tyr_query_any's answer for the same rays and tmax, and the one-sided rows are the
    front-side subsequence of the two-sided rows wherever those hold every hit"""
    nodes, prims, o, d, tmax = fixture(name)
    g = renderer(hip, nodes, prims)
    c1, t1, p1, uv1, s1, b1 = ask(g, o, d, tmax, 32, False)
    c2, t2, p2, uv2, s2, b2 = ask(g, o, d, tmax, 32, True)
    occ = g.query_any(np.array(o), np.array(d), np.array(tmax)).cpu().numpy()
    assert np.array_equal(c1 > 0, occ) and 0 < occ.sum() < occ.size
    assert not s1.any() and not b1.any() and np.array_equal(c2 - b2, c1)
    whole = c2 <= 32
    assert whole.sum() > whole.size // 4
    for i in np.nonzero(whole)[0]:
        front = (p2[i] >= 0) & (s2[i] == 0)
        m = int(front.sum())
        assert m == c1[i] and np.array_equal(p1[i, :m], p2[i, front]) and np.array_equal(bits(t1[i, :m]), bits(t2[i, front])) and np.array_equal(bits(uv1[i, :m]), bits(uv2[i, front])), i
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_hostile_input_and_optional_outputs(hip):
    """NaN / infinite rays, zero directions, tmax of 0, negative, NaN, +inf and NULL, n = 0, a scene without triangles, and the
    optional outputs NULL in every combination (what is not passed stays untouched)"""
    import torch

    nodes, prims, o, d, tmax = fixture("quads48")
    rng = np.random.default_rng(58)
    n = o.shape[0]
    o, d, tmax = o.copy(), d.copy(), tmax.copy()
    kind = rng.integers(0, 12, n)
    bad = np.array([np.nan, np.inf, -np.inf], F)
    for i in np.nonzero(kind == 0)[0]:
        (o if rng.random() < 0.5 else d)[i, rng.integers(0, 3)] = bad[rng.integers(0, 3)]
    d[kind == 1] = 0.0
    tmax[kind == 2] = 0.0
    tmax[kind == 3] = -7.0
    tmax[kind == 4] = np.nan
    tmax[kind == 5] = np.inf
    g = renderer(hip, nodes, prims)
    for two in (False, True):
        want = ref.Hits(o, d, nodes, prims, tmax, two)
        assert (want.count[(kind <= 4)] == 0).all() and (want.count[kind == 5] > 0).any()
        same(ask(g, o, d, tmax, 6, two), want.answer(6), f"hostile, two_sided {two}")
        same(ask(g, o, d, None, 6, two), ref.Hits(o, d, nodes, prims, None, two).answer(6), f"tmax NULL, two_sided {two}")
    empty = ask(g, o[:0], d[:0], tmax[:0], 4, True)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 4) and empty[3].shape == (0, 4, 2)
    # optional outputs NULL, in every combination, through the C call
    m, k = 500, 5
    want = ref.Hits(o[:m], d[:m], nodes, prims, tmax[:m], True).answer(k)
    to, td, tt = torch.from_numpy(o[:m]).cuda(), torch.from_numpy(d[:m]).cuda(), torch.from_numpy(tmax[:m]).cuda()
    P = C.c_void_p
    for use in itertools.product((False, True), repeat=3):
        outs = [torch.full((m,), 7, dtype=torch.int32).cuda(), torch.full((m, k), 7, dtype=torch.float32).cuda(), torch.full((m, k), 7, dtype=torch.int32).cuda(),
                torch.full((m, k, 2), 7, dtype=torch.float32).cuda(), torch.full((m, k), 7, dtype=torch.uint8).cuda(), torch.full((m,), 7, dtype=torch.int32).cuda()]
        torch.cuda.synchronize()
        ptrs = [outs[j].data_ptr() for j in range(3)] + [outs[3 + j].data_ptr() if use[j] else None for j in range(3)]
        out = hip.HitsOut(*ptrs)
        assert hip.lib().tyr_query_hits(g.h, m, P(to.data_ptr()), P(td.data_ptr()), P(tt.data_ptr()), k, hip.TYR_QUERY_TWO_SIDED, C.byref(out), None) == 0
        assert g.query_error() == 0
        res = [x.cpu().numpy() for x in outs]
        res[0], res[5] = res[0].view(np.uint32), res[5].view(np.uint32)
        used = (True, True, True) + use
        for name, r, w, u in zip(NAMES, res, want, used):
            if u:
                same_outputs((name,), (r,), (w,), f"outputs {use}")
            else:
                assert (r == 7).all(), (use, name)
    # a scene without triangles: every ray a row of unused entries
    g.upload(*no_triangles())
    got = ask(g, o, d, tmax, 3, True)
    assert not got[0].any() and not got[5].any() and (got[2] == -1).all() and not got[3].any() and not got[4].any()
    assert np.array_equal(bits(got[1]), bits(np.repeat(tmax[:, None], 3, axis=1)))
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_hit_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with multi-hit queries between its tyr_render calls: the same accumulation buffer,
    counters and queues as without them"""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    rng = np.random.default_rng(59)
    n = 6000
    o = np.stack([rng.uniform(-40, 40, n), rng.uniform(-140, 40, n), rng.uniform(5, 80, n)], axis=1).astype(F)
    d = unit(rng.normal(size=(n, 3)))
    want = ref.Hits(o, d, nodes, prims, None, True)
    assert want.count.max() >= 3

    def between(g):
        same(ask(g, o, d, None, 4, True), want.answer(4), "between two renders")
        ask(g, o, d, np.full(n, 90.0, F), 32, False)

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the second to the refitted scene's answer; a torch side stream works; bad arguments
    are refused before any launch; tyr_query_error stays 0"""
    import torch

    from tyrant_amd import scenes

    nodes, prims, o, d, tmax = fixture("heightfield32")
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    same(ask(g, o, d, tmax, 8, True), reference("heightfield32", True).answer(8), "before the refit")
    moved = deformed(prims, 2.0)
    new_nodes = g.refit(moved, want_nodes=True)
    want = ref.Hits(o, d, new_nodes, moved, tmax, True)
    assert not np.array_equal(want.count, reference("heightfield32", True).count)
    same(ask(g, o, d, tmax, 8, True), want.answer(8), "after the refit")
    # a side stream, device tensors taken in place
    to, td, tt = torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(d)).cuda(), torch.from_numpy(np.array(tmax)).cuda()
    res = on_side_stream(lambda side: g.query_hits(to, td, tt, max_hits=8, two_sided=True, stream=side))
    res = tuple(x.cpu().numpy() for x in res)
    same((res[0].view(np.uint32),) + res[1:5] + (res[5].view(np.uint32),), want.answer(8), "side stream")

    L, h, P = hip.lib(), g.h, C.c_void_p
    n, k = 4, 8
    cnt, t, prim = (torch.full((n,), 7, dtype=torch.int32).cuda(), torch.full((n, k), 7, dtype=torch.float32).cuda(), torch.full((n, k), 7, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    ok = hip.HitsOut(cnt.data_ptr(), t.data_ptr(), prim.data_ptr(), None, None, None)
    po, pd = P(to.data_ptr()), P(td.data_ptr())
    inv = hip.TYR_ERR_INVALID
    assert L.tyr_query_hits(None, n, po, pd, None, k, 0, C.byref(ok), None) == inv
    assert L.tyr_query_hits(h, n, None, pd, None, k, 0, C.byref(ok), None) == inv
    assert L.tyr_query_hits(h, n, po, None, None, k, 0, C.byref(ok), None) == inv
    assert L.tyr_query_hits(h, n, po, pd, None, k, 0, None, None) == inv
    assert L.tyr_query_hits(h, n, po, pd, None, k, 0, C.byref(hip.HitsOut(None, t.data_ptr(), prim.data_ptr(), None, None, None)), None) == inv
    assert L.tyr_query_hits(h, n, po, pd, None, k, 0, C.byref(hip.HitsOut(cnt.data_ptr(), None, prim.data_ptr(), None, None, None)), None) == inv
    assert L.tyr_query_hits(h, n, po, pd, None, k, 0, C.byref(hip.HitsOut(cnt.data_ptr(), t.data_ptr(), None, None, None, None)), None) == inv
    assert L.tyr_query_hits(h, n, po, pd, None, 0, 0, C.byref(ok), None) == inv
    assert L.tyr_query_hits(h, n, po, pd, None, hip.TYR_QUERY_HITS_MAX + 1, 0, C.byref(ok), None) == inv
    assert L.tyr_query_hits(h, n, po, pd, None, k, hip.TYR_QUERY_SPHERES, C.byref(ok), None) == inv  # the sphere table is not part of it
    assert L.tyr_query_hits(h, n, po, pd, None, k, hip.TYR_QUERY_TWO_SIDED | 4, C.byref(ok), None) == inv
    assert L.tyr_query_hits(h, 1 << 31, po, pd, None, k, 0, C.byref(ok), None) == inv
    assert L.tyr_query_hits(h, 0, None, None, None, k, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_hits(empty.h, n, po, pd, None, k, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_hits(to.double(), td)
    with pytest.raises(ValueError):
        g.query_hits(to, td[:, :2].contiguous())
    with pytest.raises(ValueError):
        g.query_hits(to, td, tt[:5])
    with pytest.raises(ValueError):
        g.query_hits(to, td, max_hits=33)
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() == 7).all() and (t.cpu().numpy() == 7).all() and (prim.cpu().numpy() == 7).all()  # the refused calls wrote nothing
    assert L.tyr_query_hits(h, n, po, pd, None, k, hip.TYR_QUERY_TWO_SIDED, C.byref(ok), None) == 0
    assert g.query_error() == 0
    assert np.array_equal(cnt.cpu().numpy().view(np.uint32), ref.Hits(o[:n], d[:n], new_nodes, moved, None, True).count)
    g.close()
