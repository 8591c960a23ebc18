"""Batched winding-number queries on the uploaded scene (tyr_query_winding, hip/winding.hip; Renderer.query_winding) and the
moment tree behind them (tyr_scene_moments) -- include/tyr_c.h "Winding numbers", bit for bit against its numpy restatement
(tests/winding_ref.py), which in turn is held to the brute-force sum with numpy.arctan2.

CPU: hand cases, the definition against the truth (the figures of DESIGN.md's table are printed), atan2_det against math.atan2,
what the compiler made of the kernels, the ABI.  GPU: the moments through every upload path, w and terms by bits over accuracies
and batch sizes, the probe ops, independence of the batch, refit, isolation from the render and from a ctx without the flag,
two streams, hostile input."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest

import winding_ref as ref
from kernel_resources import kernel_resources
from query_support import assert_render_undisturbed, box, build, header_code, query_exists, renderer
from query_support import same as same_outputs

F = np.float32
D = np.float64
U = np.uint32
INF = float("inf")
WINDING = 128
REFIT = 64
CLOSED = ("nested", "torus", "sphere5")
ALL = ("nested", "torus", "sphere5", "heightfield32", "soup", "box", "one", "degenerate")
ACCURACIES = (0.0, 1.0, 2.0, 3.5, INF)
SIZES = (1, 63, 64, 65, 257, 2048)


_the_query_exists = query_exists("tyr_query_winding", "tyr_scene_moments")  # nothing here means anything without the entry points


# ---- fixtures (numpy only; made once, never changed) ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def icosphere(level):
    """unit vertices (float64) and outward-wound faces of an icosahedron subdivided `level` times: 20 * 4^level triangles"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
         (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, D) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    V, Fc = np.array(v), np.array(f)
    out = np.einsum("ij,ij->i", np.cross(V[Fc[:, 1]] - V[Fc[:, 0]], V[Fc[:, 2]] - V[Fc[:, 0]]), V[Fc].sum(axis=1)) > 0
    Fc[~out] = Fc[~out][:, [0, 2, 1]]
    return V, Fc


def sphere(level, radius, centre, inward=False):
    from tyrant_amd import scenes

    V, Fc = icosphere(level)
    P = V * radius + np.asarray(centre, D)
    a, b, c = P[Fc[:, 0]], P[Fc[:, 1]], P[Fc[:, 2]]
    return scenes.make_triangles(a, c, b) if inward else scenes.make_triangles(a, b, c)


def torus(nu=48, nv=24, R=20.0, r=7.0, centre=(0.0, 0.0, 30.0)):
    from tyrant_amd import scenes

    u, v = np.meshgrid(np.arange(nu + 1) % nu * (2 * np.pi / nu), np.arange(nv + 1) % nv * (2 * np.pi / nv), indexing="ij")
    P = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1) + np.asarray(centre, D)
    p00, p10, p11, p01 = (x.reshape(-1, 3) for x in (P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]))
    return scenes.make_triangles(np.concatenate([p00, p00]), np.concatenate([p10, p11]), np.concatenate([p11, p01]))  # e1 x e2 along du x dv: outward


def one_triangle():
    from tyrant_amd import scenes

    return scenes.make_triangles(np.array([[-8, -6, 20]], F), np.array([[12, -6, 20]], F), np.array([[-8, 10, 20]], F))


def triangles_of(name):
    from tyrant_amd import scenes

    if name == "nested":  # an outward shell and an inward one at 0.4 of its size, off-centre inside it: W = 0 / 1 / 0
        return np.concatenate([sphere(3, 20.0, (0, 0, 30)), sphere(3, 8.0, (4, -3, 33), inward=True)])
    if name == "torus":
        return torus()
    if name == "sphere5":
        return sphere(5, 25.0, (2, 1, 35))
    if name == "heightfield32":
        return scenes.heightfield(32)
    if name == "soup":
        return scenes.random_soup(2000)
    if name == "box":
        return box()
    if name == "one":
        return one_triangle()
    if name == "degenerate":  # the box and, apart from it, two triangles without area: a leaf whose S is 0
        z = scenes.make_triangles(np.array([[30, 30, 40], [31, 30, 40]], F), np.array([[31, 32, 43], [31, 30, 40]], F), np.array([[32, 34, 46], [32, 31, 41]], F))
        return np.concatenate([box(), z])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(nodes, prims, tree, points): 2048 points uniform in the root box grown by a quarter on each side, then points on a vertex,
    on an edge, in a face's plane and at two nodes' centres"""
    from tyrant_amd import scenes

    if name == "empty":
        nodes, prims, tree = np.zeros(0, dtype=scenes.NODE_DTYPE), np.zeros(0, dtype=scenes.TRIANGLE_DTYPE), None
        lo, hi = np.array([-10.0, -10.0, 0.0]), np.array([10.0, 10.0, 20.0])
        hand = np.zeros((0, 3), F)
    else:
        nodes, prims = build(triangles_of(name))
        tree = ref.Tree(nodes, prims)
        lo, hi = nodes[0]["bounds"][0].astype(D), nodes[0]["bounds"][1].astype(D)
        t = prims[prims.shape[0] // 3]
        v, e1, e2 = t["vert"].astype(D), t["e1"].astype(D), t["e2"].astype(D)
        hand = np.array([v, v + 0.5 * e1, v + 0.25 * e1 + 0.25 * e2, tree.p[0], tree.p[nodes.shape[0] // 2]]).astype(F)
    rng = np.random.default_rng(sum(map(ord, name)))
    size = hi - lo
    pts = np.concatenate([((lo - 0.25 * size) + 1.5 * size * rng.random((2048, 3))).astype(F), hand])
    for a in (nodes, prims, pts):
        a.setflags(write=False)
    return nodes, prims, tree, pts


@functools.lru_cache(maxsize=None)
def reference(name, accuracy, n=None):
    """the restatement's (w, terms) for the first n points of a fixture (None: all of them), computed once per process"""
    nodes, prims, tree, pts = fixture(name)
    out = ref.winding(tree, pts if n is None else pts[:n], accuracy)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth(name, n):
    nodes, prims, tree, pts = fixture(name)
    W = ref.truth(prims, pts[:n])
    W.setflags(write=False)
    return W


def cases(name):
    """(accuracy, points asked) of the bit-for-bit tests: the 20480-triangle fixture at 2 and, on 256 points, at inf"""
    if name == "sphere5":
        return [(2.0, None), (INF, 256)]
    return [(a, None) for a in ACCURACIES]


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
def test_hand_cases():
    """inside and outside the box: 1 and 0 at accuracy inf (1 exactly; 0 within the 12 triangles' share of atan2_det's 2^-45 each,
    far below 2^-40).  On a face: a point inside a triangle and in its plane adds 2 pi -- 0.5 on the one-triangle sheet, and on the
    closed box, whose other faces add the far hemisphere, 1, as the brute-force sum with numpy.arctan2 has it; on a box edge and
    vertex, where the touching triangles add nothing, 0.25 and 0.125.  Every one of the 12 triangles is summed, no dipole."""
    nodes, prims, tree, _ = fixture("box")
    pts = np.array([[0, 0, 15], [30, 0, 15], [3, 1, 25], [0, 10, 25], [10, 10, 25], [np.nan, 0, 0], [0, -np.inf, 0]], F)
    w, terms = ref.winding(tree, pts, INF)
    assert w[0] == 1.0 and abs(w[1]) < 2.0 ** -40
    assert w[2] == 1.0 and w[3] == 0.25 and w[4] == 0.125
    assert np.abs(ref.truth(prims, pts[:5]) - w[:5]).max() < 2.0 ** -40
    assert terms[:5].tolist() == [[0, 12]] * 5
    assert w[5:].view(U).tolist() == [ref.QNAN] * 2 and terms[5:].tolist() == [[0, 0]] * 2
    n1, p1, t1, _ = fixture("one")
    w, terms = ref.winding(t1, np.array([[-3, -1, 20], [-3, -1, 21], [-3, -1, 19], [-8, -6, 20]], F), INF)
    assert w[0] == 0.5 and -0.5 < w[1] < 0 and w[2] == -w[1] and w[3] == 0.0 and terms.tolist() == [[0, 1]] * 4  # (the normal side is outside)
    # far away the box is one dipole, and a closed mesh's area vectors cancel: N = 0 up to rounding, w = 0
    w, terms = ref.winding(tree, np.array([[500, 300, 100]], F), 2.0)
    assert terms.tolist() == [[1, 0]] and abs(w[0]) < 1e-12
    # accuracy 0: every node whose centre is not the point is far -- the root alone
    w, terms = ref.winding(tree, pts[:2], 0.0)
    assert terms.tolist() == [[1, 0]] * 2
    # no triangles
    w, terms = ref.winding(None, pts, 2.0)
    assert w[:5].tolist() == [0.0] * 5 and not terms.any() and w[5:].view(U).tolist() == [ref.QNAN] * 2


def test_atan2_det_special_values():
    a = ref.atan2_det
    assert a(0.0, 0.0) == 0.0 and a(-0.0, 0.0) == 0.0 and a(0.0, -0.0) == 0.0
    assert a(0.0, 1.0) == 0.0 and a(0.0, -1.0) == ref.PI and a(1.0, 0.0) == ref.PIO2 and a(-1.0, 0.0) == -ref.PIO2
    assert a(1.0, 1.0) == ref.PIO4 and a(-1.0, -1.0) == -(ref.PI - ref.PIO4) and a(1e-300, 1e300) == 0.0
    assert np.isnan(a(np.nan, 1.0)) and np.isnan(a(1.0, np.nan)) and np.isnan(a(np.inf, np.inf))
    assert ref.PI == math.pi and ref.INV_4PI == 1.0 / (4.0 * math.pi) and abs(ref.TAN_PIO8 - (2.0 ** 0.5 - 1.0)) < 2.0 ** -52
    assert [float(c) for c in ref.SERIES[:3]] == [1.0, -1.0 / 3.0, 0.2]


def test_skip_on_a_tree_written_out_by_hand():
    """five nodes: 0 = (1, 4), 1 = (2, 3), leaves 2, 3, 4"""
    from tyrant_amd import scenes

    nodes = np.zeros(5, dtype=scenes.NODE_DTYPE)
    nodes["offset"] = [4, 3, 0, 1, 2]
    nodes["primitiveCount"] = [0, 0, 1, 1, 1]
    assert ref.skips(nodes).tolist() == [5, 4, 3, 4, 5]
    assert ref.skips(nodes[:0]).tolist() == []
    one = nodes[2:3]
    assert ref.skips(one).tolist() == [1]


def test_the_zero_area_branch_is_reached():
    """the degenerate fixture has a node without area: its centre is its box's, and a point there meets no NaN"""
    nodes, prims, tree, pts = fixture("degenerate")
    zero = np.nonzero(tree.S == 0.0)[0]
    assert zero.size > 0
    i = zero[0]
    lo, hi = nodes[i]["bounds"][0].astype(D), nodes[i]["bounds"][1].astype(D)
    assert np.array_equal(tree.p[i], 0.5 * (lo + hi)) and not tree.N[i].any()
    w, _ = ref.winding(tree, np.concatenate([tree.p[zero].astype(F), pts[:64]]), 2.0)
    assert np.isfinite(w).all()


def atan2_arguments():
    """a seeded million (y, x) spanning 2^+-60 in ratio, as binary32 pairs (the probe's input), and a fine sweep of the circle"""
    rng = np.random.default_rng(2024)
    n = 1 << 20
    y = (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-30, 31, n))).astype(F)
    x = (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-30, 31, n))).astype(F)
    th = (np.arange(1 << 18) + 0.5) * (2.0 * np.pi / (1 << 18)) - np.pi
    return np.concatenate([y, np.sin(th).astype(F)]), np.concatenate([x, np.cos(th).astype(F)])


def test_atan2_det_against_libm():
    y, x = atan2_arguments()
    got = ref.atan2_det(y.astype(D), x.astype(D))
    err = np.abs(got - np.arctan2(y.astype(D), x.astype(D)))
    i = int(np.argmax(err))
    assert abs(got[i] - math.atan2(float(y[i]), float(x[i]))) <= 2.0 ** -45  # ... and math.atan2 at the worst argument
    print(f"atan2_det against atan2 over {y.size} arguments: largest difference {err.max():.3e} (2^-45 = {2.0 ** -45:.3e})")
    assert err.max() <= 2.0 ** -45
    th = np.linspace(-np.pi, np.pi, 1 << 18)
    e2 = np.abs(ref.atan2_det(np.sin(th), np.cos(th)) - np.arctan2(np.sin(th), np.cos(th)))
    assert e2.max() <= 2.0 ** -45


@pytest.mark.parametrize("name", ALL)
def test_the_exact_mode_against_the_truth(name):
    """accuracy inf is the sum over every triangle: within 2^-22 of the brute-force binary64 sum with numpy.arctan2"""
    nodes, prims, tree, pts = fixture(name)
    n = 256 if name == "sphere5" else None
    w, terms = reference(name, INF, n)
    W = truth(name, w.shape[0])
    err = np.abs(w.astype(D) - W)
    print(f"{name}: accuracy inf against the truth over {w.shape[0]} points, largest difference {err.max():.3e}, mean {err.mean():.2e}")
    assert err.max() <= 2.0 ** -22
    assert (terms[:, 0] == 0).all() and (terms[:, 1] == prims.shape[0]).all()


@pytest.mark.parametrize("name", CLOSED)
def test_the_expansion_against_the_truth(name):
    """the three closed fixtures, 2048 sampled points: every point rounds to the truth's integer at accuracy 2, 3 and 4, and the
    largest error at 4 is below the one at 2.  Prints the rows of DESIGN.md's table: largest and mean error, dipoles and triangles
    per point."""
    nodes, prims, tree, pts = fixture(name)
    W = truth(name, 2048)
    assert set(np.round(W).astype(int).tolist()) == ({0, 1}) and np.abs(W - np.round(W)).max() < 1e-4
    worst = {}
    for acc in (1.0, 2.0, 3.0, 4.0):
        w, terms = reference(name, acc, 2048)
        err = np.abs(w.astype(D) - W)
        worst[acc] = err.max()
        print(f"{name} accuracy {acc}: max error {err.max():.4f}, mean {err.mean():.2e}, dipoles {terms[:, 0].mean():.1f}, triangles {terms[:, 1].mean():.1f}")
        if acc >= 2.0:
            assert np.array_equal(np.round(w.astype(D)), np.round(W)), (acc, np.count_nonzero(np.round(w.astype(D)) != np.round(W)))
    assert worst[4.0] < worst[2.0]


def test_winding_kernels_need_no_scratch():
    """k_winding is stackless: no spilled VGPR and not a byte of scratch; the two build kernels spill no VGPR.  Occupancy and
    LDS are printed (DESIGN.md "Winding numbers" records them), not held to a guess."""
    res = kernel_resources("winding")
    found = {}
    for key, pat in (("query", "9k_windingE"), ("parents", "k_winding_parents"), ("moments", "k_winding_moments")):
        names = [n for n in res if pat in n]
        assert len(names) == 1, list(res)
        found[key] = res[names[0]]
        print(names[0], found[key])
        assert found[key]["VGPRs Spill"] == 0, found[key]
    assert found["query"]["ScratchSize [bytes/lane]"] == 0, found["query"]


def test_abi_declares_exports_and_refuses(hip):
    code = header_code()
    assert re.search(r"\bint\s+tyr_query_winding\s*\(", code) and re.search(r"\bint\s+tyr_scene_moments\s*\(", code)
    assert re.search(r"#define\s+TYR_FLAG_WINDING\s+128u", code) and re.search(r"#define\s+TYR_ABI_VERSION\s+5\b", code)
    L = hip.lib()
    assert L.tyr_abi_version() == 5 and hip.TYR_FLAG_WINDING == WINDING
    buf = (C.c_float * 12)()
    assert L.tyr_query_winding(None, 1, buf, 2.0, buf, None, None) == hip.TYR_ERR_INVALID
    assert L.tyr_scene_moments(None, 0, 0, None) == hip.TYR_ERR_INVALID
    for op in list(range(20, 32)) + [53, 64]:
        assert L.tyr_vecmath_probe(0, op, buf, buf, buf, 1, buf) == hip.TYR_ERR_INVALID, op


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, pts, accuracy, terms=True, **kw):
    """query_winding's answer as numpy arrays, terms as the library's uint32 (the fixtures' arrays are read-only: torch wants its own)"""
    res = g.query_winding(np.array(pts), accuracy=accuracy, terms=terms, **kw)
    if not terms:
        return res.cpu().numpy(), None
    return res[0].cpu().numpy(), res[1].cpu().numpy().view(U)


same = functools.partial(same_outputs, ("w", "terms"))  # (terms not asked for: None, and not compared)


def same_moments(got, tree, what=""):
    want = tree.moments()
    assert got.shape == want.shape, what
    bad = got.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), f"{what}: moments differ at {np.argwhere(bad)[:5].tolist()} ({np.count_nonzero(bad)} words)"


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_moments_bit_for_bit_through_every_upload_path(hip, name):
    """tyr_scene_moments (p, N, r2, S of every node) against the restatement by bits: tyr_scene_upload with the layout pass on the
    host and on the device, and tyr_scene_build_upload, whose tree is the device builder's"""
    nodes, prims, tree, _ = fixture(name)
    for lod in (0, 1):
        g = renderer(hip, nodes, prims, flags=WINDING, layout_on_device=lod)
        same_moments(g.scene_moments(), tree, f"{name}, layout_on_device {lod}")
        last = nodes.shape[0] - 1
        assert np.array_equal(g.scene_moments(last, 1).view(np.uint64), tree.moments()[last:].view(np.uint64))  # a range of its own
        g.close()
    g = hip.Renderer(64, 64, 4096, flags=WINDING)
    n2, p2, _ = g.build_upload(triangles_of(name))
    same_moments(g.scene_moments(), ref.Tree(n2, p2), f"{name}, build_upload")
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL + ("empty",))
def test_bit_for_bit_against_the_restatement(hip, name):
    """w and terms by bits at accuracy 0, 1, 2, 3.5 and inf, on batches of 1, 63, 64, 65, 257, 2048 points and on the whole set
    with its hand-placed points (a vertex, an edge, a face's plane, two nodes' centres)"""
    nodes, prims, tree, pts = fixture(name)
    g = renderer(hip, nodes, prims, flags=WINDING)
    for acc, limit in cases(name):
        want = reference(name, acc, limit)
        total = want[0].shape[0]
        for n in [s for s in SIZES if s < total] + [total]:
            same(ask(g, pts[:n], acc), (want[0][:n], want[1][:n]), f"{name}, accuracy {acc}, n {n}")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_probe_ops_bit_for_bit(hip):
    """ops 50-52 on the device -- atan2_det, the binary64 quotient and the square root of a binary64 product -- equal numpy's"""
    y, x = atan2_arguments()
    a, b = np.zeros((y.size, 3), F), np.zeros((y.size, 3), F)
    a[:, 0], b[:, 0] = y, x
    with np.errstate(all="ignore"):
        want = {50: ref.atan2_det(y.astype(D), x.astype(D)), 51: y.astype(D) / x.astype(D), 52: np.sqrt(y.astype(D) * x.astype(D))}
    for op, w in want.items():
        out = hip.contract_probe(op, a, b)
        got = (out[:, 1].astype(np.uint64) | (out[:, 2].astype(np.uint64) << np.uint64(32)))
        wb = w.view(np.uint64).copy()
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(got.view(D)), nan), op
        assert np.array_equal(got[~nan], wb[~nan]), (op, np.count_nonzero(got[~nan] != wb[~nan]))
        assert not out[:, 0].any()


@pytest.mark.gpu
def test_independence(hip):
    """the first m points of a batch give what a batch of m gives; terms_out NULL changes nothing; a permuted batch gives the
    permuted answers; two runs are identical"""
    nodes, prims, tree, pts = fixture("torus")
    g = renderer(hip, nodes, prims, flags=WINDING)
    big = ask(g, pts, 2.0)
    same(big, reference("torus", 2.0), "the whole batch")
    for m in (1, 100, 1000):
        same(ask(g, pts[:m], 2.0), (big[0][:m], big[1][:m]), f"the first {m}")
    same(ask(g, pts, 2.0, terms=False), big, "without terms")
    perm = np.random.default_rng(5).permutation(pts.shape[0])
    same(ask(g, pts[perm], 2.0), (big[0][perm], big[1][perm]), "permuted")
    same(ask(g, pts, 2.0), big, "a second run")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_refit_rebuilds_the_moments(hip):
    """a ctx with both flags: after a refit of the torus with displaced vertices the moments and the answers are the restatement's
    on nodes_out and the new triangles; a ctx with TYR_FLAG_WINDING alone refuses the refit as a ctx without flags does"""
    nodes, prims, tree, pts = fixture("torus")
    g = renderer(hip, nodes, prims, flags=WINDING | REFIT)
    same_moments(g.scene_moments(), tree, "before the refit")
    moved = prims.copy()
    moved["vert"][:, 2] += (1.5 * np.sin(moved["vert"][:, 0] * 0.2)).astype(F)
    moved["e1"] = (moved["e1"] * F(1.125)).astype(F)
    new_nodes = g.refit(moved, want_nodes=True)
    t2 = ref.Tree(new_nodes, moved)
    assert not np.array_equal(t2.moments(), tree.moments())
    same_moments(g.scene_moments(), t2, "after the refit")
    for acc in (2.0, INF):
        same(ask(g, pts[:512], acc), ref.winding(t2, pts[:512], acc), f"after the refit, accuracy {acc}")
    assert g.query_error() == 0
    g.close()
    for flags in (WINDING, 0):
        g = renderer(hip, nodes, prims, flags=flags)
        with pytest.raises(hip.TyrError) as e:
            g.refit(moved)
        assert e.value.status == hip.TYR_ERR_UNSUPPORTED
        if flags:
            same_moments(g.scene_moments(), tree, "after the refused refit")
        g.close()


@pytest.mark.gpu
def test_winding_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64) with winding queries between its two halves: the same accumulation buffer, counters, queues
    and scene hash as the uninterrupted render's, and as a ctx without the flag"""
    from tyrant_amd import scenes

    tree = ref.Tree(*build(scenes.cornell_box().triangles))
    pts = fixture("box")[3]
    want = ref.winding(tree, pts[:512], 2.0)

    def between(g):
        same(ask(g, pts[:512], 2.0), want, "between two renders")
        ask(g, pts, INF, terms=False)

    # the first run on a ctx without the flag, the other two with it
    (_, k0, _, _, h0), (_, k1, _, _, h1), (_, kq, _, _, hq) = assert_render_undisturbed(between, flags=(0, WINDING, WINDING), also=lambda g: g.scene_hash())
    assert kq == k0 == k1, {k: (k0[k], k1[k]) for k in k0 if k0[k] != k1[k]}
    drop = lambda h: {k: v for k, v in h.items() if k != "seconds"}  # noqa: E731
    assert drop(hq) == drop(h0) == drop(h1)


@pytest.mark.gpu
@pytest.mark.parametrize("lod", [0, 1])
def test_a_ctx_without_the_flag_is_what_it_was(hip, lod):
    """without TYR_FLAG_WINDING: device_bytes is the scene's arrays alone, the hash is the host layout's, and both calls answer
    TYR_ERR_UNSUPPORTED; with it: the same hash, and device_bytes grows by the moment tree (72 bytes per node)"""
    import torch

    nodes, prims, tree, pts = fixture("torus")
    g0, g1 = (renderer(hip, nodes, prims, flags=f, layout_on_device=lod) for f in (0, WINDING))
    i0, i1 = g0.scene_info(), g1.scene_info()
    assert i0["device_bytes"] == i0["n_quad_nodes"] * 128 + i0["n_prims"] * 48
    assert i1["device_bytes"] == i0["device_bytes"] + 72 * nodes.shape[0]
    assert {k: v for k, v in i0.items() if not k.endswith("_s") and k != "device_bytes"} == {k: v for k, v in i1.items() if not k.endswith("_s") and k != "device_bytes"}
    probe = hip.layout_probe(nodes, prims)
    for g in (g0, g1):
        h = g.scene_hash()
        assert (h["hash_quads"], h["hash_tris"], h["n_quad_nodes"]) == (probe["hash_quads"], probe["hash_tris"], probe["n_quad_nodes"])
    p = torch.from_numpy(np.array(pts[:4])).cuda()
    w = torch.full((4,), 7.0, dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    assert hip.lib().tyr_query_winding(g0.h, 4, C.c_void_p(p.data_ptr()), 2.0, C.c_void_p(w.data_ptr()), None, None) == hip.TYR_ERR_UNSUPPORTED
    out = np.zeros(8, D)
    assert hip.lib().tyr_scene_moments(g0.h, 0, 1, out.ctypes.data_as(C.c_void_p)) == hip.TYR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (w.cpu().numpy() == 7.0).all()
    g0.close()
    g1.close()


@pytest.mark.gpu
def test_two_streams_and_invalid_arguments(hip):
    """two torch streams each carry a query of their own; bad arguments are refused before any launch; n == 0 is TYR_OK"""
    import torch

    nodes, prims, tree, pts = fixture("nested")
    g = renderer(hip, nodes, prims, flags=WINDING)
    tp = torch.from_numpy(np.array(pts)).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        r1 = g.query_winding(tp, accuracy=2.0, terms=True, stream=s1)
    with torch.cuda.stream(s2):
        r2 = g.query_winding(tp, accuracy=3.5, terms=True, stream=s2)
    s1.synchronize()
    s2.synchronize()
    same((r1[0].cpu().numpy(), r1[1].cpu().numpy().view(U)), reference("nested", 2.0), "stream 1")
    same((r2[0].cpu().numpy(), r2[1].cpu().numpy().view(U)), reference("nested", 3.5), "stream 2")

    L, h, P = hip.lib(), g.h, C.c_void_p
    m = 4
    w, t = torch.full((m,), 7.0, dtype=torch.float32).cuda(), torch.full((m, 2), 7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    inv = hip.TYR_ERR_INVALID
    call = lambda ctx=h, n=m, a=P(tp.data_ptr()), acc=2.0, out=P(w.data_ptr()): L.tyr_query_winding(ctx, n, a, acc, out, P(t.data_ptr()), None)  # noqa: E731
    assert call(ctx=None) == inv and call(a=None) == inv and call(out=None) == inv and call(n=1 << 31) == inv
    assert call(acc=float("nan")) == inv and call(acc=-1.0) == inv and call(acc=-0.0) == 0 and call(acc=INF) == 0
    assert L.tyr_query_winding(h, 0, None, 2.0, None, None, None) == 0
    nn = nodes.shape[0]
    buf = np.zeros(8 * nn, D)
    bp = buf.ctypes.data_as(P)
    assert L.tyr_scene_moments(h, -1, 1, bp) == inv and L.tyr_scene_moments(h, 0, -1, bp) == inv and L.tyr_scene_moments(h, 1, nn, bp) == inv
    assert L.tyr_scene_moments(h, 0, 1, None) == inv and L.tyr_scene_moments(h, nn, 0, None) == 0
    empty = hip.Renderer(64, 64, 1024, flags=WINDING)  # no scene uploaded
    assert call(ctx=empty.h) == hip.TYR_ERR_NO_SCENE and L.tyr_scene_moments(empty.h, 0, 0, None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_winding(tp.double())
    with pytest.raises(ValueError):
        g.query_winding(tp[:, :2].contiguous())
    assert ask(g, pts[:0], 2.0)[0].shape == (0,)
    assert call() == 0
    assert g.query_error() == 0
    same((w.cpu().numpy(), t.cpu().numpy().view(U)), ref.winding(tree, pts[:m], 2.0), "the accepted call")
    g.close()


@pytest.mark.gpu
def test_hostile_input(hip):
    """NaN and infinite points, a point 1e30 away, accuracy 1e-30 and 1e30, and the scene without triangles -- against the restatement"""
    nodes, prims, tree, pts = fixture("soup")
    g = renderer(hip, nodes, prims, flags=WINDING)
    p = np.array(pts[:512])
    rng = np.random.default_rng(9)
    kind = rng.integers(0, 6, p.shape[0])
    for i in np.nonzero(kind == 0)[0]:
        p[i, rng.integers(0, 3)] = (np.nan, np.inf, -np.inf)[rng.integers(0, 3)]
    p[kind == 1] *= F(1e30)
    p[kind == 2, 0] = F(3e38)
    for acc in (1e-30, 2.0, 1e30, INF):
        want = ref.winding(tree, p, acc)
        assert (want[0][kind == 0].view(U) == ref.QNAN).all() and not want[1][kind == 0].any() and np.isfinite(want[0][kind != 0]).all()
        same(ask(g, p, acc), want, f"hostile, accuracy {acc}")
    none_n, none_p, _, epts = fixture("empty")
    g.upload(none_n, none_p)
    assert g.scene_moments().shape == (0, 8)
    e = np.array(epts[:64])
    e[3, 1] = np.nan
    got = ask(g, e, 2.0)
    same(got, ref.winding(None, e, 2.0), "no triangles")
    assert got[0][0] == 0.0 and got[0][3:4].view(U)[0] == ref.QNAN
    assert g.query_error() == 0
    g.close()
