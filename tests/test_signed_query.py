"""Signed-distance queries and the SDF grid bake on the uploaded scene (tyr_query_signed, tyr_bake_sdf, hip/signed.hip;
Renderer.query_signed, Renderer.bake_sdf): include/tyr_c.h "Signed-distance queries", bit for bit against the numpy restatement
(tests/signed_ref.py), which joins the restatements of the two contracts a signed distance is made of.

CPU: the join's rules by hand, what the grid fixtures are for (far bricks inside and outside, near bricks of both signs) and that
the restatement agrees with itself on the closed shapes, what the compiler made of the kernels, the ABI.  GPU: every scene
family with points and bounds of every kind, the composition against this ctx's own query_nearest and query_winding, grids cut
on every axis, bands from below half a cell to beyond the grid, large origins, the shortcut property on closed meshes, refit,
streams, repeatability, isolation from the render, argument checks, and the recorded answers on C3's 1 M-triangle tree."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest

import nearest_ref
import signed_ref as ref
from conftest import GOLDEN, bits, built_scene
from query_support import (assert_kernel_budget, assert_query_abi, assert_render_undisturbed, box, box_points, build, deformed, duplicated, launch_bounds_blocks, no_triangles,
                           offset_soup, on_side_stream, query_exists, renderer, surface_points)
from query_support import same as same_outputs

F = np.float32
D = np.float64
INF = float("inf")
WINDING = 128
REFIT = 64
NAMES = ref.NAMES
GRID_NAMES = ("sd", "prim", "stats")
C3_ANSWERS = os.path.join(GOLDEN, "signed_c3.npz")
SIZES = (1, 63, 64, 65, 4097)

_the_query_exists = query_exists("tyr_query_signed", "tyr_bake_sdf")  # nothing here means anything without the entry points


# ---- fixtures (numpy only; made once, never changed) ------------------------------------------------------------------
def inward(tris):
    t = tris.copy()
    t["e1"], t["e2"] = tris["e2"], tris["e1"]
    return t


@functools.lru_cache(maxsize=None)
def icosphere(level, radius, centre):
    """a closed outward-facing sphere of 20 * 4^level triangles"""
    from tyrant_amd import scenes

    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [np.array(x, D) / np.linalg.norm(x) for x in ((-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1))]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9),
         (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
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
    P = V * radius + np.asarray(centre, D)
    return scenes.make_triangles(P[Fc[:, 0]], P[Fc[:, 1]], P[Fc[:, 2]])


CUBE_LO, CUBE_HI = (2.25, 2.25, 2.25), (18.25, 18.25, 18.25)  # 16 cells across in a 24^3 grid of unit cells at the origin


def cube_special_points():
    """inside, outside, on a face, on an edge, on a vertex, at the centre -- of the cube CUBE_LO .. CUBE_HI"""
    lo, hi, c = CUBE_LO[0], CUBE_HI[0], 10.25
    return np.array([[5, 6, 7], [c, c, 17.75], [30, 6, 7], [-4, -5, -6], [c, c, 25], [lo, 7, 9], [c, hi, c], [lo, lo, 8], [hi, c, hi], [lo, lo, lo], [hi, lo, hi], [c, c, c], [lo, 7, 9.000001],
                     [2.2500002, 7, 9]], F)


@functools.lru_cache(maxsize=None)
def family(name):
    """(nodes, prims, points, max_dist per point) of a scene family; the points are hand-placed ones where the family has them,
    seeded ones in the inflated root box and seeded ones within 1e-2 of the surface (every tenth of those on it)"""
    from tyrant_amd import scenes

    rng = np.random.default_rng(sum(map(ord, name)))
    hand = np.zeros((0, 3), F)
    n_box, n_surf = 300, 200
    if name == "cube":
        nodes, prims = build(box(CUBE_LO, CUBE_HI))
        hand = cube_special_points()
    elif name == "inward":
        nodes, prims = build(inward(box(CUBE_LO, CUBE_HI)))
        hand = cube_special_points()
    elif name == "nested":
        nodes, prims = build(np.concatenate([box(CUBE_LO, CUBE_HI), box((6.5, 6.5, 6.5), (13.5, 13.5, 13.5))]))
        hand = np.concatenate([cube_special_points(), np.array([[10, 10, 10], [7, 8, 9], [6.5, 8, 9], [4, 8, 9]], F)])
    elif name == "sheet":
        nodes, prims = build(scenes.heightfield(16))
    elif name == "soup":
        nodes, prims = offset_soup(True)
    elif name == "duplicated":
        nodes, prims, pts, _ = duplicated(61, 200)
        hand = pts[::3].copy()
        n_box = 0
    elif name == "sphere":
        nodes, prims = build(icosphere(3, 9.0, (11.0, 12.0, 13.0)))
    elif name == "empty":
        nodes, prims = no_triangles()
        some = box((0, 0, 0), (1, 1, 1))
        pts = np.concatenate([cube_special_points(), box_points(rng, some, 100)])
        return nodes, prims, pts, rng.choice(np.array([0.0, 0.5, 3.0, np.inf], F), len(pts)).astype(F)
    else:
        raise KeyError(name)
    surf = surface_points(rng, prims, n_surf, 1e-2)
    surf[::10] = surface_points(rng, prims, len(surf[::10]), 0.0)
    pts = np.ascontiguousarray(np.concatenate([hand, box_points(rng, prims, n_box), surf]), F)
    md = rng.choice(np.array([0.0, 0.05, 0.5, 3.0, 50.0, np.inf, np.inf], F), len(pts)).astype(F)
    return nodes, prims, pts, md


FAMILIES = ("cube", "inward", "nested", "sheet", "soup", "duplicated", "empty")


@functools.lru_cache(maxsize=None)
def tree(name):
    nodes, prims, _, _ = family(name)
    return ref.tree_of(nodes, prims)


@functools.lru_cache(maxsize=None)
def want_points(name, bound, accuracy):
    """the restatement's answers for family(name): bound "none" (max_dist NULL), "each" (per point) or "zero" (all 0)"""
    nodes, prims, pts, md = family(name)
    md = {"none": None, "each": md, "zero": np.zeros(len(pts), F)}[bound]
    return ref.signed(pts, nodes, prims, md, accuracy, tree=tree(name))


# the grids: name -> (family, origin, cell, dims, band)
GRIDS = {
    "one": ("cube", (9.0, 9.0, 1.5), 1.0, (1, 1, 1), 1.0),
    "cut": ("cube", (0.0, 0.5, 1.0), 1.0, (5, 6, 7), 1.0),  # bricks cut short on every axis
    "cube24": ("cube", (0.0, 0.0, 0.0), 1.0, (24, 24, 24), 1.0),
    "thin": ("cube", (0.0, 0.0, 0.0), 1.5, (14, 13, 15), 0.6),  # band < cell / 2
    "wide": ("cube", (0.0, 0.0, 0.0), 2.0, (11, 12, 10), 100.0),  # band larger than the grid: no brick is far
    "nested": ("nested", (0.1, 0.2, 0.3), 1.0, (22, 21, 23), 1.0),
    "sphere": ("sphere", (0.0, 1.0, 2.0), 1.0, (23, 22, 24), 1.0),
    "sheet": ("sheet", (-30.0, -30.0, -5.0), 3.0, (20, 19, 10), 4.0),
    "empty": ("empty", (-1.0, 0.0, 1.0), 1.0, (5, 4, 3), 1.0),  # a scene without triangles: every brick far, +band
}


@functools.lru_cache(maxsize=None)
def far_cube():
    """the cube moved by about 1e4 per axis, where the binary32 rounding of the voxel centres matters: (nodes, prims, grid)"""
    shift = np.array([10000.0, -9000.0, 12000.0], F)
    tris = box(tuple(np.array(CUBE_LO, F) + shift), tuple(np.array(CUBE_HI, F) + shift))
    nodes, prims = build(tris)
    return nodes, prims, (tuple(float(x) for x in shift + F(0.13)), 0.3697, (60, 58, 62), 0.9)


def grid_scene(name):
    if name == "far_cube":
        nodes, prims, grid = far_cube()
        return nodes, prims, grid
    fam, *grid = GRIDS[name]
    nodes, prims, _, _ = family(fam)
    return nodes, prims, tuple(grid)


@functools.lru_cache(maxsize=None)
def want_grid(name, accuracy=2.0):
    nodes, prims, (origin, cell, dims, band) = grid_scene(name)
    return ref.bake(nodes, prims, origin, cell, dims, band, accuracy)


ALL_GRIDS = tuple(GRIDS) + ("far_cube",)
CLOSED_GRIDS = ("cube24", "nested", "sphere")


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
def test_hand_cases():
    """exactly representable numbers on the cube: sign, root, the gradient's three rules, the bound, every invalid input"""
    nodes, prims, _, _ = family("cube")
    t = tree("cube")
    lo, hi, c = CUBE_LO[0], CUBE_HI[0], 10.25

    def one(p, md=None, acc=2.0, scene=(nodes, prims, t)):
        res = ref.signed(np.array([p], F), scene[0], scene[1], None if md is None else np.array([md], F), acc, tree=scene[2])
        return tuple(a[0] for a in res)

    sd, prim, point, grad, w = one((c, c, hi + 4))
    assert (float(sd), point.tolist(), grad.tolist()) == (4.0, [c, c, hi], [0, 0, 1]) and prim >= 0 and abs(w) < 1e-6
    sd, prim, point, grad, w = one((c, c, hi - 3))  # inside: negative, and the gradient still points outward
    assert (float(sd), point.tolist(), grad.tolist()) == (-3.0, [c, c, hi], [0, 0, 1]) and abs(w - 1) < 1e-6
    sd, prim, point, grad, w = one((c - 1, c + 2, hi))  # on a face: the triangle's unit normal
    assert (float(sd), grad.tolist()) == (0.0, [0, 0, 1])  # (+0 or -0: on the surface w is 0.5 up to its rounding)
    sd, prim, point, grad, w = one((hi + 3, hi + 4, c))  # off an edge
    assert (float(sd), point.tolist(), grad.tolist()) == (5.0, [hi, hi, c], [F(3.0 / 5.0), F(4.0 / 5.0), 0])
    # the root is the correctly rounded binary32 root of dist2
    sd, _, point, _, _ = one((hi + 1, hi + 1, hi + 1))
    assert point.tolist() == [hi, hi, hi] and bits(sd) == bits(F(np.sqrt(D(3.0))))
    # the bound: without a triangle nearer than max_dist the bound itself, with the point's own sign; strict as 4l's
    for p, md, want in (((c, c, hi + 4), 1.5, 1.5), ((c, c, c), 1.5, -1.5), ((c, c, hi + 4), 4.0, 4.0), ((c, c, c), None, -8.0), ((c, c, hi + 4), 0.0, 0.0), ((c, c, c), 0.0, -0.0)):
        sd, prim, point, grad, _ = one(p, md)
        assert bits(sd) == bits(F(want)) and (prim >= 0) == (md is None) and (md is None or (point.tolist() == list(p) and grad.tolist() == [0, 0, 0])), (p, md, sd)
    assert int(one((c, c, hi + 4), np.nextafter(F(4), F(5)))[1]) >= 0
    # the cube facing inward: the inside is positive; a scene without triangles: +max_dist, +inf
    inn, ipr, _, _ = family("inward")
    assert float(one((c, c, c), scene=(inn, ipr, tree("inward")))[0]) == 8.0 and float(one((c, c, 40), scene=(inn, ipr, tree("inward")))[0]) == 21.75  # (w = -1 inside, 0 outside)
    e = no_triangles()
    assert float(one((1, 2, 3), scene=(e[0], e[1], None))[0]) == INF and float(one((1, 2, 3), 2.5, scene=(e[0], e[1], None))[0]) == 2.5
    # invalid input: sd and w the quiet NaN, prim -1, point p, gradient 0
    for p, md in (((np.nan, 1, 2), None), ((1, np.inf, 2), 3.0), ((1, 2, -np.inf), None), ((1, 2, 3), np.nan), ((1, 2, 3), -1.0), ((1, 2, 3), -np.inf)):
        sd, prim, point, grad, w = one(p, md)
        assert bits(sd) == bits(w) == 0x7FC00000 and prim == -1 and grad.tolist() == [0, 0, 0] and np.array_equal(bits(point), bits(np.array(p, F)))
    assert float(one((c, c, hi + 4), -0.0)[0]) == 0.0  # -0 is a valid bound
    # accuracy 0 sums the root's dipole alone; inf is the exact sum
    assert abs(float(one((c, c, c), acc=INF)[4]) - 1) < 1e-6 and float(one((c, c, c), acc=0.0)[4]) != float(one((c, c, c), acc=INF)[4])


def test_voxel_and_brick_centres_and_reach():
    """the grid's rules: centres rounded operation by operation (not origin + cell * i + cell / 2), bricks of four, the reach"""
    x = ref.voxel_axis(10000.13, 0.3697, 60)
    assert x.dtype == F and bits(x)[7] == bits(F(F(10000.13) + F(F(0.3697) * F(7.5))))
    # on the far cube's grid the roundings are visible: one rounding of the exact sum (what an fma would give) is another word
    (origin, cell, dims, _), differ = far_cube()[2], 0
    for k in range(3):
        once = (D(F(origin[k])) + D(F(cell)) * (np.arange(dims[k]) + 0.5)).astype(F)
        differ += int((bits(ref.voxel_axis(origin[k], cell, dims[k])) != bits(once)).sum())
    assert differ >= 2
    b = ref.brick_axis(1.0, 0.5, 3)
    assert b.tolist() == [2.0, 4.0, 6.0]
    assert bits(ref.reach(1.0, 1.0)) == bits(F(3.625)) and bits(ref.reach(0.9, 0.37)) == bits(F(F(0.9) + F(F(2.625) * F(0.37))))
    # no voxel centre of a brick lies farther from the brick's centre than 2.625 cells, roundings included, on a grid whose cell is at
    # least 2^-15 of its largest coordinate (DESIGN.md "Signed distance" derives it; a finer grid's centres collide anyway)
    for origin, cell in ((0.0, 1.0), (10000.13, 0.3697), (-9000.0, 0.3697), (12000.0, 0.3697), (-3.0e4, 1.0), (3.0, 1e4), (2.0**20, 33.0)):
        v, c = ref.voxel_axis(origin, cell, 64).astype(D), ref.brick_axis(origin, cell, 16).astype(D)
        worst = np.abs(v.reshape(16, 4) - c[:, None]).max()
        assert np.sqrt(3.0) * worst <= 2.625 * D(F(cell)), (origin, cell, worst)


def test_grid_fixtures_hold_what_they_are_for():
    """the 24^3 grid round the cube: a far brick inside, one outside, near bricks, and a near brick with voxels of both signs; the
    thin band has far bricks, the wide band none; the far cube's centres are not what exact arithmetic would give"""
    sd, prim, stats, far = want_grid("cube24")
    fill = sd[::4, ::4, ::4]
    assert (far & (fill < 0)).any() and (far & (fill > 0)).any() and (~far).any()
    assert stats.tolist() == [int((~far).sum()), int(far.sum())] and stats.sum() == 216
    both = False
    for bk, bj, bi in np.argwhere(~far):
        v = sd[4 * bk:4 * bk + 4, 4 * bj:4 * bj + 4, 4 * bi:4 * bi + 4]
        both = both or ((v < 0).any() and (v > 0).any())
    assert both
    assert (prim[np.abs(sd) < 1] >= 0).all() and (prim[np.abs(sd) == 1] == -1).all()
    assert want_grid("thin")[2][1] > 0 and want_grid("wide")[2][1] == 0 and want_grid("one")[2].sum() == 1
    assert want_grid("cut")[2].sum() == 2 * 2 * 2 and want_grid("far_cube")[2][1] > 0
    assert want_grid("empty")[2].tolist() == [0, 2] and (want_grid("empty")[0] == 1).all()


@pytest.mark.parametrize("name", CLOSED_GRIDS)
def test_the_restatement_agrees_with_itself_on_closed_meshes(name):
    """the shortcut property of the restatement: on a closed, well-shaped mesh the bake equals the point query at every voxel centre"""
    nodes, prims, (origin, cell, dims, band) = grid_scene(name)
    sd, prim, stats, far = want_grid(name)
    assert stats[1] > 0
    pts = ref.voxel_centres(origin, cell, dims)
    fam = GRIDS[name][0]
    psd, pprim, _, _, _ = ref.signed(pts, nodes, prims, np.full(len(pts), band, F), 2.0, tree=tree(fam))
    same_outputs(("sd", "prim"), (sd.reshape(-1), prim.reshape(-1)), (psd, pprim), name)


def test_signed_kernels_keep_registers_and_lds_in_budget():
    """exactly one kernel each for the points, the bricks and the voxels; no vector spills; scratch no larger than the LdsStack's
    private spill arrays (52 entries of 8 bytes, plus the frame's alignment); LDS (24,576 + 7,168 bytes) and an occupancy that admit
    the blocks per CU the launch bounds plan for (profiles/signed_isa.txt records what the compiler reports)"""
    for kernel in ("k_query_signed", "k_sdf_bricks", "k_sdf_voxels"):
        assert_kernel_budget("signed", kernel, 1, (64 - 12) * 8 + 16, 24576 + 7168, planned=launch_bounds_blocks("signed", kernel))


def test_abi_declares_and_exports_the_queries(hip):
    assert_query_abi(hip, "tyr_query_signed", "tyr_signed_out", hip.SignedOut, 5)
    assert_query_abi(hip, "tyr_bake_sdf", "tyr_sdf_out", hip.SdfOut, 3)
    assert C.sizeof(hip.SdfGrid) == 9 * 4


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, pts, md=None, accuracy=2.0, **kw):
    sd, prim, point, w, grad = g.query_signed(np.array(pts), None if md is None else np.array(md), accuracy=accuracy, gradient=True, **kw)
    return tuple(x.cpu().numpy() for x in (sd, prim, point, grad, w))


def ask_grid(g, grid, accuracy=2.0, **kw):
    origin, cell, dims, band = grid
    sd, prim, stats = g.bake_sdf(origin, cell, dims, band, accuracy=accuracy, prim=True, stats=True, **kw)
    return sd.cpu().numpy(), prim.cpu().numpy(), stats.cpu().numpy().view(np.uint32)


same = functools.partial(same_outputs, NAMES)
same_grid = functools.partial(same_outputs, GRID_NAMES)


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_points_bit_for_bit_and_composed(hip, name):
    """all five outputs against the restatement with max_dist NULL, per point and 0; and against this ctx's own query_nearest and
    query_winding joined by the header's rule"""
    nodes, prims, pts, md = family(name)
    g = renderer(hip, nodes, prims, flags=WINDING)
    for bound, m in (("none", None), ("each", md), ("zero", np.zeros(len(pts), F))):
        got = ask(g, pts, m)
        same(got, want_points(name, bound, 2.0), f"{name}, max_dist {bound}")
        dist2, prim, _, _, point = (x.cpu().numpy() for x in g.query_nearest(pts, m))
        w = g.query_winding(pts, accuracy=2.0).cpu().numpy()
        same(got, ref.join(pts, m, dist2, prim, point, w, prims), f"{name}, max_dist {bound}: the two entry points joined")
    sd, prim = want_points(name, "none", 2.0)[:2]
    if name in ("cube", "nested"):  # inside, outside and on the surface
        assert (prim >= 0).all() and (sd < 0).sum() >= 100 and (sd > 0).sum() >= 100 and (sd == 0).sum() >= 10
    if name == "inward":  # w = -1 inside: positive everywhere
        assert not (sd < 0).any()
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("nested", "soup"))
@pytest.mark.parametrize("accuracy", (0.0, INF))
def test_accuracy_is_the_winding_querys(hip, name, accuracy):
    nodes, prims, pts, md = family(name)
    g = renderer(hip, nodes, prims, flags=WINDING)
    same(ask(g, pts, md, accuracy), want_points(name, "each", accuracy), f"{name}, accuracy {accuracy}")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_hostile_input_batch_sizes_and_optional_outputs(hip):
    """the nested cubes: NaN / infinite coordinates, NaN / negative / -0 bounds; batches that go through the refill and the partial
    last wave; every combination of the optional outputs through the C call"""
    import itertools

    import torch

    nodes, prims, _, _ = family("nested")
    rng = np.random.default_rng(71)
    n = SIZES[-1]
    pts = np.concatenate([box_points(rng, prims, n - 1000), surface_points(rng, prims, 1000, 0.3)]).astype(F)
    rng.shuffle(pts)
    md = rng.choice(np.array([0.0, 0.5, 3.0, np.inf, np.inf], F), n).astype(F)
    kind = rng.integers(0, 20, n)
    bad = np.array([np.nan, np.inf, -np.inf], F)
    w = np.nonzero(kind == 0)[0]
    pts[w, rng.integers(0, 3, w.size)] = bad[rng.integers(0, 3, w.size)]
    md[kind == 1] = rng.choice(np.array([np.nan, -1.0, -np.inf, -0.0], F), (kind == 1).sum())
    want = ref.signed(pts, nodes, prims, md, 2.0, tree=tree("nested"))
    invalid = bits(want[0]) == 0x7FC00000
    assert invalid.sum() >= n // 20 and (want[1] < 0).sum() >= n // 10 and (want[4][~invalid] > 1.5).any()
    g = renderer(hip, nodes, prims, flags=WINDING)
    same(ask(g, pts, md), want, "nested, hostile")
    for m in SIZES:  # every prefix answers as the whole batch did
        same(ask(g, pts[:m], md[:m]), tuple(a[:m] for a in want), f"n = {m}")
    m = 500
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a[:m])).cuda()  # noqa: E731
    tp, tm = on(pts), on(md)
    P = C.c_void_p
    kinds = (((), torch.float32), ((), torch.int32), ((3,), torch.float32), ((3,), torch.float32), ((), torch.float32))
    for use in itertools.product((False, True), repeat=4):
        outs = [torch.full((m, *shape), 7, dtype=dtype).cuda() for shape, dtype in kinds]
        torch.cuda.synchronize()
        used = (True,) + use
        out = hip.SignedOut(*[x.data_ptr() if u else None for x, u in zip(outs, used)])
        assert hip.lib().tyr_query_signed(g.h, m, P(tp.data_ptr()), P(tm.data_ptr()), 2.0, 0, C.byref(out), None) == 0
        assert g.query_error() == 0
        res = [x.cpu().numpy() for x in outs]
        same_outputs([nm for nm, u in zip(NAMES, used) if u], [x for x, u in zip(res, used) if u], [a[:m] for a, u in zip(want, used) if u], f"outputs {use}")
        assert all((x == 7).all() for x, u in zip(res, used) if not u), use
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_GRIDS)
def test_grid_bit_for_bit(hip, name):
    """sd, prim and stats of a bake against the restatement; twice, and the two runs are bit-equal"""
    nodes, prims, grid = grid_scene(name)
    sd, prim, stats, _ = want_grid(name)
    g = renderer(hip, nodes, prims, flags=WINDING)
    first = ask_grid(g, grid)
    same_grid(first, (sd, prim, stats), name)
    same_grid(ask_grid(g, grid), first, f"{name}, again")
    only = g.bake_sdf(*grid)
    assert tuple(only.shape) == grid[2][::-1] and np.array_equal(bits(only.cpu().numpy()), bits(sd))
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOSED_GRIDS)
def test_the_bake_equals_the_point_query_on_closed_meshes(hip, name):
    """the shortcut property: every voxel of the bake is query_signed at its centre with max_dist = band, no voxel left out"""
    nodes, prims, grid = grid_scene(name)
    origin, cell, dims, band = grid
    g = renderer(hip, nodes, prims, flags=WINDING)
    sd, prim, stats = ask_grid(g, grid)
    assert stats[1] > 0
    pts = ref.voxel_centres(origin, cell, dims)
    psd, pprim = (x.cpu().numpy() for x in g.query_signed(pts, np.full(len(pts), band, F))[:2])
    same_outputs(("sd", "prim"), (sd.reshape(-1), prim.reshape(-1)), (psd, pprim), name)
    g.close()


@pytest.mark.gpu
def test_refit_and_side_streams(hip):
    """a refit between two calls moves both answers to the refitted scene's; both calls run on a torch side stream with device
    tensors taken in place"""
    import torch

    nodes, prims, grid = grid_scene("sphere")
    origin, cell, dims, band = grid
    rng = np.random.default_rng(72)
    pts = np.concatenate([box_points(rng, prims, 300), surface_points(rng, prims, 200, 0.2)]).astype(F)
    g = renderer(hip, nodes, prims, flags=WINDING | REFIT)
    same(ask(g, pts), ref.signed(pts, nodes, prims), "before the refit")
    moved = deformed(prims, 2.0)
    new_nodes = g.refit(moved, want_nodes=True)
    t = ref.tree_of(new_nodes, moved)
    want = ref.signed(pts, new_nodes, moved, None, 2.0, tree=t)
    assert not np.array_equal(bits(want[0]), bits(ref.signed(pts, nodes, prims)[0]))
    same(ask(g, pts), want, "after the refit")
    wsd, wprim, wstats, _ = ref.bake(new_nodes, moved, origin, cell, dims, band, 2.0, tree=t)
    same_grid(ask_grid(g, grid), (wsd, wprim, wstats), "the bake after the refit")
    tp = torch.from_numpy(pts).cuda()
    res = on_side_stream(lambda side: g.query_signed(tp, None, gradient=True, stream=side))
    same(tuple(res[k].cpu().numpy() for k in (0, 1, 2, 4, 3)), want, "side stream")
    res = on_side_stream(lambda side: g.bake_sdf(*grid, prim=True, stats=True, stream=side))
    same_grid((res[0].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy().view(np.uint32)), (wsd, wprim, wstats), "the bake on a side stream")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_signed_queries_leave_the_render_alone(hip):
    """a Cornell-box render with a signed query and a bake between its tyr_render calls: the same accumulation buffer and counters"""
    def between(g):
        rng = np.random.default_rng(73)
        pts = np.stack([rng.uniform(-40, 40, 5000), rng.uniform(-40, 40, 5000), rng.uniform(5, 80, 5000)], axis=1).astype(F)
        sd = g.query_signed(pts)[0]
        grid = g.bake_sdf((-40.0, -40.0, 0.0), 2.0, (40, 40, 40), 3.0)
        assert bool(sd.isfinite().all()) and bool(grid.isfinite().all())

    assert_render_undisturbed(between, flags=(0, WINDING, WINDING))


@pytest.mark.gpu
def test_invalid_arguments(hip):
    """bad arguments are refused before any launch and write nothing; a ctx without TYR_FLAG_WINDING and a ctx without a scene say so"""
    import torch

    nodes, prims, pts, _ = family("cube")
    g = renderer(hip, nodes, prims, flags=WINDING)
    L, h, P = hip.lib(), g.h, C.c_void_p
    n = 64
    tp = torch.from_numpy(pts[:n].copy()).cuda()
    sd = torch.full((4096,), 7.0).cuda()
    torch.cuda.synchronize()
    ok = hip.SignedOut(sd.data_ptr(), None, None, None, None)
    pp = P(tp.data_ptr())
    inv, nan = hip.TYR_ERR_INVALID, float("nan")
    call = L.tyr_query_signed
    assert call(None, n, pp, None, 2.0, 0, C.byref(ok), None) == inv
    assert call(h, n, None, None, 2.0, 0, C.byref(ok), None) == inv
    assert call(h, n, pp, None, 2.0, 0, None, None) == inv
    assert call(h, n, pp, None, 2.0, 0, C.byref(hip.SignedOut(None, None, None, None, None)), None) == inv
    assert call(h, n, pp, None, 2.0, 1, C.byref(ok), None) == inv  # flags must be 0
    assert call(h, n, pp, None, nan, 0, C.byref(ok), None) == inv
    assert call(h, n, pp, None, -1.0, 0, C.byref(ok), None) == inv
    assert call(h, 1 << 31, pp, None, 2.0, 0, C.byref(ok), None) == inv
    assert call(h, 0, None, None, 2.0, 0, None, None) == 0  # n == 0: nothing to do
    gout = hip.SdfOut(sd.data_ptr(), None, None)

    def grid(origin=(0.0, 0.0, 0.0), cell=1.0, dims=(8, 8, 8), band=1.0, accuracy=2.0):
        return hip.SdfGrid((C.c_float * 3)(*origin), cell, (C.c_uint32 * 3)(*dims), band, accuracy)

    bake = L.tyr_bake_sdf
    assert bake(None, C.byref(grid()), 0, C.byref(gout), None) == inv
    assert bake(h, None, 0, C.byref(gout), None) == inv
    assert bake(h, C.byref(grid()), 0, None, None) == inv
    assert bake(h, C.byref(grid()), 0, C.byref(hip.SdfOut(None, None, None)), None) == inv
    assert bake(h, C.byref(grid()), 1, C.byref(gout), None) == inv
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=INF), dict(band=0.0), dict(band=-1.0), dict(band=nan), dict(band=INF), dict(origin=(0.0, nan, 0.0)),
                dict(origin=(INF, 0.0, 0.0)), dict(dims=(0, 8, 8)), dict(dims=(8, 8, 0)), dict(dims=(2048, 1024, 1024)), dict(dims=(65536, 65536, 65536)), dict(accuracy=nan),
                dict(accuracy=-2.0)):
        assert bake(h, C.byref(grid(**bad)), 0, C.byref(gout), None) == inv, bad
    assert g.query_error() == 0
    assert (sd.cpu().numpy() == 7).all()  # the refused calls wrote nothing
    assert bake(h, C.byref(grid()), 0, C.byref(gout), None) == 0 and g.query_error() == 0
    assert (sd.cpu().numpy()[:512] != 7).all() and (sd.cpu().numpy()[512:] == 7).all()
    plain = renderer(hip, nodes, prims)  # no TYR_FLAG_WINDING
    assert call(plain.h, n, pp, None, 2.0, 0, C.byref(ok), None) == hip.TYR_ERR_UNSUPPORTED
    assert bake(plain.h, C.byref(grid()), 0, C.byref(gout), None) == hip.TYR_ERR_UNSUPPORTED
    plain.close()
    empty = hip.Renderer(64, 64, 1024, flags=WINDING)  # no scene uploaded
    assert call(empty.h, n, pp, None, 2.0, 0, C.byref(ok), None) == hip.TYR_ERR_NO_SCENE
    assert bake(empty.h, C.byref(grid()), 0, C.byref(gout), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_signed(tp.double())
    with pytest.raises(ValueError):
        g.query_signed(tp, torch.ones(5).cuda())
    with pytest.raises(hip.TyrError):
        g.bake_sdf((0, 0, 0), 1.0, (0, 4, 4), 1.0)
    # the list of near bricks is the ctx's and counted once a bake has run
    fresh = renderer(hip, nodes, prims, flags=WINDING)
    assert g.scene_info()["device_bytes"] > fresh.scene_info()["device_bytes"]
    fresh.close()
    g.close()


@pytest.mark.gpu
def test_c3_tree(hip):
    """C3's 1 M-triangle tree against tests/golden/signed_c3.npz (tools/signed_c3_golden.py: the restatement's answers): 256 points
    near the surface, a quarter of them with a bound, and a 16^3 window of a bake that holds near and far bricks.  Every run checks
    that the file belongs to these triangles, that the recorded answers obey the join, and recomputes one point's closest triangle
    by brute force."""
    sc, nodes, prims = built_scene("mesh706")
    z = np.load(C3_ANSWERS)
    assert str(z["digest"]) == hashlib.sha256(np.ascontiguousarray(prims).tobytes()).hexdigest(), "the recorded answers belong to other triangles"
    pts, md = z["points"], z["max_dist"]
    want = tuple(z[k] for k in NAMES)
    assert len(pts) == 256 and (want[1] >= 0).sum() >= 128 and (want[1] < 0).sum() >= 16
    assert want[4].min() < -1.2 and want[4].max() > 0.1 and not (want[0] < 0).any()  # (a room seen from inside: w from -1.5 to 0.15, no point counts as inside)
    live = int(np.random.default_rng(74).integers(0, 256))
    d2, pr, _, _, pt = nearest_ref.nearest(pts[live:live + 1], prims, md[live:live + 1])
    assert int(pr[0]) == int(want[1][live])
    won = want[1] >= 0
    val, _, _, _, c = nearest_ref.pair_value(pts[won], *(a[want[1][won]] for a in nearest_ref.records(prims)))
    dist2 = np.where(won, 0, md * md).astype(F)
    dist2[won] = val
    point = pts.copy()
    point[won] = c
    same(ref.join(pts, md, dist2, want[1], point, want[4], prims), want, "the recorded answers against the join")
    grid = (tuple(float(x) for x in z["origin"]), float(z["cell"]), tuple(int(d) for d in z["dims"]), float(z["band"]))
    gsd, gprim, gstats = z["grid_sd"], z["grid_prim"], z["grid_stats"]
    assert gsd.shape == (16, 16, 16) and gstats[0] > 0 and gstats[1] > 0
    g = renderer(hip, nodes, prims, flags=WINDING)
    same(ask(g, pts, md), want, "C3 points")
    same_grid(ask_grid(g, grid), (gsd, gprim, gstats), "C3 window")
    assert g.query_error() == 0
    g.close()
