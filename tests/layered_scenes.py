"""Scenes and ray sets for the tests of the visit-order rule (tests/test_visit_order.py, tests/golden/make_golden.py).

bvh.h:134 accepts a triangle hit only when `t > epsilon && t < dist && (dist - t) > epsilon` (epsilon = 1e-3): of two
surfaces less than epsilon apart along a ray the one TESTED FIRST wins, even if the other is nearer.  Closest hit is a left
fold over the triangle tests in the reference's visit order, and only geometry with several surfaces within epsilon of each
other can tell a traversal that keeps that order from one that returns the nearest hit.  `layered` makes such geometry from
any scene: copies of every triangle moved by less than, about and more than epsilon along a random direction per copy.

A helper module (no tests, no fixtures): everything here is a pure function of its arguments and seeds.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tyrant_amd import scenes

EPSILON = np.float32(1e-3)  # variables.h:14
VERY_FAR = np.float32(1e20)
# below, at and above epsilon; the two zeros are exact duplicates of each other
OFFSETS = (0.0, 0.0, 2e-4, 5e-4, 9e-4, 1.0e-3, 1.1e-3, 1.6e-3, 2.5e-3)
# every camera ray enters the room (from the Cornell camera 85 % of a frame misses the tree, and the rest meets the layers at
# a grazing angle, where few of them lie within epsilon of each other along the ray)
CAMERA = scenes.FRAMED_CAMERA


def layered(base_triangles: np.ndarray, offsets, seed: int) -> np.ndarray:
    """for each offset a copy of every base triangle, its three vertices moved by offset * u_k (u_k: a seeded random unit
    vector per copy, so the layers are parallel to no coordinate plane and cross each other); materials and pad_ copied"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(len(offsets), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v0 = base_triangles["vert"].astype(np.float64)
    v1 = v0 + base_triangles["e1"].astype(np.float64)
    v2 = v0 + base_triangles["e2"].astype(np.float64)
    out = []
    for off, uk in zip(offsets, u):
        s = float(off) * uk
        t = scenes.make_triangles(v0 + s, v1 + s, v2 + s, base_triangles["materialType"])
        t["pad_"] = base_triangles["pad_"]
        out.append(t)
    return np.concatenate(out)


def _six_plane_stack(x0: float, copies: int, rng) -> np.ndarray:
    """the 60 x 60 "stack" triangle of the long-leaf tests with its three vertices' y drawn from STACK_Y + {0, 2e-3}, not all equal:
    six different planes through ONE bounding box (one centroid: the builder cannot split them), `copies` of each, shuffled"""
    ys = [(a, b, c) for a in (0.0, 2e-3) for b in (0.0, 2e-3) for c in (0.0, 2e-3) if not a == b == c]
    ys = np.array(ys * copies) + STACK_Y
    ys = ys[rng.permutation(len(ys))]
    n = len(ys)
    v0 = np.stack([np.full(n, x0 - 30.0), ys[:, 0], np.full(n, 10.0)], axis=1)
    v1 = np.stack([np.full(n, x0 + 30.0), ys[:, 1], np.full(n, 10.0)], axis=1)
    v2 = np.stack([np.full(n, x0), ys[:, 2], np.full(n, 70.0)], axis=1)
    return scenes.make_triangles(v0, v1, v2)


STACK_Y = -40.0  # in front of the Cornell box's two boxes, which would hide half of a stack at y = 0
STACKS = ((-10.0, 4), (15.0, 12))  # (x0, copies of each of the six planes): leaves of 24 and of 72 triangles


def _long_leaves() -> scenes.SceneData:
    rng = np.random.default_rng(31)
    tris = np.concatenate([scenes.cornell_box().triangles] + [_six_plane_stack(x0, c, rng) for x0, c in STACKS])
    return scenes.SceneData("layered_long_leaves", tris, scenes.cornell_spheres(), CAMERA)


def _materials() -> scenes.SceneData:
    """neighbouring layers differ in material: a wrong winner changes the path (mirror / glass / diffuse / emitter)"""
    base = scenes.mesh_scene(16, seed=99, spec_fraction=0.0).triangles
    n = len(base)
    tris = layered(base, OFFSETS, 0x1A7E)
    cycle = (scenes.DIFF, scenes.SPEC, scenes.REFR, scenes.DIFF, scenes.SPEC, scenes.LIGHT, scenes.REFR, scenes.DIFF, scenes.SPEC)
    for k, m in enumerate(cycle):
        mat = np.full(n, m, dtype=np.uint8)
        if m == scenes.LIGHT:  # a whole emissive layer would drown the rest: one triangle in sixteen of it emits
            mat[scenes.hash_unit(np.arange(n, dtype=np.uint64), 4242) >= 1.0 / 16.0] = scenes.DIFF
        tris["materialType"][k * n : (k + 1) * n] = mat
    return scenes.SceneData("layered_materials", tris, scenes.cornell_spheres(), CAMERA, triangle_materials=True, light_list=True, triangle_emission=(4.0, 3.5, 3.0))


def _plain(name, base: scenes.SceneData, offsets, seed) -> scenes.SceneData:
    return dataclasses.replace(base, name=name, triangles=layered(base.triangles, offsets, seed), camera=CAMERA)


MAKERS = {
    "layered_mesh24": lambda: _plain("layered_mesh24", scenes.mesh_scene(24), OFFSETS, 0x1A7E),
    "layered_soup300": lambda: _plain("layered_soup300", scenes.cornell_soup(300), OFFSETS, 0x1A7E),
    "layered_mesh128": lambda: _plain("layered_mesh128", scenes.mesh_scene(128), OFFSETS, 0x1A7E),
    "layered_dup6": lambda: _plain("layered_dup6", scenes.mesh_scene(10), (0.0,) * 6, 6),
    "layered_dup24": lambda: _plain("layered_dup24", scenes.mesh_scene(10), (0.0,) * 24, 24),
    "layered_long_leaves": _long_leaves,
    "layered_materials": _materials,
    # layered_mesh24's tree shape with every layer at offset 0 (nine exact copies): the scene the refit test uploads first
    "layered_mesh24_flat": lambda: _plain("layered_mesh24_flat", scenes.mesh_scene(24), (0.0,) * len(OFFSETS), 24),
}
SMALL = ("layered_mesh24", "layered_soup300", "layered_long_leaves", "layered_materials")
DUPS = ("layered_dup6", "layered_dup24")


@functools.lru_cache(maxsize=None)
def built_layered(name: str):
    """(scene, nodes, prims) with the tree built by the oracle's builder, as conftest.built_scene does"""
    from oracle import pyorc

    sc = MAKERS[name]()
    nodes, prims = pyorc.bvh_build(sc.triangles, scenes.triangle_bboxes(sc.triangles))
    return sc, nodes, prims


def scene_flags(sc) -> int:
    return (1 if sc.triangle_materials else 0) | (8 if sc.light_list else 0) | (16 if sc.triangle_colors else 0)


# ---- ray sets -----------------------------------------------------------------------------------------------------------
def random_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def octant(d: np.ndarray) -> np.ndarray:
    """0..7 from the signs of 1/d as the traversal sees them (dirIsNeg, bvh.h:121)"""
    with np.errstate(divide="ignore"):
        inv = np.float32(1) / d.astype(np.float32)
    return (inv[:, 0] < 0).astype(np.int32) | ((inv[:, 1] < 0).astype(np.int32) << 1) | ((inv[:, 2] < 0).astype(np.int32) << 2)


def ray_set(sc, nodes, n: int, seed: int):
    """(origins, directions): random origins in the root box with random directions, camera rays, rays dealt evenly to the
    eight direction octants, and -- mixed into the same waves -- axis-aligned and zero-component directions"""
    rng = np.random.default_rng(seed)
    lo, hi = nodes[0]["bounds"][0].astype(np.float64), nodes[0]["bounds"][1].astype(np.float64)
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = random_dirs(rng, n)
    kind = rng.random(n)
    cam = kind < 0.2
    o[cam] = np.asarray(sc.camera.position, dtype=np.float32)
    dc = np.asarray(sc.camera.direction) * 1.5 + rng.uniform(-0.75, 0.75, size=(int(cam.sum()), 3))
    d[cam] = (dc / np.linalg.norm(dc, axis=1, keepdims=True)).astype(np.float32)
    dealt = (kind >= 0.2) & (kind < 0.55)  # octant k = i % 8: no octant is left to chance
    k = np.arange(n) % 8
    sign = np.stack([np.where(k & 1, -1.0, 1.0), np.where(k & 2, -1.0, 1.0), np.where(k & 4, -1.0, 1.0)], axis=1).astype(np.float32)
    d[dealt] = (np.abs(d) * sign)[dealt]
    zero = (kind >= 0.55) & (kind < 0.7)  # one or two zero components (1/d infinite: the generic box test)
    z = rng.random((n, 3)) < 0.45
    z[z.all(axis=1), 0] = False
    dz = np.where(z, np.float32(0), d)
    dz = (dz / np.maximum(np.linalg.norm(dz, axis=1, keepdims=True), 1e-30)).astype(np.float32)
    d[zero] = dz[zero]
    return o, d


def stack_rays(n: int, seed: int):
    """rays aimed at layered_long_leaves' two stacks from in front of them (a tenth elsewhere into the room)"""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, len(STACKS), n)
    x0 = np.array([s[0] for s in STACKS])[which]
    o = np.stack([rng.uniform(-45, 45, n), rng.uniform(-140, -55, n), rng.uniform(2, 98, n)], axis=1)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)  # a point of the stack triangle (x0 - 30, y, 10), (x0 + 30, y, 10), (x0, y, 70)
    target = np.stack([x0 - 30.0 * w[:, 0] + 30.0 * w[:, 1], np.full(n, STACK_Y + 1e-3), 10.0 + 60.0 * w[:, 2]], axis=1)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    stray = rng.random(n) < 0.1
    d[stray] = random_dirs(rng, int(stray.sum()))
    axis = rng.random(n) < 0.1  # straight at the stacks: two zero components
    o[axis, 0] = target[axis, 0]
    o[axis, 2] = target[axis, 2]
    d[axis] = np.float32([0, 1, 0])
    return o.astype(np.float32), d


def secondary(o, d, t, hit, seed: int):
    """rays that start ON the surfaces the first pass hit: origins o + t d (float32, one rounding per operation), new random
    directions -- the other layers lie within epsilon of such an origin (the `t > epsilon` edge)"""
    rng = np.random.default_rng(seed)
    o2 = (o[hit] + (d[hit] * t[hit, None]).astype(np.float32)).astype(np.float32)
    return o2, random_dirs(rng, o2.shape[0])


def reorder(o, d, how: str, seed: int = 0):
    """the permutation that puts the rays in `how` order: "shuffled", or "sorted" (by octant, then by origin cell) -- the
    composition of the waves changes what the wide drain and the packed leaf rounds see; the answers must not"""
    n = o.shape[0]
    if how == "shuffled":
        return np.random.default_rng(seed).permutation(n)
    cell = np.floor(o.astype(np.float64) / 12.5).astype(np.int64)
    return np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2], octant(d)))


def ulp_step(x: np.ndarray, k: int) -> np.ndarray:
    """positive finite float32 x moved by k units in the last place"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.int32) + np.int32(k)).view(np.float32)


def tmax_sweep(t_star: np.ndarray):
    """{k: float32(t* + epsilon) moved by k ulp} for k = -2 .. +2: the `(dist - t) > epsilon` edge of the accept rule"""
    base = (t_star.astype(np.float32) + EPSILON).astype(np.float32)
    return {k: ulp_step(base, k) for k in (-2, -1, 0, 1, 2)}


# ---- the oracle's answers -----------------------------------------------------------------------------------------------
def tree_closest(orc, nodes, prims, o, d, tmax=None):
    """(t, prim or -1) of the ORACLE's CachedBVH::intersect restatement with ray.distance = tmax (default VERY_FAR)"""
    n = o.shape[0]
    r = np.zeros(n, dtype=scenes.RAY_DTYPE)
    r["origin"], r["direction"], r["identifier"] = o, d, -1
    r["distance"] = VERY_FAR if tmax is None else tmax
    hit = np.zeros(n, dtype=np.int32)
    nodes, prims = np.ascontiguousarray(nodes), np.ascontiguousarray(prims)
    orc.lib().orc_bvh_intersect_batch(nodes.ctypes.data, prims.ctypes.data, r.ctypes.data, n, hit.ctypes.data)
    return r["distance"].copy(), np.where(hit != 0, r["identifier"], -1).astype(np.int32)


def tree_any(orc, nodes, prims, o, d, tmax):
    """the ORACLE's intersectSimple(ray, closestAllowed = tmax)"""
    n = o.shape[0]
    s = np.zeros(n, dtype=scenes.SHADOW_DTYPE)
    s["origin"], s["direction"], s["closestDistance"] = o, d, tmax
    nodes, prims = np.ascontiguousarray(nodes), np.ascontiguousarray(prims)
    f = orc.lib().orc_bvh_intersect_simple
    pn, pp, base, size = nodes.ctypes.data, prims.ctypes.data, s.ctypes.data, s.dtype.itemsize
    tm = s["closestDistance"]
    return np.array([f(pn, pp, base + i * size, float(tm[i]), None) for i in range(n)], dtype=np.int32) != 0


def order_sensitive(orc, prims, o, d, t, prim, tmax=None):
    """rays whose tree answer (distance bits or triangle) is not the nearest accepted hit of the order-free comparator"""
    bt, bp = orc.brute_closest(prims, o, d, VERY_FAR if tmax is None else tmax)
    return (bt.view(np.uint32) != np.ascontiguousarray(t, dtype=np.float32).view(np.uint32)) | (bp != prim)
