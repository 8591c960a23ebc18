"""Every query-like entry under every shape of the scene its ctx can hand it, bit for bit against the entry's restatement.

A query takes its scene from launch_scene (host/driver.cpp): nStaged = min(the tree's staged records, TYR_TUNE_STAGED_NODES).
That count decides, at every step of every descent, which tail of the node fetch runs: `idx < nStaged` reads the block's
vector-major LDS copy through an explicit address-space-3 pointer, everything else reads the quad array in HBM.  The fetch is
written out in one place, fetch_quad in hip/traverse.hpp, and every kernel family reaches it through its own descent -- the
keyed descent (nearest, nearest_k, sweep, segment), the overlap descent (box, tri) and test_quad behind the ray descent (hits;
closest / any with and without spheres, occlusion, the AOV and chain kernels) -- with its own key, slot test and push order
behind it; q_stage_nodes fills the LDS copy from the same count.  The entries' own modules only ever run at
nStaged = min(64, quads in the tree).

Why a wrong fetch cannot pass here.  Which fetch a shape forces:
  staged0      no record is in LDS: every node, the root included, comes from HBM, and q_stage_nodes copies nothing.  A kernel
               that compares with the constant 64 instead of the count reads LDS nobody filled; a root that is wrong only
               from HBM is wrong for every item.
  staged1      the root alone comes from LDS, its children from HBM: the first step of every descent crosses from one tail of
               the fetch to the other, so a push order or a record layout that differs between the tails shows at once.
  staged2, 7   the crossing moves down the breadth-first top; 7 is no multiple of the 4 children of a quad, so siblings of
               one parent lie on both sides of it.
  staged_last  one record short of what the tree staged: the last LDS slot is the one that moves to HBM.
  staged64     today's case, the control.
On the small trees (the whole tree fits in LDS) every count below the tree's is the TUNING's limit, not the tree's: records that
every earlier test read from LDS now come from HBM, and the staging loop runs for a count the tree did not choose.  On the large
trees every shape mixes both fetches in one descent.  The staged shapes run on ONE live ctx with tyr_set_tuning between calls
(launch_scene reads the key at every launch: the answer must follow it without a new upload), and staged0 / staged7 again set
before the upload of a fresh ctx.  layout_host / layout_device (layout_on_device 0 / 1 before the upload) and counting
(TYR_FLAG_COUNT_VISITS: pair nodes beside the quads, the upload takes the host pass) change who wrote the quad array the
fetches read.  The inputs are held to conditions checked on the restatement alone (test_restatements_answer_enough): enough
items have an answer, enough have none, and on the large trees the winners are spread over the primitives, so descents reach
the HBM part of the tree and an empty answer cannot hide a fetch that finds nothing.

What each entry is compared with is its own module's restatement, computed once per (entry, fixture) and shared by all shapes --
never the device's answer at another shape.  tyr_query_winding is left out: k_winding walks its own moment tree and never reads
nStaged.  tyr_render_motion_chain walks no tree either (hip/temporal.hip); it is run on each shape's chain guides with the
current camera as the previous one, where its answer is exact: no motion anywhere, and a previous depth of VERY_FAR exactly
where the restatement's chain left the scene."""
import dataclasses
import functools

import numpy as np
import pytest

import aov_ref
import box_ref
import hits_ref
import nearest_k_ref
import nearest_ref
import occlusion_ref
import ray_ref
import segment_ref
import specular_ref
import sweep_ref
import tri_ref
from query_support import box_points, lattice, renderer, same, surface_points, unit

F = np.float32
U = np.uint32
VERY_FAR = aov_ref.VERY_FAR
TYR_FLAG_COUNT_VISITS = 4
# the trees: lattice(cells, seed), and how many items a call has (more than one block of 256, a ragged last wave)
TREES = {"small": (8, 81, 325), "large": (16, 82, 1349)}
# the guide passes' items are the pixels of a GUIDE_W x GUIDE_H frame (1872 = 29 * 64 + 16), seen from 60 in front of the room's
# opening: the room fills 100 of the frame's 130 columns, the columns beside it see nothing
GUIDE_W, GUIDE_H = 52, 36
GUIDE_SCENES = {"cornell": "cornell36", "mesh128": "mesh128"}
MAX_CHAIN = 4
STAGED = {"staged0": 0, "staged1": 1, "staged2": 2, "staged7": 7, "staged_last": None, "staged64": 64}  # (None: the tree's count - 1)
BEFORE_UPLOAD = ("staged0", "staged7")
FRESH = {"layout_host": dict(layout_on_device=0), "layout_device": dict(layout_on_device=1), "counting": dict(flags=TYR_FLAG_COUNT_VISITS)}


def _orc():
    from oracle import pyorc

    pyorc.lib()
    return pyorc


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- fixtures (numpy only; made once, never changed) --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tree(fixture):
    """(nodes, prims) of a lattice fixture"""
    cells, seed, _ = TREES[fixture]
    return lattice(cells, seed)[:2]


def items_of(fixture):
    return TREES[fixture][2]


def rng_of(fixture, salt):
    return np.random.default_rng([TREES[fixture][1], salt])


@functools.lru_cache(maxsize=None)
def spheres():
    """the sphere table of tests/test_ray_query.py's sphere test: two spheres within reach, the ground sphere, the others parked"""
    from tyrant_amd import scenes

    s = scenes.cornell_spheres()
    s[2] = (6.0, (-10.0, 0.0, 30.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), scenes.DIFF)
    s[5] = (8.0, (12.0, 20.0, 40.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), scenes.DIFF)
    return frozen(s)[0]


@functools.lru_cache(maxsize=None)
def guide_scene(fixture):
    """(scene, nodes, prims) of a guide-pass fixture, the tree by the oracle's builder as in tests/test_aov.py"""
    from conftest import built_scene
    from tyrant_amd import scenes

    sc, nodes, prims = built_scene(GUIDE_SCENES[fixture])
    cam = dataclasses.replace(scenes.CORNELL_CAMERA, position=(0.0, -110.0, 50.0))
    return dataclasses.replace(sc, camera=cam), nodes, prims


def down_rays(fixture, salt, reach):
    """rays from z = 40 above seeded points of the surface downwards, tilted, with a seeded reach: the surface lies 5 .. 31
    below, so a ray stops short of it or not"""
    n = items_of(fixture)
    rng = rng_of(fixture, salt)
    o = surface_points(rng, tree(fixture)[1], n, 0.0)
    o[:, 2] = 40.0
    d = unit(np.concatenate([rng.normal(size=(n, 2)) * 0.3, np.full((n, 1), -1.0)], axis=1))
    return o, d, rng.uniform(*reach, n).astype(F)


def aimed(fixture, salt, reach):
    """(start, displacement): from the inflated root box towards points near the surface, some stopping short, some passing through"""
    n = items_of(fixture)
    rng = rng_of(fixture, salt)
    prims = tree(fixture)[1]
    p = box_points(rng, prims, n)
    target = surface_points(rng, prims, n, 0.5)
    return p, ((target - p) * rng.uniform(*reach, (n, 1))).astype(F)


def near_and_far(fixture, salt, noise):
    """(the generator, centres): seven in ten near the surface, the others anywhere in the inflated root box"""
    n = items_of(fixture)
    rng = rng_of(fixture, salt)
    prims = tree(fixture)[1]
    near = n * 7 // 10
    return rng, np.concatenate([surface_points(rng, prims, near, noise), box_points(rng, prims, n - near)])


@functools.lru_cache(maxsize=None)
def ray_items(fixture):
    return frozen(*down_rays(fixture, 1, (2.0, 45.0)))


@functools.lru_cache(maxsize=None)
def hit_items(fixture):
    """every second ray comes down onto the surface, the others skim through it from inside the root box"""
    o, d, tmax = down_rays(fixture, 2, (2.0, 90.0))
    rng = rng_of(fixture, 3)
    skim = np.arange(len(o)) % 2 == 1
    m = int(skim.sum())
    o[skim] = box_points(rng, tree(fixture)[1], m)
    d[skim] = unit(rng.normal(size=(m, 3)) * np.array([1.0, 1.0, 0.25]))
    tmax[skim] = rng.uniform(20.0, 150.0, m).astype(F)
    return frozen(o, d, tmax)


@functools.lru_cache(maxsize=None)
def point_items(fixture, salt, noise, bound):
    """(points of the surface moved by `noise`, a max_dist of `bound` each)"""
    n = items_of(fixture)
    return frozen(surface_points(rng_of(fixture, salt), tree(fixture)[1], n, noise), np.full(n, bound, F))


@functools.lru_cache(maxsize=None)
def occlusion_items(fixture):
    """points on the surface, their normals tilted off the vertical so that a hemisphere dips into the terrain"""
    n = items_of(fixture)
    rng = rng_of(fixture, 6)
    p = surface_points(rng, tree(fixture)[1], n, 0.0)
    return frozen(p, unit(np.array([0.0, 0.0, 1.0]) + rng.normal(size=(n, 3)) * 0.7))


@functools.lru_cache(maxsize=None)
def sweep_items(fixture):
    return frozen(*aimed(fixture, 7, (0.3, 1.7)))


@functools.lru_cache(maxsize=None)
def box_items(fixture):
    rng, c = near_and_far(fixture, 8, 1.0)
    half = (10.0 ** rng.uniform(-1.0, 0.5, c.shape)).astype(F)
    return frozen((c - half).astype(F), (c + half).astype(F))


@functools.lru_cache(maxsize=None)
def tri_items(fixture):
    rng, c = near_and_far(fixture, 9, 1.0)
    return frozen(*((c + rng.normal(size=c.shape) * 1.5).astype(F) for _ in range(3)))


@functools.lru_cache(maxsize=None)
def own_triangles(fixture):
    """the mesh's own triangles as queries, every second one with its corner C moved 20 along x and y, across the terrain: with skip_shared the
    first kind touches nothing (all it touches shares a corner with it), the second what it crosses farther away"""
    prims = tree(fixture)[1]
    pick = rng_of(fixture, 10).integers(0, len(prims), items_of(fixture))
    a, b, c = (x[pick].astype(F) for x in tri_ref.corners(*tri_ref.records(prims)))
    c[1::2] += np.array([20.0, 20.0, 0.0], F)
    return frozen(a, b, c)


@functools.lru_cache(maxsize=None)
def segment_items(fixture):
    p, d = aimed(fixture, 11, (0.2, 1.1))
    return frozen(p, (p + d).astype(F))


# ---- the entries --------------------------------------------------------------------------------------------------------
# An entry: the fixtures it runs on; cases: label -> (the outputs' names, ask(g, fixture) -> the device's outputs as numpy arrays,
# want(fixture) -> the restatement's); answered(wants) -> which items have a non-empty answer; winners(wants) -> the primitive
# indices answered (None: the entry reports none).
@dataclasses.dataclass(frozen=True)
class Entry:
    fixtures: tuple
    cases: dict
    answered: object
    winners: object = None


LATTICES = ("small", "large")
GUIDES = ("cornell", "mesh128")
ENTRIES = {}


def as_numpy(res):
    return tuple(None if x is None else x.cpu().numpy() for x in res)


def args(*arrays):
    """the fixtures' arrays are read-only: torch wants its own"""
    return tuple(np.array(a) for a in arrays)


# closest / any: the oracle, as tests/test_ray_query.py asks it
def want_closest(with_spheres):
    def want(fixture):
        o, d, tmax = ray_items(fixture)
        nodes, prims = tree(fixture)
        orc = _orc()
        if with_spheres:
            t, prim, geom = ray_ref.oracle_spheres_closest(orc, spheres(), nodes, prims, o, d, tmax)
        else:
            t, prim = ray_ref.oracle_closest(orc, nodes, prims, o, d, tmax)
            geom = np.where(prim >= 0, 1, -1).astype(np.int32)
        uv = np.zeros((len(o), 2), F)
        on = geom == 1
        uv[on, 0], uv[on, 1] = ray_ref.glm_uv(orc, prims, prim[on], o[on], d[on])
        return t.astype(F), prim.astype(np.int32), geom, uv

    return want


def want_any(with_spheres):
    def want(fixture):
        o, d, tmax = ray_items(fixture)
        nodes, prims = tree(fixture)
        if with_spheres:
            return (ray_ref.oracle_spheres_any(_orc(), spheres(), nodes, prims, o, d, tmax),)
        return (ray_ref.oracle_any(_orc(), nodes, prims, o, d, tmax),)

    return want


CLOSEST_NAMES = ("t", "prim", "geom", "uv")
ENTRIES["closest"] = Entry(LATTICES, {
    "tree": (CLOSEST_NAMES, lambda g, f: as_numpy(g.query_closest(*args(*ray_items(f)))), want_closest(False)),
    "spheres": (CLOSEST_NAMES, lambda g, f: as_numpy(g.query_closest(*args(*ray_items(f)), spheres=True)), want_closest(True)),
}, lambda w: w["tree"][1] >= 0, lambda w: w["tree"][1][w["tree"][1] >= 0])
ENTRIES["any"] = Entry(LATTICES, {
    "tree": (("occluded",), lambda g, f: as_numpy((g.query_any(*args(*ray_items(f))),)), want_any(False)),
    "spheres": (("occluded",), lambda g, f: as_numpy((g.query_any(*args(*ray_items(f)), spheres=True),)), want_any(True)),
}, lambda w: w["tree"][0])


# hits: one Hits per sidedness answers for every max_hits
@functools.lru_cache(maxsize=None)
def all_hits(fixture, two_sided):
    return hits_ref.Hits(*hit_items(fixture)[:2], *tree(fixture), hit_items(fixture)[2], two_sided)


def ask_hits(k, two_sided):
    def ask(g, fixture):
        res = as_numpy(g.query_hits(*args(*hit_items(fixture)), max_hits=k, two_sided=two_sided))
        return (res[0].view(U),) + res[1:5] + (res[5].view(U),)

    return ask


HIT_NAMES = ("count", "t", "prim", "uv", "side", "back_count")
ENTRIES["hits"] = Entry(LATTICES, {
    f"{'two' if two else 'one'}-sided max_hits {k}": (HIT_NAMES, ask_hits(k, two), lambda f, k=k, two=two: all_hits(f, two).answer(k)) for two in (False, True) for k in (1, 8)
}, lambda w: w["one-sided max_hits 8"][0] > 0, lambda w: w["two-sided max_hits 8"][2][w["two-sided max_hits 8"][2] >= 0])


# nearest / nearest_k: noise of 3 round the surface; a bound of 4 (nearest) and of 3.5 (nearest_k) leaves some points without
def nearest_points(f):
    return point_items(f, 4, 3.0, 4.0)


def nearest_k_points(f):
    return point_items(f, 5, 3.0, 3.5)


def ask_nearest_k(k):
    def ask(g, fixture):
        p, md = args(*nearest_k_points(fixture))
        res = as_numpy(g.query_nearest_k(p, k, md, count=True))
        return res[:5] + (res[5].astype(np.int64),)

    return ask


NEAREST_NAMES = ("dist2", "prim", "uv", "region", "point")
ENTRIES["nearest"] = Entry(LATTICES, {
    "unbounded": (NEAREST_NAMES, lambda g, f: as_numpy(g.query_nearest(*args(nearest_points(f)[0]))), lambda f: nearest_ref.nearest(nearest_points(f)[0], tree(f)[1])),
    "max_dist 4": (NEAREST_NAMES, lambda g, f: as_numpy(g.query_nearest(*args(*nearest_points(f)))), lambda f: nearest_ref.nearest(nearest_points(f)[0], tree(f)[1], nearest_points(f)[1])),
}, lambda w: w["max_dist 4"][1] >= 0, lambda w: w["unbounded"][1])
ENTRIES["nearest_k"] = Entry(LATTICES, {
    f"k {k} with count, max_dist 3.5": (NEAREST_NAMES + ("count",), ask_nearest_k(k), lambda f, k=k: nearest_k_ref.nearest_k(nearest_k_points(f)[0], tree(f)[1], k, nearest_k_points(f)[1]))
    for k in (1, 8)
}, lambda w: w["k 8 with count, max_dist 3.5"][1][:, 0] >= 0, lambda w: w["k 8 with count, max_dist 3.5"][1][w["k 8 with count, max_dist 3.5"][1] >= 0])


# occlusion: an item has an answer where something blocks one of its samples
SEED = 0x9E3779B9


def ask_occlusion(g, fixture):
    res = as_numpy(g.query_occlusion(*args(*occlusion_items(fixture)), samples=8, seed=SEED, mask=True, bent=True))
    return tuple(None if x is None else (x.view(U) if x.dtype == np.int32 else x) for x in res)


ENTRIES["occlusion"] = Entry(LATTICES, {
    "8 samples, mask and bent": (("visible", "mask", "bent", "origin", "direction"), ask_occlusion, lambda f: occlusion_ref.occlusion(*tree(f), *occlusion_items(f), 8, seed=SEED)),
}, lambda w: w["8 samples, mask and bent"][0] < 8)


SWEEP_NAMES = ("t", "prim", "region", "point", "center", "normal")
ENTRIES["sweep"] = Entry(LATTICES, {
    f"radius {r}": (SWEEP_NAMES, lambda g, f, r=r: as_numpy(g.query_sweep(*args(*sweep_items(f)), r, normal=True)), lambda f, r=r: sweep_ref.sweep(*sweep_items(f), r, tree(f)[1])) for r in (0.0, 1.5)
}, lambda w: w["radius 0.0"][1] >= 0, lambda w: w["radius 0.0"][1][w["radius 0.0"][1] >= 0])


# box / tri: a count alone, a row of 8, ANY; tri also with skip_shared on the mesh's own triangles
def member_cases(query, items, ref, tag="", **kw):
    def ask(g, fixture, k=0, **more):
        res = query(g)(*args(*items(fixture)), max_prims=k, **more, **kw)
        return as_numpy(res if k else (res,))

    return {
        f"{tag}count": (("count",), ask, lambda f: ref(*items(f), tree(f)[1], **kw)[:1]),
        f"{tag}max_prims 8": (("count", "prim"), functools.partial(ask, k=8), lambda f: ref(*items(f), tree(f)[1], 8, **kw)),
        f"{tag}any": (("any",), functools.partial(ask, any=True), lambda f: (ref(*items(f), tree(f)[1], any=True, **kw),)),
    }


def members_of(w):
    return w["max_prims 8"][1][w["max_prims 8"][1] >= 0]


ENTRIES["box"] = Entry(LATTICES, member_cases(lambda g: g.query_box, box_items, box_ref.box), lambda w: w["count"][0] > 0, members_of)
ENTRIES["tri"] = Entry(LATTICES, {
    **member_cases(lambda g: g.query_tri, tri_items, tri_ref.tri),
    **member_cases(lambda g: g.query_tri, own_triangles, tri_ref.tri, tag="its own triangles, skip_shared, ", skip_shared=True),
}, lambda w: w["count"][0] > 0, members_of)


# segment: a bound of 2 leaves some segments without
ENTRIES["segment"] = Entry(LATTICES, {
    "unbounded": (segment_ref.NAMES, lambda g, f: as_numpy(g.query_segment(*args(*segment_items(f)))), lambda f: segment_ref.segment(*segment_items(f), tree(f)[1])),
    "max_dist 2": (segment_ref.NAMES, lambda g, f: as_numpy(g.query_segment(*args(*segment_items(f)), 2.0)), lambda f: segment_ref.segment(*segment_items(f), tree(f)[1], 2.0)),
}, lambda w: w["max_dist 2"][1] >= 0, lambda w: w["unbounded"][1])


# the guide passes: the expected values are the oracle's first wavefront restated as tests/test_aov.py and
# tests/test_specular_guides.py restate it, the vector operations by the oracle's glm (aov_ref.OracleMath)
AOV_KEYS = ("albedo", "normal", "depth", "prim", "geom")
CHAIN_KEYS = AOV_KEYS + ("chain", "end_prim", "end_geom", "length0", "depth_first")


def per_pixel(res, keys):
    return tuple(res[k].cpu().numpy().reshape(GUIDE_W * GUIDE_H, -1) for k in keys)


def in_frame(pix, want, keys):
    """the restatement's per-ticket values as whole frames (every pixel has a ticket: the ctx is not sharded)"""
    n = GUIDE_W * GUIDE_H
    assert np.array_equal(np.sort(pix), np.arange(n))
    out = []
    for k in keys:
        a = np.zeros((n,) + want[k].shape[1:], want[k].dtype)
        a[pix] = want[k]
        out.append(a.reshape(n, -1))
    return tuple(out)


def want_aov(fixture):
    sc, nodes, prims = guide_scene(fixture)
    orc = _orc()
    o, q = aov_ref.oracle_queue(orc, sc, nodes, prims, 1, GUIDE_W, GUIDE_H)
    o.close()
    pix, want = aov_ref.expected_aov(aov_ref.OracleMath(orc.lib()), q, sc, prims, np.ascontiguousarray(sc.spheres), 1, GUIDE_W, GUIDE_H, sc.triangle_colors)
    return in_frame(pix, want, AOV_KEYS)


@functools.lru_cache(maxsize=None)
def want_chain(fixture):
    sc, nodes, prims = guide_scene(fixture)
    o, q = aov_ref.oracle_queue(_orc(), sc, nodes, prims, 1, GUIDE_W, GUIDE_H)
    pix, want, _ = specular_ref.expected_chain(o, q, sc, prims, np.ascontiguousarray(sc.spheres), 1, MAX_CHAIN)
    o.close()
    return in_frame(pix, want, CHAIN_KEYS)


def chain_left(chain, length0):
    """per pixel: its chain has bounces and left the scene"""
    return ((chain.reshape(-1) > 0) & (length0.reshape(-1) == VERY_FAR)).reshape(-1, 1)


def want_motion(fixture):
    w = dict(zip(CHAIN_KEYS, want_chain(fixture)))
    return np.zeros((GUIDE_W * GUIDE_H, 2), F), chain_left(w["chain"], w["length0"])


def ask_motion(g, fixture):
    """(motion, previous depth is VERY_FAR) of the chain motion pass on this ctx's own chain guides, the camera unmoved; a pixel
    without bounces takes tyr_render_motion's path and is not asked here"""
    aov = g.render_aov(1, max_chain=MAX_CHAIN)
    m = g.render_motion(aov["prim"], aov["geom"], guide_scene(fixture)[0].camera, chain=aov["chain"], length0=aov["length0"])
    motion, depth = per_pixel(m, ("motion", "prev_depth"))
    return motion, (aov["chain"].cpu().numpy().reshape(-1, 1) > 0) & (depth == VERY_FAR)


def chain_label(what):
    return f"spp 1, max_chain {MAX_CHAIN}{what}"


ENTRIES["aov"] = Entry(GUIDES, {
    "spp 1": (AOV_KEYS, lambda g, f: per_pixel(g.render_aov(1), AOV_KEYS), want_aov),
}, lambda w: w["spp 1"][4][:, 0] >= 0, lambda w: w["spp 1"][3][w["spp 1"][4] == 1])
ENTRIES["aov_chain"] = Entry(GUIDES, {
    chain_label(""): (CHAIN_KEYS, lambda g, f: per_pixel(g.render_aov(1, max_chain=MAX_CHAIN), CHAIN_KEYS), want_chain),
}, lambda w: w[chain_label("")][7][:, 0] >= 0, lambda w: w[chain_label("")][6][w[chain_label("")][7] == 1])
ENTRIES["motion_chain"] = Entry(GUIDES, {
    chain_label(", an unmoved camera"): (("motion", "prev_depth is VERY_FAR"), ask_motion, want_motion),
}, None)


@functools.lru_cache(maxsize=None)
def expected(entry, fixture):
    """label -> the restatement's outputs, computed once per process and read-only"""
    out = {label: tuple(want(fixture)) for label, (_, _, want) in ENTRIES[entry].cases.items()}
    for w in out.values():
        frozen(*(a for a in w if a.flags.writeable))
    return out


# ---- CPU: the fixtures and the restatements' answers --------------------------------------------------------------------
def layout_of(fixture):
    from tyrant_amd import binding

    nodes, prims = tree(fixture) if fixture in TREES else guide_scene(fixture)[1:]
    return binding.layout_probe(nodes, prims, want_pairs=False)


def assert_tree_is(fixture, info):
    """the small trees fit in LDS whole, with room for a count below theirs; the large ones do not fit"""
    quads, staged = info["n_quad_nodes"], info["n_staged_nodes"]
    if fixture in ("small", "cornell"):
        assert 2 <= quads == staged < 64, (fixture, quads, staged)
    else:
        assert staged == 64 < quads, (fixture, quads, staged)


def test_fixtures_reach_what_they_are_for():
    for fixture in LATTICES + GUIDES:
        lay = layout_of(fixture)
        print(fixture, "quads", lay["n_quad_nodes"], "staged", lay["n_staged_nodes"])
        assert_tree_is(fixture, lay)
    for fixture in LATTICES:
        assert items_of(fixture) >= 320 and items_of(fixture) % 64
    assert GUIDE_W * GUIDE_H >= 320 and (GUIDE_W * GUIDE_H) % 64


@pytest.mark.parametrize("entry", [e for e in ENTRIES if ENTRIES[e].answered])
def test_restatements_answer_enough(entry):
    """on the restatement alone, for every fixture of the entry: at least 40 % of the items have a non-empty answer (a hit, a
    member, prim >= 0; for occlusion a blocked sample), at least 10 % have none, and on the large fixture the winners are spread
    over the primitives -- on the lattice at least half of its triangles win somewhere; in the guide frames, whose 1872 pixels
    cannot name half of 32,778 triangles, the winners' indices reach over at least half of the index range and fall into at
    least half of its 64 equal slices.  The skip_shared case of tri holds the contrast it is there for."""
    e = ENTRIES[entry]
    for fixture in e.fixtures:
        w = expected(entry, fixture)
        has = np.asarray(e.answered(w)).reshape(-1)
        share = has.mean()
        line = f"{entry} {fixture}: {has.size} items, {share:.1%} with an answer"
        assert share >= 0.40 and 1.0 - share >= 0.10, line
        if e.winners is not None and fixture in ("large", "mesh128"):
            won = np.unique(e.winners(w))
            n_prims = len(tree(fixture)[1]) if fixture == "large" else len(guide_scene(fixture)[2])
            line += f", {won.size} of {n_prims} primitives win"
            if fixture == "large":
                assert won.size >= n_prims // 2, line
            else:
                assert won.max() - won.min() + 1 >= n_prims // 2 and np.unique(won * 64 // n_prims).size >= 32, line
        print(line)
    if entry == "tri":
        for fixture in e.fixtures:
            tag = "its own triangles, skip_shared, "
            cnt = expected(entry, fixture)[tag + "count"][0]
            plain = tri_ref.tri(*own_triangles(fixture), tree(fixture)[1])[0]
            assert (plain[0::2] > 0).all() and not cnt[0::2].any() and (cnt[1::2] > 0).mean() >= 0.4 and (cnt < plain).all(), fixture
    if entry == "aov_chain":
        chain = expected(entry, "mesh128")[chain_label("")][5]
        print(f"{entry} mesh128: {int((chain > 0).sum())} pixels with a chain, the longest {int(chain.max())}")
        assert (chain > 0).sum() >= 64 and chain.max() >= 2  # (a wave's worth of pixels whose chain traces again)
        left = want_motion("mesh128")[1]
        assert left.sum() >= 10 and ((chain > 0) & ~left).sum() >= 50


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def make_ctx(hip, fixture, flags=0, **tuning):
    """a ctx with the fixture's scene uploaded; tuning: set before the upload"""
    if fixture in TREES:
        return renderer(hip, *tree(fixture), flags=flags, spheres=spheres(), **tuning)
    sc, nodes, prims = guide_scene(fixture)
    g = hip.Renderer(GUIDE_W, GUIDE_H, 4096, flags=aov_ref.flags_of(sc) | flags)
    g.set_tuning(**tuning)
    g.load_scene(sc, nodes, prims)
    return g


def check(entry, g, fixture, what):
    want = expected(entry, fixture)
    for label, (names, ask, _) in ENTRIES[entry].cases.items():
        same(names, ask(g, fixture), want[label], f"{what}, {label}")


def uploaded(hip, fixture, **kw):
    g = make_ctx(hip, fixture, **kw)
    info = g.scene_info()
    assert_tree_is(fixture, info)
    assert info["n_staged_nodes"] == layout_of(fixture)["n_staged_nodes"], (fixture, info)
    return g, info


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_under_every_staged_shape(hip, entry):
    """every case of the entry on every fixture: on one live ctx with TYR_TUNE_STAGED_NODES set between the calls, the scene
    uploaded once; and for staged0 and staged7 with the key set before the upload of a fresh ctx"""
    for fixture in ENTRIES[entry].fixtures:
        g, info = uploaded(hip, fixture)
        for shape, count in STAGED.items():
            g.set_tuning(staged_nodes=info["n_staged_nodes"] - 1 if count is None else count)
            check(entry, g, fixture, f"{entry} {fixture} {shape} on a live ctx")
        assert g.query_error() == 0
        g.close()
        for shape in BEFORE_UPLOAD:
            g, _ = uploaded(hip, fixture, staged_nodes=STAGED[shape])
            check(entry, g, fixture, f"{entry} {fixture} {shape} set before the upload")
            assert g.query_error() == 0
            g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(FRESH))
def test_every_entry_on_a_ctx_of_another_make(hip, shape):
    """the shapes that need a ctx of their own -- the layout pass on the host and on the device, and the counting ctx -- every
    entry on every fixture"""
    knobs = dict(FRESH[shape])
    for fixture in LATTICES + GUIDES:
        g, info = uploaded(hip, fixture, **knobs)
        if "layout_on_device" in knobs:
            assert info["layout_on_device"] == knobs["layout_on_device"], (shape, fixture, info)
        for entry in ENTRIES:
            if fixture in ENTRIES[entry].fixtures:
                check(entry, g, fixture, f"{entry} {fixture} {shape}")
        assert g.query_error() == 0
        g.close()
