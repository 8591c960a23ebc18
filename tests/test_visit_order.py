"""Traversal where the hit depends on the reference's VISIT ORDER.

bvh.h:134 accepts a triangle hit only when `t > epsilon && t < dist && (dist - t) > epsilon`: of two surfaces less than
epsilon = 1e-3 apart along a ray, the one tested first wins even if the other is nearer.  Every device loop that re-lays the
tree out (quad nodes with visit-order ranks, staged top levels, the LDS stack and its spill, packed leaf rounds, the wide
drain, chains for leaves longer than 31 primitives; k_trace_flat, k_query_closest, k_render_aov, the pair-node loop of the
counting build and k_extend_debug) has to reproduce that fold, and on ordinary scenes nothing tells it from "the nearest hit
wins": on the three older ref_traverse_*.npz fixtures and on random rays through cornell_soup2k / mesh32 not one ray's
answer differs from the nearest accepted hit.  The scenes of tests/layered_scenes.py put up to nine surfaces within 0 .. 2.5
epsilon of each other; an order-free comparator in the oracle (orc_brute_closest_batch: the nearest accepted hit of ALL
triangles) tells which rays are "order-sensitive" -- the tree's answer is not the comparator's.

Every GPU test below first asserts, from the oracle alone, that its inputs do reach the rule (`case`, `sweep_case`,
`oracle_render`); measured:
    order-sensitive share of the rays, primary + secondary (>= 0.10 asked; every ray compared, 2,048 sampled on mesh128):
        layered_mesh24 0.34   layered_soup300 0.39   layered_materials 0.33   layered_long_leaves 0.42   layered_mesh128 0.34
    >= 100 order-sensitive rays in each direction octant on the three scenes of offset layers whose every ray is compared
        (fewest: 1,087 / 947 / 1,067), each octant with at least 1/16 of the hits.  Not asked of layered_long_leaves (its stacks
        face one way and back faces are culled: four octants cannot hit them; 0.91 of the aimed rays hit a stack, 0.61 of those are
        order-sensitive), of layered_mesh128 (2,048 sampled rays hold 69 - 128 per octant), or of the exact duplicates, where
        no ray is order-sensitive by construction and the TIE rule is checked instead:
    layered_dup6 / layered_dup24 (leaves of 12, and chains of 48): 0.88 / 0.89 of the primary rays hit, every hit's t is shared
        bit for bit by another triangle and the winner is the LOWEST index of them (with the comparator's last-index-on-ties
        switch every hit goes to another triangle)
    tmax = float32(t* + epsilon) moved by -2 .. +2 ulp: the answer changes between the two ends for 1.00 of 4,096 hit rays
    secondary rays from the first pass's hit points: 0.15 - 0.16 answered with t < 1.5 epsilon
    camera rays (FRAMED_CAMERA: every ray enters the room): 0.47 - 0.51 of the triangle hits of a frame are order-sensitive
and the CPU tests hold the oracle to the reference's own bvh.h on the same rays (tests/golden/ref_answers.npz, live where
oracle/_ref is built).  All GPU comparisons are bit for bit; nothing differed when the module was written.

Run time on an MI355X box (`pytest -m gpu -x -q --durations=0 tests`): this module's 50 GPU tests 12.2 s in all (the longest,
the queries on layered_mesh128, 2.8 s; the comparator included); the whole run 262 s with the module, 241 s without it on the
same box right after (the limit is 900 s, the longest single test 75 s).
"""
import functools

import numpy as np
import pytest

import layered_scenes as ls
from conftest import bits

VERY_FAR = ls.VERY_FAR
OFFSET_SCENES = ("layered_mesh24", "layered_soup300", "layered_materials")  # nine offset layers, every ray compared with the comparator
ALL = ("layered_mesh24", "layered_soup300", "layered_materials", "layered_long_leaves", "layered_dup6", "layered_dup24", "layered_mesh128")
N_RAYS = 16384
N_BRUTE_MESH128 = 2048  # rays of layered_mesh128 that go through the comparator (295,002 triangles each)
COUNTER_FIELDS = ("total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible", "start_position", "frame")


def _orc():
    from oracle import pyorc

    pyorc.lib()
    return pyorc


def parked_spheres():
    """every sphere where no ray can reach it: only the BVH answers"""
    from tyrant_amd import scenes

    s = scenes.cornell_spheres()
    s["position"] = np.array([0.0, 1e6, -1e6], dtype=np.float32)
    s["radius"] = 1.0
    return s


# ---- the inputs and what the oracle says about them (computed once per process) -----------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """scene, rays (primary set, then the secondary rays from its hit points), the oracle's answers, the order-sensitive rays
    -- and the non-vacuity conditions of the module docstring, asserted on the oracle's answers alone"""
    orc = _orc()
    sc, nodes, prims = ls.built_layered(name)
    seed = 1 + ALL.index(name)
    o1, d1 = ls.stack_rays(N_RAYS, seed) if name == "layered_long_leaves" else ls.ray_set(sc, nodes, N_RAYS, seed)
    t1, p1 = ls.tree_closest(orc, nodes, prims, o1, d1)
    o2, d2 = ls.secondary(o1, d1, t1, p1 >= 0, seed + 100)
    t2, p2 = ls.tree_closest(orc, nodes, prims, o2, d2)
    o, d, t, p = np.concatenate([o1, o2]), np.concatenate([d1, d2]), np.concatenate([t1, t2]), np.concatenate([p1, p2])
    n = o.shape[0]
    brute = np.arange(n) if name != "layered_mesh128" else np.sort(np.random.default_rng(seed).choice(n, N_BRUTE_MESH128, replace=False))
    bt, bp = orc.brute_closest(prims, o[brute], d[brute], VERY_FAR)
    sens = (bits(bt) != bits(t[brute])) | (bp != p[brute])
    c = dict(name=name, sc=sc, nodes=nodes, prims=prims, o=o, d=d, t=t, p=p, n1=N_RAYS, brute=brute, sens=sens, share=float(sens.mean()),
             per_octant=np.bincount(ls.octant(d[brute])[sens], minlength=8), hits_per_octant=np.bincount(ls.octant(d1)[p1 >= 0], minlength=8),
             near=float(np.mean((p2 >= 0) & (t2 < np.float32(1.5e-3)))))
    print(f"{name}: {len(prims)} triangles, largest leaf {nodes['primitiveCount'].max()}, {n} rays, hit {np.mean(p >= 0):.3f}, order-sensitive {c['share']:.3f} "
          f"(per octant {c['per_octant'].tolist()}), secondary rays answered below 1.5 epsilon {c['near']:.3f}")
    if name in ls.DUPS:
        hit = p >= 0
        lt, lp = orc.brute_closest(prims, o, d, VERY_FAR, last_on_ties=True)
        assert np.mean(p1 >= 0) >= 0.5, name
        assert np.array_equal(bits(bt), bits(t)) and np.array_equal(bp, p), f"{name}: the tree's winner is not the lowest index of the nearest hits"
        assert np.array_equal(bits(lt), bits(t)) and np.all(lp[hit] > p[hit]), f"{name}: a hit whose t no other triangle shares"
        assert nodes["primitiveCount"].max() > (31 if name == "layered_dup24" else 5), name
    else:
        assert c["share"] >= 0.10, (name, c["share"])
        assert c["near"] >= 0.05, (name, c["near"])
    if name in OFFSET_SCENES:
        assert c["per_octant"].min() >= 100, (name, c["per_octant"])
        assert c["hits_per_octant"].min() * 16 >= (p1 >= 0).sum(), (name, c["hits_per_octant"])
    if name == "layered_long_leaves":
        counts = set(nodes["primitiveCount"].tolist())
        assert 24 in counts and 72 in counts, counts
        stack = (prims["vert"][:, 2] == np.float32(10.0)) & (prims["e1"][:, 0] == np.float32(60.0))  # the stacks' triangles (none of the Cornell box starts at z = 10)
        assert stack.sum() == 96
        on_stack = (p1 >= 0) & stack[np.maximum(p1, 0)]  # (of the aimed rays; the secondary rays leave the stacks in all directions)
        assert on_stack.mean() >= 0.5 and sens[:N_RAYS][on_stack].mean() >= 0.10, (on_stack.mean(), sens[:N_RAYS][on_stack].mean())
    return c


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """the first 4,096 hit rays of case(name) with tmax = float32(t* + epsilon) moved by -2 .. +2 ulp: {k: (tmax, closest t,
    closest prim, any hit)} from the oracle, and the condition that the two ends differ for >= 0.9 of the rays"""
    orc = _orc()
    c = case(name)
    idx = np.nonzero(c["p"][: c["n1"]] >= 0)[0][:4096]
    o, d = c["o"][idx], c["d"][idx]
    res = {}
    for k, tm in ls.tmax_sweep(c["t"][idx]).items():
        t, p = ls.tree_closest(orc, c["nodes"], c["prims"], o, d, tm)
        res[k] = (tm, t, p, ls.tree_any(orc, c["nodes"], c["prims"], o, d, tm))
    ends = float(np.mean((bits(res[-2][1]) != bits(res[2][1])) | (res[-2][2] != res[2][2])))
    print(f"{name}: tmax sweep over {len(idx)} hit rays, answers differ between -2 and +2 ulp for {ends:.3f}")
    assert len(idx) >= 2048 and ends >= 0.9, (name, len(idx), ends)
    return o, d, res


# ---- CPU: the conditions, and the oracle against the reference's own bvh.h ------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_inputs_reach_the_visit_order_rule(name):
    """the non-vacuity conditions (module docstring) hold for every scene's ray set -- asserted inside case / sweep_case, which
    the GPU tests call too; layered_mesh128's tree has more quad nodes than are staged and needs more stack than the LDS part"""
    from tyrant_amd import binding

    c = case(name)
    if name != "layered_mesh128":
        sweep_case(name)
    else:
        lp = binding.layout_probe(c["nodes"], c["prims"])
        assert lp["n_quad_nodes"] > 64 and lp["quad_max_stack"] > 12, lp


def test_ordinary_scenes_do_not_reach_the_rule(orc):
    """the gap this module closes: on cornell_soup2k and mesh32 the reference's answer is the nearest accepted hit for every
    one of 8,192 random rays, so a traversal that lets the nearest hit win passes every test built on them"""
    from conftest import built_scene

    for name in ("cornell_soup2k", "mesh32"):
        sc, nodes, prims = built_scene(name)
        o, d = ls.ray_set(sc, nodes, 8192, 3)
        t, p = ls.tree_closest(orc, nodes, prims, o, d)
        assert not ls.order_sensitive(orc, prims, o, d, t, p).any(), name


@pytest.mark.parametrize("name", ALL)
def test_oracle_equals_the_reference_on_layered_scenes(orc, ref_answers, name):
    """orc_bvh_intersect / _simple against CachedBVH::intersect / intersectSimple compiled from the reference's bvh.h
    (live where oracle/_ref is built, else its recorded digests): every ray of the scene's set from VERY_FAR, and the hit rays
    of the tmax sweep with distance / closestAllowed at the five values around t* + epsilon"""
    import ctypes as C
    import hashlib

    from tyrant_amd import scenes

    c = case(name)
    nodes, prims = np.ascontiguousarray(c["nodes"]), np.ascontiguousarray(c["prims"])
    o, d = c["o"], c["d"]
    idx = np.nonzero(c["p"][: c["n1"]] >= 0)[0][:4096]
    sweep = ls.tmax_sweep(c["t"][idx])
    os_, ds_ = np.tile(o[idx], (5, 1)), np.tile(d[idx], (5, 1))
    tms = np.concatenate([sweep[k] for k in (-2, -1, 0, 1, 2)])

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return np.array(h.hexdigest())

    t, p = ls.tree_closest(orc, nodes, prims, o, d)
    ts, ps = ls.tree_closest(orc, nodes, prims, os_, ds_, tms)
    mine = {"closest": sha(t, p), "sweep_closest": sha(ts, ps), "sweep_any": sha(ls.tree_any(orc, nodes, prims, os_, ds_, tms).astype(np.int32))}

    def ask(ref):
        ip = C.POINTER(C.c_int)
        out = {}
        for key, (oo, dd, tm) in {"closest": (o, d, None), "sweep_closest": (os_, ds_, tms)}.items():
            n = oo.shape[0]
            r = np.zeros(n, dtype=scenes.RAY_DTYPE)
            r["origin"], r["direction"], r["identifier"] = oo, dd, -1
            r["distance"] = VERY_FAR if tm is None else tm
            hit = np.zeros(n, dtype=np.int32)
            ref.ref_bvh_intersect(nodes.ctypes.data, prims.ctypes.data, r.ctypes.data, n, hit.ctypes.data_as(ip), None)
            out[key] = sha(r["distance"], np.where(hit != 0, r["identifier"], -1).astype(np.int32))
        n = os_.shape[0]
        s = np.zeros(n, dtype=scenes.SHADOW_DTYPE)
        s["origin"], s["direction"], s["closestDistance"] = os_, ds_, tms
        occ = np.zeros(n, dtype=np.int32)
        ref.ref_bvh_intersect_simple(nodes.ctypes.data, prims.ctypes.data, s.ctypes.data, n, occ.ctypes.data_as(ip))
        out["sweep_any"] = sha((occ != 0).astype(np.int32))
        return out

    want = ref_answers(f"visit_order_{name}", ask, inputs=(nodes, prims, o, d, tms))
    for k in mine:
        assert str(mine[k]) == str(want[k]), f"{name}: the oracle's {k} answers are not the reference's"


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def renderer(hip, c, n=4096, W=64, H=64, flags=0, spheres=None, **knobs):
    g = hip.Renderer(W, H, n, flags=flags)
    if "layout_on_device" in knobs:  # (read by the upload)
        g.set_tuning(layout_on_device=knobs.pop("layout_on_device"))
    g.upload(c["nodes"], c["prims"])
    g.set_spheres(parked_spheres() if spheres is None else spheres)
    g.set_tuning(**knobs)
    return g


def check_closest(orc, g, prims, o, d, tmax, want_t, want_p, what, spheres=False, want_geom=None):
    from test_ray_query import glm_uv, np_results

    t, prim, geom, uv = np_results(g.query_closest(o, d, tmax, spheres=spheres))
    assert g.query_error() == 0, what
    assert np.array_equal(bits(t), bits(want_t)), f"{what}: {np.count_nonzero(bits(t) != bits(want_t))} of {len(t)} distances differ"
    assert np.array_equal(prim, want_p), f"{what}: {np.count_nonzero(prim != want_p)} of {len(t)} primitives differ"
    assert np.array_equal(geom, np.where(want_p >= 0, 1, -1) if want_geom is None else want_geom), what
    tri = geom == 1
    u, v = glm_uv(orc, prims, prim[tri], o[tri], d[tri])
    assert np.array_equal(bits(uv[tri, 0]), bits(u)) and np.array_equal(bits(uv[tri, 1]), bits(v)), f"{what}: barycentrics"
    assert np.all(uv[~tri] == 0), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_queries_on_layered_scenes(orc, hip, name):
    """query_closest / query_any over the scene's whole ray set in one batch (seven times the ctx's queue), in the given, a
    shuffled and a sorted order, without and with the spheres"""
    from test_ray_query import oracle_spheres_any, oracle_spheres_closest

    c = case(name)
    o, d, t, p, prims = c["o"], c["d"], c["t"], c["p"], c["prims"]
    n = o.shape[0]
    spheres = np.ascontiguousarray(c["sc"].spheres)
    g = renderer(hip, c, spheres=spheres)
    # any-hit limits: at the accept rule's edge for the rays that hit (t* + epsilon, -2 .. +2 ulp), mid-room for the others
    tm = np.full(n, 80.0, dtype=np.float32)
    hit = p >= 0
    edge = (t + ls.EPSILON).astype(np.float32)
    tm[hit] = (edge.view(np.int32) + (np.arange(n, dtype=np.int32) % 5 - 2)).view(np.float32)[hit]
    occ_want = ls.tree_any(orc, c["nodes"], prims, o, d, tm)
    for how in ("given", "shuffled", "sorted"):
        perm = np.arange(n) if how == "given" else ls.reorder(o, d, how, seed=7)
        oo, dd = np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm])
        check_closest(orc, g, prims, oo, dd, None, t[perm], p[perm], f"{name} {how}")
        occ = g.query_any(oo, dd, np.ascontiguousarray(tm[perm])).cpu().numpy()
        assert g.query_error() == 0
        assert np.array_equal(occ, occ_want[perm]), f"{name} {how}: {np.count_nonzero(occ != occ_want[perm])} any-hit answers differ"
    # with the spheres (intersect_scene: the spheres shorten the ray before the tree is walked): a third of the rays
    sub = np.arange(0, n, 3)
    oo, dd = np.ascontiguousarray(o[sub]), np.ascontiguousarray(d[sub])
    far = np.full(len(sub), VERY_FAR, dtype=np.float32)
    st, sp, sg = oracle_spheres_closest(orc, spheres, c["nodes"], prims, oo, dd, far)
    assert (sg == 0).sum() > 50 and (sg == 1).sum() > 1000, name
    check_closest(orc, g, prims, oo, dd, None, st, sp, f"{name} with spheres", spheres=True, want_geom=sg)
    occ = g.query_any(oo, dd, np.ascontiguousarray(tm[sub]), spheres=True).cpu().numpy()
    assert np.array_equal(occ, oracle_spheres_any(orc, spheres, c["nodes"], prims, oo, dd, tm[sub])), f"{name}: any hit with spheres"
    assert g.query_error() == 0 and g.counters()["device_error"] == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in ALL if n != "layered_mesh128"])
def test_tmax_sweep_through_queries_and_shadow_records(orc, hip, name):
    """tmax = float32(t* + epsilon) moved by -2 .. +2 ulp: query_closest (ray.distance) and query_any (closestAllowed); and on
    the render path, where extend always starts from VERY_FAR, as shadow records with closestDistance at the five values
    through the connect stage, merged and unmerged: visible count and the pixels the records add to (one record per pixel)"""
    from tyrant_amd import scenes

    c = case(name)
    o, d, res = sweep_case(name)
    n = o.shape[0]
    g = renderer(hip, c)
    for k, (tm, t, p, occ) in res.items():
        check_closest(orc, g, c["prims"], o, d, tm, t, p, f"{name} tmax {k:+d} ulp")
        got = g.query_any(o, d, tm).cpu().numpy()
        assert np.array_equal(got, occ), f"{name} tmax {k:+d} ulp: {np.count_nonzero(got != occ)} any-hit answers differ"
    assert g.query_error() == 0
    g.close()
    W, H = 64, (n + 63) // 64
    for merge in (1, 0):
        for k, (tm, _, _, occ) in res.items():
            g = renderer(hip, c, n=n, W=W, H=H, merge_trace=merge)
            sh = np.zeros(n, dtype=scenes.SHADOW_DTYPE)
            sh["origin"], sh["direction"], sh["closestDistance"], sh["color"] = o, d, tm, 1.0
            sh["buffer_index"] = np.arange(n, dtype=np.int32)
            g.stage("begin")
            g.import_shadow_queue(sh)
            g.stage("connect")
            kc = g.counters()
            what = f"{name} shadow records, closestDistance {k:+d} ulp, merge_trace {merge}"
            assert kc["device_error"] == 0 and kc["n_shadow_visible"] == int((~occ).sum()), what
            b = g.blit_buffer()[:n]
            assert np.array_equal(b[:, 0] == 1.0, ~occ) and np.array_equal(b[:, :3].sum(axis=1) == 0.0, occ), what
            g.close()


@functools.lru_cache(maxsize=None)
def extend_rays(name, n):
    """n queue records from the scene's ray set (primary and secondary rays, shuffled into the same waves) and the oracle's
    extend stage for them: (records, records after extend, the oracle's counters)"""
    from tyrant_amd import scenes

    orc = _orc()
    c = case(name)
    pick = np.random.default_rng(n).permutation(c["o"].shape[0])[:n]
    rays = np.zeros(n, dtype=scenes.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["direct"], rays["distance"] = c["o"][pick], c["d"][pick], 1.0, VERY_FAR
    rays["index"] = np.arange(n, dtype=np.int32) % 4096
    o = orc.Oracle(64, 64, n)
    o.upload(c["nodes"], c["prims"])
    o.set_spheres(parked_spheres())
    stage_extend(o, rays, n)
    q, k = o.ray_queue(0, n), o.counters()
    o.close()
    # (the records' own share of order-sensitive rays, where every ray went through the comparator)
    if name != "layered_mesh128" and name not in ls.DUPS and n >= 1000:
        assert c["sens"][pick].mean() >= 0.10, (name, n)
    return rays, q, k


def stage_extend(r, rays, n):
    r.stage("begin")
    r.import_work_queue(rays, n)
    r.set_budget(0)
    r.stage("primary")  # budget 0: no new rays, n_live = n
    r.stage("extend")


EXTEND_SHAPES = {
    "default": dict(),
    "wide_drain0": dict(wide_drain=0),  # a wave's last rays stay one to a lane
    "wide_blocks": dict(wide_block_min_items=0),  # every launch as 768-thread blocks
    "narrow_blocks": dict(wide_block_min_items=-1),
    "staged0": dict(staged_nodes=0), "staged1": dict(staged_nodes=1), "staged7": dict(staged_nodes=7), "staged64": dict(staged_nodes=64),
    "waves1": dict(waves_per_simd=1), "waves3": dict(waves_per_simd=3),
    "refill1": dict(refill_min_idle=1, min_traversing=1), "refill64": dict(refill_min_idle=64, min_traversing=64),
    "static0": dict(static_share=0), "static15": dict(static_share=15),
    "layout_host": dict(layout_on_device=0), "layout_device": dict(layout_on_device=1),
    "counting": dict(flags=4),  # TYR_FLAG_COUNT_VISITS: the pair-node loop; the NUMBER of tests is the oracle's too
}
# queue sizes: ragged last waves (the wide drain and the refill see few rays) and a full launch
EXTEND_CASES = (("layered_mesh24", (65, 1000, 4097, 16384)), ("layered_long_leaves", (65, 1000, 4097)), ("layered_dup24", (1000, 4097)),
                ("layered_materials", (4097,)), ("layered_mesh128", (4097, 16384)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(EXTEND_SHAPES))
def test_extend_stage_under_every_traversal_shape(orc, hip, shape):
    """the render path's extend stage on imported records against the oracle's, under each launch shape of tyr_set_tuning
    that changes what the traversal loop does, and as the counting build"""
    knobs = dict(EXTEND_SHAPES[shape])
    flags = knobs.pop("flags", 0)
    for name, sizes in EXTEND_CASES:
        c = case(name)
        for n in sizes:
            rays, qo, ko = extend_rays(name, n)
            g = renderer(hip, c, n=n, flags=flags, **knobs)
            stage_extend(g, rays, n)
            kg = g.counters()
            qg = g.ray_queue(0, n)
            what = f"{name} n={n} {shape}"
            assert kg["device_error"] == 0 and kg["n_live"] == n, what
            assert np.array_equal(bits(qo["distance"]), bits(qg["distance"])), f"{what}: {np.count_nonzero(bits(qo['distance']) != bits(qg['distance']))} distances differ"
            hit = qo["distance"] < VERY_FAR
            assert hit.mean() > 0.4, what
            assert np.array_equal(qo["identifier"][hit], qg["identifier"][hit]), f"{what}: {np.count_nonzero(qo['identifier'][hit] != qg['identifier'][hit])} identifiers differ"
            assert np.array_equal(qo["geometry_type"][hit], qg["geometry_type"][hit]), what
            if flags & 4:
                for f in ("nodes_extend", "tris_extend", "rays_in_tree_extend"):
                    assert ko[f] == kg[f] and ko[f] > 0, (what, f, ko[f], kg[f])
            g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["layered_mesh24", "layered_mesh128"])
def test_debug_picture_on_a_layered_scene(orc, hip, name):
    """k_extend_debug's traversal-cost picture = the oracle's intersect_debug counts: the number of steps is the visit order's
    (the picture has one level per 19.5 steps, kernel.cu:300-328: the two deeper trees, where it has more than eight)"""
    from test_debug_bvh import FLAG, paint

    c = case(name)
    n = 4096
    rays, _, _ = extend_rays(name, 4097)
    rays = rays[:n].copy()
    rays["index"] = np.arange(n, dtype=np.int32)
    o = orc.Oracle(64, 64, n, flags=FLAG)
    g = hip.Renderer(64, 64, n, flags=FLAG)
    want = paint(o, c["nodes"], c["prims"], rays, n, "extend_debug")
    got = paint(g, c["nodes"], c["prims"], rays, n, "extend")
    assert g.counters()["device_error"] == 0
    assert len(np.unique(want[:, :2], axis=0)) > 8  # a picture, not one colour
    assert np.array_equal(got, want), f"{np.count_nonzero((got != want).any(axis=1))} pixels differ"
    g.close()


def pair(orc, hip, name, W, H, N, extra_flags=0):
    c = case(name)
    sc = c["sc"]
    flags = ls.scene_flags(sc)
    o = orc.Oracle(W, H, N, flags=flags & 25)
    o.load_scene(sc, c["nodes"], c["prims"])
    g = hip.Renderer(W, H, N, flags=flags | extra_flags)
    g.load_scene(sc, c["nodes"], c["prims"])
    return o, g


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["layered_mesh24", "layered_materials"])
def test_aov_and_motion_on_layered_scenes(orc, hip, name):
    """render_aov's ids / depth / normal / albedo = the oracle's first wavefront (as tests/test_aov.py derives them), and
    render_motion from those ids against the float64 restatement of tests/test_temporal.py, on a scene where the first
    hit is one of nine within 2.5 epsilon"""
    from test_aov import aov_into, assert_aov_equal, expected_aov, first_wavefront
    from test_temporal import check_motion, expected_motion, moved_camera, sample0_rays

    c = case(name)
    sc, nodes, prims = c["sc"], c["nodes"], c["prims"]
    W, H = 96, 64
    flags = ls.scene_flags(sc)
    g = hip.Renderer(W, H, 4096, flags=flags)
    g.load_scene(sc, nodes, prims)
    spheres = np.ascontiguousarray(sc.spheres)
    for spp in (1, 3):
        o = orc.Oracle(W, H, spp * W * H, flags=flags & 25)
        o.load_scene(sc, nodes, prims)
        q = first_wavefront(o, spp * W * H)
        o.close()
        tri = (q["distance"] < VERY_FAR) & (q["geometry_type"] == 1)
        sens = ls.order_sensitive(orc, prims, q["origin"][tri], q["direction"][tri], q["distance"][tri], q["identifier"][tri])
        assert tri.mean() > 0.1 and sens.mean() >= 0.10, (name, tri.mean(), sens.mean())  # the camera rays reach the rule too
        pix, want = expected_aov(hip, q, sc, prims, spheres, spp, W, H, sc.triangle_colors)
        rc, got = aov_into(hip, g, spp)
        assert rc == 0, rc
        assert_aov_equal(got, pix, want, f"{name} spp {spp}")
    assert g.query_error() == 0
    prev = sc.camera
    cur = moved_camera(prev, -1.0)
    g.set_camera(cur)
    aov = g.render_aov(1, albedo=False, normal=False, depth=False)
    got = g.render_motion(aov["prim"], aov["geom"], prev)
    q = sample0_rays(orc, sc, nodes, prims, cur, W, H)
    check_motion(got, expected_motion(hip, g, q, prims, spheres, cur, prev, W, H), W, H, name)
    g.close()


@functools.lru_cache(maxsize=None)
def oracle_render(name, W, H, N, spp):
    """the oracle's render(spp), a second render cut after two iterations and the iteration that follows it, stage by stage:
    what every tuning profile has to reproduce"""
    orc = _orc()
    c = case(name)
    sc = c["sc"]
    o = orc.Oracle(W, H, N, flags=ls.scene_flags(sc) & 25)
    o.load_scene(sc, c["nodes"], c["prims"])
    out = dict(iterations=o.render(spp), counters=o.counters(), accum=o.blit_buffer())
    o.reset_accum()  # a second render cut after two iterations: its survivors are the next iteration's rays
    assert o.render(spp, 2) == 2
    out["cut_counters"], out["cut_accum"] = o.counters(), o.blit_buffer()
    for st in ("begin", "primary"):
        o.stage(st)
    n = o.counters()["n_live"]
    out["n_live"], out["after_primary"] = n, o.ray_queue(0, n)
    # this iteration's rays (survivors of the render and fresh camera rays) reach the rule: the condition of the module docstring
    q = out["after_primary"]
    t, p = ls.tree_closest(orc, c["nodes"], c["prims"], q["origin"], q["direction"])
    share = ls.order_sensitive(orc, c["prims"], q["origin"], q["direction"], t, p).mean()
    assert share >= 0.10, (name, share)
    o.stage("extend")
    out["after_extend"] = o.ray_queue(0, n)
    o.stage("shade")
    k = o.counters()
    out["ns"], out["nh"] = k["primary_ray_cnt"], k["shadow_ray_cnt"]
    out["survivors"], out["shadows"] = o.ray_queue(1, out["ns"]), o.shadow_queue(out["nh"])
    o.stage("connect")
    out["visible"], out["accum_staged"] = o.counters()["n_shadow_visible"], o.blit_buffer()
    o.close()
    return out


def _profiles():
    from test_render_sequences import PROFILES

    return PROFILES


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["layered_mesh24", "layered_materials"])
@pytest.mark.parametrize("profile", ["default", "run_ahead0", "merge_trace0", "fold_prologue0", "scan_snapshot0", "resolve_shadows0", "wide_blocks"])
def test_render_and_staged_iteration_on_layered_scenes(orc, hip, name, profile):
    """render(spp) = the oracle's (iterations, counters, completed-path counts, radiance); a second render cut after two
    iterations, then the next iteration stage by stage with the extend answers and both queues equal to the oracle's (survivors
    of two bounces beside fresh camera rays), on every tuning profile of test_render_sequences.
    The shadow rays here start within epsilon of other layers: the any-hit rule's `t > epsilon` edge."""
    from test_gpu_parity import assert_accum_close, assert_state_equal

    assert set(_profiles()) == {"default", "run_ahead0", "merge_trace0", "fold_prologue0", "scan_snapshot0", "resolve_shadows0", "wide_blocks"}
    W, H, N, spp = 96, 64, 5000, 2
    want = oracle_render(name, W, H, N, spp)
    c = case(name)
    sc = c["sc"]
    g = hip.Renderer(W, H, N, flags=ls.scene_flags(sc))
    g.load_scene(sc, c["nodes"], c["prims"])
    g.set_tuning(**_profiles()[profile])
    what = f"{name} {profile}"
    assert g.render(spp) == want["iterations"], what
    kg = g.counters()
    assert kg["device_error"] == 0, what
    for f in COUNTER_FIELDS:
        assert want["counters"][f] == kg[f], (what, f, want["counters"][f], kg[f])
    assert_accum_close(want["accum"], g.blit_buffer(), what)
    g.reset_accum()
    assert g.render(spp, 2) == 2, what
    kg = g.counters()
    for f in COUNTER_FIELDS:
        assert want["cut_counters"][f] == kg[f], (what, "render cut at two iterations", f, want["cut_counters"][f], kg[f])
    assert_accum_close(want["cut_accum"], g.blit_buffer(), what + " render cut at two iterations")
    g.stage("begin"), g.stage("primary")
    n = want["n_live"]
    assert g.counters()["n_live"] == n, what
    assert_state_equal(want["after_primary"], g.ray_queue(0, n), what + " after primary")
    g.stage("extend")
    qo, qg = want["after_extend"], g.ray_queue(0, n)
    assert np.array_equal(bits(qo["distance"]), bits(qg["distance"])), what + " extend distance"
    hit = qo["distance"] < VERY_FAR
    assert np.array_equal(qo["identifier"][hit], qg["identifier"][hit]) and np.array_equal(qo["geometry_type"][hit], qg["geometry_type"][hit]), what + " extend identifier"
    g.stage("shade")
    kg = g.counters()
    assert kg["device_error"] == 0 and (kg["primary_ray_cnt"], kg["shadow_ray_cnt"]) == (want["ns"], want["nh"]), what
    assert_state_equal(want["survivors"], g.ray_queue(1, want["ns"]), what + " survivors")
    assert want["shadows"].tobytes() == g.shadow_queue(want["nh"]).tobytes(), what + " shadow queue"
    g.stage("connect")
    assert g.counters()["n_shadow_visible"] == want["visible"], what
    assert_accum_close(want["accum_staged"], g.blit_buffer(), what + " staged iteration")
    g.stage("end")
    g.close()


@pytest.mark.gpu
def test_refit_from_exact_copies_to_offset_layers(orc, hip):
    """layered_mesh24 uploaded with every layer at offset 0 (nine exact copies), then refitted to the offset layers: the tree
    keeps the shape and the split axes the builder chose for the copies -- the visit order comes from the OLD tree, the
    geometry is new -- and queries and a render equal the oracle's on the refitted tree"""
    from test_gpu_parity import assert_accum_close
    from test_scene_refit import TYR_FLAG_REFIT, refit_nodes, tri_bboxes
    from tyrant_amd import scenes

    flat = ls.MAKERS["layered_mesh24_flat"]()
    tagged = flat.triangles.copy()
    tag = np.arange(len(tagged), dtype=np.uint32)
    tagged["pad_"] = np.stack([tag & 255, (tag >> 8) & 255, tag >> 16], axis=1).astype(np.uint8)  # (the builder does not read them)
    nodes, built = orc.bvh_build(tagged, scenes.triangle_bboxes(tagged))
    order = built["pad_"][:, 0].astype(np.int64) | (built["pad_"][:, 1].astype(np.int64) << 8) | (built["pad_"][:, 2].astype(np.int64) << 16)
    prims = np.ascontiguousarray(flat.triangles[order])
    assert nodes.tobytes() == orc.bvh_build(flat.triangles, scenes.triangle_bboxes(flat.triangles))[0].tobytes()
    sc = ls.MAKERS["layered_mesh24"]()
    moved = np.ascontiguousarray(sc.triangles[order])  # the offset layers in the uploaded (build) order
    assert not np.array_equal(moved["vert"], prims["vert"]) and np.array_equal(moved["materialType"], prims["materialType"])
    want_nodes = refit_nodes(nodes, tri_bboxes(moved))
    # what the oracle says on the refitted tree, and that the rays reach the rule there
    o, d = ls.ray_set(sc, want_nodes, N_RAYS, 77)
    t, p = ls.tree_closest(orc, want_nodes, moved, o, d)
    share = ls.order_sensitive(orc, moved, o, d, t, p).mean()
    assert share >= 0.10, share
    W, H, N, spp = 96, 64, 5000, 2
    flags = ls.scene_flags(sc)
    g = hip.Renderer(W, H, N, flags=flags | TYR_FLAG_REFIT)
    g.load_scene(sc, nodes, prims)
    got_nodes = g.refit(moved, want_nodes=True)
    assert got_nodes.tobytes() == want_nodes.tobytes()
    check_closest(orc, g, moved, o, d, None, t, p, "refitted layers")
    tm = np.where(p >= 0, ls.ulp_step((t + ls.EPSILON).astype(np.float32), 1), np.float32(80.0)).astype(np.float32)
    occ = g.query_any(o, d, tm).cpu().numpy()
    assert np.array_equal(occ, ls.tree_any(orc, want_nodes, moved, o, d, tm))
    assert g.query_error() == 0
    ref = orc.Oracle(W, H, N, flags=flags & 25)
    ref.load_scene(sc, want_nodes, moved)
    assert ref.render(spp) == g.render(spp)
    ko, kg = ref.counters(), g.counters()
    assert kg["device_error"] == 0
    for f in COUNTER_FIELDS:
        assert ko[f] == kg[f], f
    assert_accum_close(ref.blit_buffer(), g.blit_buffer(), "render after the refit to offset layers")
    g.close()


@pytest.mark.gpu
def test_fuzz_slice_with_layers(hip):
    """25 seeded cases of tests/fuzz_parity.py (random scenes, shards, queue sizes, cameras and launch-shape knobs against the
    oracle), every third with its scene wrapped in layered_scenes.layered"""
    import fuzz_parity

    rng = np.random.default_rng(20261016)
    failed, layered = [], 0
    for i in range(25):
        c = fuzz_parity.draw_case(rng, i, layers=True)
        layered += c["sc"].name.endswith("+layers")
        ok, why, line = fuzz_parity.run_case(c)
        print(line)
        if not ok:
            failed.append(line)
    assert layered == 9
    assert not failed, "\n".join(failed)
