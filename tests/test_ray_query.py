"""Batched ray queries on the uploaded scene (tyr_query_closest / tyr_query_any, hip/query.hip; Renderer.query_closest /
query_any): the reference's CachedBVH::intersect (bvh.h:118-161) and intersectSimple (bvh.h:213-256) with a caller's tmax,
intersect_scene / intersect_scene_simple (kernel.cu:125-140 / 163-174) with TYR_QUERY_SPHERES -- bit for bit.

CPU: what the compiler made of the query kernels (make asm).  GPU: the reference's committed answers, C3's 1 M-triangle tree
against the reference harness (or the oracle the CPU tests pin to it), the spheres against the render's own extend stage,
hostile rays and batch sizes, barycentrics, isolation from the render state, streams and argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits, built_scene
from kernel_resources import kernel_resources
from query_support import assert_render_undisturbed, check_kernel_budget, on_side_stream, renderer
from ray_ref import _rays, glm_uv, oracle_any, oracle_closest, oracle_spheres_any, oracle_spheres_closest  # noqa: F401 (test_visit_order takes them from here)


# ---- CPU: resources of the query kernels ------------------------------------------------------------------------------
def test_query_kernels_keep_registers_and_lds_in_budget():
    """no vector spills; scratch no larger than the LdsStack's private spill arrays (52 entries of 8 / 4 bytes, plus the
    frame's alignment); LDS that admits the five (closest) / seven (any) blocks per CU that the occupancy query plans for"""
    res = kernel_resources("query")
    spill_entries = 64 - 12
    for kind, with_t, blocks in (("k_query_closest", True, 5), ("k_query_any", False, 7)):
        for sph in (0, 1):
            check_kernel_budget(res, f"{kind}ILb{sph}E", 1, spill_entries * (8 if with_t else 4) + 16, planned=blocks)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def parked_spheres():
    """every sphere where no ray can reach it: only the BVH answers"""
    from tyrant_amd import scenes

    spheres = scenes.cornell_spheres()
    spheres["position"] = np.array([0.0, 1e6, -1e6], dtype=np.float32)
    spheres["radius"] = 1.0
    return spheres


def np_results(res):
    return tuple(x.cpu().numpy() for x in res)


def random_dirs(rng, n):
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_fixtures_closest_and_any(hip):
    """tests/golden/ref_traverse_*.npz -- the reference's own bvh.h answers -- for every ray, the pre-shortened ones included"""
    from tyrant_amd import scenes

    for name in ("cornell36", "soup2k", "mesh32", "layered"):
        z = np.load(os.path.join(GOLDEN, f"ref_traverse_{name}.npz"))
        nodes = np.ascontiguousarray(z["nodes"]).view(scenes.NODE_DTYPE).reshape(-1)
        prims = np.ascontiguousarray(z["prims"]).view(scenes.TRIANGLE_DTYPE).reshape(-1)
        g = renderer(hip, nodes, prims, spheres=parked_spheres())
        t, prim, geom, uv = np_results(g.query_closest(z["origin"], z["direction"], z["distance_in"]))
        hit = z["hit"].astype(bool)
        assert np.array_equal(bits(t), bits(z["distance"])), name
        assert np.array_equal(prim >= 0, hit), name
        assert np.array_equal(prim[hit], z["identifier"][hit]), name
        assert np.all(prim[~hit] == -1) and np.all(geom[~hit] == -1) and np.all(geom[hit] == 1) and np.all(uv[~hit] == 0), name
        occ = g.query_any(z["origin"], z["direction"], z["closest"]).cpu().numpy()
        assert np.array_equal(occ, z["anyhit"].astype(bool)), name
        assert g.query_error() == 0
        g.close()


def c3_rays(rng, box, cam, n_cam=512 * 512, n_rand=786432):
    """camera rays through a 512 x 512 grid + random rays in the scene box, with random tmax (values below epsilon and inf
    among them)"""
    lo, hi = box
    ys, xs = np.meshgrid(np.linspace(-0.6, 0.6, 512, dtype=np.float32), np.linspace(-0.9, 0.9, 512, dtype=np.float32), indexing="ij")
    fwd, up = np.asarray(cam.direction, np.float32), np.asarray(cam.up, np.float32)
    right = np.cross(fwd, up).astype(np.float32)
    dc = fwd[None, :] + xs.reshape(-1, 1) * right[None, :] + ys.reshape(-1, 1) * up[None, :]
    dc = (dc / np.linalg.norm(dc, axis=1, keepdims=True)).astype(np.float32)
    oc = np.tile(np.asarray(cam.position, np.float32), (n_cam, 1))
    orand = (lo + (hi - lo) * rng.random((n_rand, 3))).astype(np.float32)
    o = np.concatenate([oc, orand]).astype(np.float32)
    d = np.concatenate([dc, random_dirs(rng, n_rand)]).astype(np.float32)
    n = o.shape[0]
    tmax = (rng.random(n) * 400.0).astype(np.float32)
    sel = rng.random(n)
    tmax[sel < 0.02] = (rng.random(int((sel < 0.02).sum())) * 2e-3).astype(np.float32)  # below / around epsilon
    tmax[(sel >= 0.02) & (sel < 0.05)] = np.inf
    tmax[(sel >= 0.05) & (sel < 0.3)] = np.float32(1e20)
    return o, d, tmax


@pytest.mark.gpu
def test_c3_tree_live_against_the_reference(orc, hip):
    """about a million rays through C3's 996,882-triangle tree, bit for bit against the reference harness (or the oracle)"""
    sc, nodes, prims = built_scene("mesh706")
    rng = np.random.default_rng(7)
    box = (nodes[0]["bounds"][0].astype(np.float32), nodes[0]["bounds"][1].astype(np.float32))
    o, d, tmax = c3_rays(rng, box, sc.camera)
    g = renderer(hip, nodes, prims, spheres=parked_spheres())
    t, prim, geom, uv = np_results(g.query_closest(o, d, tmax))
    want_t, want_p = oracle_closest(orc, nodes, prims, o, d, tmax)
    assert (want_p >= 0).sum() > o.shape[0] // 4
    assert np.array_equal(bits(t), bits(want_t)), f"{np.count_nonzero(bits(t) != bits(want_t))} distances differ"
    assert np.array_equal(prim, want_p)
    assert np.array_equal(geom, np.where(want_p >= 0, 1, -1))
    occ = g.query_any(o, d, tmax).cpu().numpy()
    assert np.array_equal(occ, oracle_any(orc, nodes, prims, o, d, tmax))
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_spheres_equal_the_extend_stage_and_intersect_scene(orc, hip):
    """TYR_QUERY_SPHERES: the render's own extend stage on the same records (tmax = VERY_FAR), and intersect_scene /
    intersect_scene_simple composed from the oracle's sphere and tree tests with a random tmax"""
    from tyrant_amd import scenes

    sc, nodes, prims = built_scene("cornell36")
    spheres = scenes.cornell_spheres()
    spheres[2] = (6.0, (-10.0, 0.0, 30.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), scenes.DIFF)  # two spheres inside the room
    spheres[5] = (8.0, (12.0, 20.0, 40.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), scenes.DIFF)
    rng = np.random.default_rng(11)
    n = 4096
    o = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(5, 80, n)], axis=1).astype(np.float32)
    d = random_dirs(rng, n)
    g = renderer(hip, nodes, prims, spheres=spheres, n=n)
    t, prim, geom, uv = np_results(g.query_closest(o, d, spheres=True))
    # the extend stage
    rays = _rays(o, d, np.full(n, 1e20, np.float32))
    rays["direct"] = 1.0
    g.stage("begin")
    g.import_work_queue(rays, n)
    g.set_budget(0)
    g.stage("primary")
    g.stage("extend")
    q = g.ray_queue(0, n)
    hit = q["distance"] < np.float32(1e20)
    assert (geom == 0).sum() > 50 and (geom == 1).sum() > 1000
    assert np.array_equal(bits(t), bits(q["distance"]))
    assert np.array_equal(prim[hit], q["identifier"][hit]) and np.array_equal(geom[hit], q["geometry_type"][hit])
    assert np.all(prim[~hit] == -1) and np.all(geom[~hit] == -1)
    assert np.all(uv[geom == 0] == 0)
    # intersect_scene with a caller's tmax
    tmax = (rng.random(n) * 120.0).astype(np.float32)
    t, prim, geom, _ = np_results(g.query_closest(o, d, tmax, spheres=True))
    wt, wp, wg = oracle_spheres_closest(orc, spheres, nodes, prims, o, d, tmax)
    assert np.array_equal(bits(t), bits(wt)) and np.array_equal(prim, wp) and np.array_equal(geom, wg)
    occ = g.query_any(o, d, tmax, spheres=True).cpu().numpy()
    want = oracle_spheres_any(orc, spheres, nodes, prims, o, d, tmax)
    assert np.array_equal(occ, want) and want.sum() > n // 4 and (~want).sum() > n // 8
    # without the flag the spheres are not asked
    occ0 = g.query_any(o, d, tmax).cpu().numpy()
    assert np.array_equal(occ0, oracle_any(orc, nodes, prims, o, d, tmax))
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_hostile_rays_and_batch_sizes(orc, hip):
    """axis-aligned rays in mixed waves through over-long leaves, NaN / Inf rays (misses), and n = 0, 1, 1000, 3 x queue_size"""
    import torch

    from tyrant_amd import scenes

    rng = np.random.default_rng(5)

    def stack(x0, k):
        return scenes.make_triangles(np.tile([x0 - 30, 0, 10], (k, 1)), np.tile([x0 + 30, 0, 10], (k, 1)), np.tile([x0, 0, 70], (k, 1)))

    tris = np.concatenate([scenes.cornell_box().triangles, stack(-10.0, 40), stack(15.0, 70)])
    nodes, prims = orc.bvh_build(tris, scenes.triangle_bboxes(tris))
    assert nodes["primitiveCount"].max() >= 40
    qsize = 4096
    n = 3 * qsize
    o = np.stack([rng.uniform(-45, 45, n), np.full(n, -100.0), rng.uniform(2, 98, n)], axis=1).astype(np.float32)
    axes = np.array([[0, 1, 0], [0, 1, 0], [0.6, 0.8, 0], [0, 0.8, 0.6], [0, 0.8, -0.6], [-0.6, 0.8, 0]], dtype=np.float32)
    dd = rng.normal(size=(n, 3)).astype(np.float32)
    dd[:, 1] = np.abs(dd[:, 1]) + 0.5
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    d = np.where((rng.random(n) < 0.5)[:, None], axes[rng.integers(0, len(axes), n)], dd).astype(np.float32)
    tmax = np.where(rng.random(n) < 0.5, np.float32(1e20), (rng.random(n) * 200).astype(np.float32)).astype(np.float32)
    bad = rng.random(n) < 0.03
    badval = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    where = rng.integers(0, 6, n)
    for i in np.nonzero(bad)[0]:
        (o if where[i] < 3 else d)[i, where[i] % 3] = badval[rng.integers(0, 3)]
    g = renderer(hip, nodes, prims, spheres=parked_spheres(), n=qsize)
    t, prim, geom, uv = np_results(g.query_closest(o, d, tmax))
    occ = g.query_any(o, d, tmax).cpu().numpy()
    ok = ~bad
    wt, wp = oracle_closest(orc, nodes, prims, o[ok], d[ok], tmax[ok])
    assert np.array_equal(bits(t[ok]), bits(wt)) and np.array_equal(prim[ok], wp)
    assert (wp >= 0).sum() > ok.sum() // 3
    assert np.array_equal(occ[ok], oracle_any(orc, nodes, prims, o[ok], d[ok], tmax[ok]))
    assert np.array_equal(bits(t[bad]), bits(tmax[bad])) and np.all(prim[bad] == -1) and np.all(geom[bad] == -1) and not occ[bad].any()
    # batch sizes: every prefix answers as the whole batch did
    for m in (0, 1, 63, 1000, qsize + 1):
        tm, pm, _, _ = np_results(g.query_closest(o[:m], d[:m], tmax[:m]))
        om = g.query_any(o[:m], d[:m], tmax[:m]).cpu().numpy()
        assert tm.shape == (m,) and np.array_equal(bits(tm), bits(t[:m])) and np.array_equal(pm, prim[:m]) and np.array_equal(om, occ[:m]), m
    # tmax omitted: VERY_FAR
    t2, p2, _, _ = np_results(g.query_closest(torch.from_numpy(o[:512]).cuda(), torch.from_numpy(d[:512]).cuda()))
    w2, wp2 = oracle_closest(orc, nodes, prims, o[:512][ok[:512]], d[:512][ok[:512]], np.full(ok[:512].sum(), 1e20, np.float32))
    assert np.array_equal(bits(t2[ok[:512]]), bits(w2)) and np.array_equal(p2[ok[:512]], wp2)
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_barycentrics(orc, hip):
    """uv = the winning triangle's u, v, bit-equal to a float32 restatement in glm's order; inside the triangle"""
    sc, nodes, prims = built_scene("cornell_soup2k")
    rng = np.random.default_rng(3)
    n = 65536
    o = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(5, 80, n)], axis=1).astype(np.float32)
    d = random_dirs(rng, n)
    g = renderer(hip, nodes, prims, spheres=parked_spheres())
    t, prim, geom, uv = np_results(g.query_closest(o, d))
    hit = prim >= 0
    assert hit.sum() > n // 2
    u, v = glm_uv(orc, prims, prim[hit], o[hit], d[hit])
    assert np.array_equal(bits(uv[hit, 0]), bits(u)) and np.array_equal(bits(uv[hit, 1]), bits(v))
    assert np.all(uv[hit] >= 0) and np.all(uv[hit].sum(axis=1) <= 1)
    assert np.all(uv[~hit] == 0)
    g.close()


@pytest.mark.gpu
def test_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with queries between its tyr_render calls: the same accumulation buffer and
    counters as without them"""
    rng = np.random.default_rng(1)
    o = np.stack([rng.uniform(-40, 40, 20000), rng.uniform(-40, 40, 20000), rng.uniform(5, 80, 20000)], axis=1).astype(np.float32)
    d = random_dirs(rng, 20000)

    def between(g):
        g.query_closest(o, d, spheres=True)
        g.query_any(o, d, np.full(20000, 50.0, np.float32), spheres=True)

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_side_stream_and_invalid_arguments(orc, hip):
    """queries on a torch side stream answer correctly once it is synchronised; bad arguments are refused before any launch"""
    import torch

    from tyrant_amd import scenes

    sc, nodes, prims = built_scene("cornell36")
    rng = np.random.default_rng(9)
    n = 50000
    o = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(5, 80, n)], axis=1).astype(np.float32)
    d = random_dirs(rng, n)
    tmax = (rng.random(n) * 100).astype(np.float32)
    g = renderer(hip, nodes, prims, spheres=parked_spheres())
    to, td, tt = (torch.from_numpy(a).cuda() for a in (o, d, tmax))
    (t, prim, geom, uv), occ = on_side_stream(lambda side: (g.query_closest(to, td, tt, stream=side), g.query_any(to, td, tt, stream=side)))
    wt, wp = oracle_closest(orc, nodes, prims, o, d, tmax)
    assert np.array_equal(bits(t.cpu().numpy()), bits(wt)) and np.array_equal(prim.cpu().numpy(), wp)
    assert np.array_equal(occ.cpu().numpy(), oracle_any(orc, nodes, prims, o, d, tmax))

    L, h = hip.lib(), g.h
    P = C.c_void_p
    tp, pp, op_ = (P(x.data_ptr()) for x in (t, prim, occ))
    oo, dd = P(to.data_ptr()), P(td.data_ptr())
    assert L.tyr_query_closest(None, 4, oo, dd, None, 0, tp, pp, None, None, None) == hip.TYR_ERR_INVALID
    assert L.tyr_query_closest(h, 4, None, dd, None, 0, tp, pp, None, None, None) == hip.TYR_ERR_INVALID
    assert L.tyr_query_closest(h, 4, oo, None, None, 0, tp, pp, None, None, None) == hip.TYR_ERR_INVALID
    assert L.tyr_query_closest(h, 4, oo, dd, None, 0, None, pp, None, None, None) == hip.TYR_ERR_INVALID
    assert L.tyr_query_closest(h, 4, oo, dd, None, 0, tp, None, None, None, None) == hip.TYR_ERR_INVALID
    assert L.tyr_query_closest(h, 4, oo, dd, None, 8, tp, pp, None, None, None) == hip.TYR_ERR_INVALID  # unknown flag
    assert L.tyr_query_closest(h, 1 << 31, oo, dd, None, 0, tp, pp, None, None, None) == hip.TYR_ERR_INVALID
    assert L.tyr_query_any(h, 4, oo, dd, None, 0, None, None) == hip.TYR_ERR_INVALID
    assert L.tyr_query_any(None, 4, oo, dd, None, 0, op_, None) == hip.TYR_ERR_INVALID
    assert L.tyr_query_closest(h, 0, None, None, None, 0, None, None, None, None, None) == 0  # n == 0: nothing to do
    bitsv = C.c_uint32(7)
    assert L.tyr_query_error(None, C.byref(bitsv), 0) == hip.TYR_ERR_INVALID
    assert L.tyr_query_error(h, None, 0) == hip.TYR_ERR_INVALID
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert L.tyr_query_closest(empty.h, 4, oo, dd, None, 0, tp, pp, None, None, None) == hip.TYR_ERR_NO_SCENE
    assert L.tyr_query_any(empty.h, 4, oo, dd, None, 0, op_, None) == hip.TYR_ERR_NO_SCENE
    assert L.tyr_query_error(empty.h, C.byref(bitsv), 1) == 0 and bitsv.value == 0
    empty.close()
    with pytest.raises(ValueError):
        g.query_closest(to.double(), td)
    with pytest.raises(ValueError):
        g.query_closest(to[:, :2].contiguous(), td)
    # the outputs were not touched by the refused calls
    assert np.array_equal(prim.cpu().numpy(), wp)
    # a scene without triangles: misses, or the spheres alone
    g.upload(np.zeros(0, dtype=scenes.NODE_DTYPE), np.zeros(0, dtype=scenes.TRIANGLE_DTYPE))
    t0, p0, g0, _ = np_results(g.query_closest(o[:1000], d[:1000], tmax[:1000]))
    assert np.array_equal(bits(t0), bits(tmax[:1000])) and np.all(p0 == -1) and np.all(g0 == -1)
    assert not g.query_any(o[:1000], d[:1000], tmax[:1000]).cpu().numpy().any()
    assert g.query_error() == 0
    g.close()
