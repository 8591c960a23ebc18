"""k_shade's dense path (TYR_TUNE_SHADE_DENSE): a tile's atmosphere requests and shadow-ray sphere / root-box
tests evaluated across its four waves on dense lanes, against the lane path (shade_dense = 0) on the same inputs.

Only requests and answers cross LDS and every lane applies its answers with the lane path's expressions in the lane path's
order, so everything a ray leaves behind is the same bits: the survivor queue, the shadow queue (both exports are in the
serial order: the physical order of the records is free), the survive bytes (through the rank tables of the scan), the
counters, and -- one record per pixel -- the accumulation buffer, which is each ray's own colour.

What runs, each with shade_dense 0 and with shade_dense 1:
    the crafted batches of tests/shade_cases.py (DIFF, SPEC, REFR, PHONG and LIGHT, both kinds of next-event sample, misses
        with either lastSpecular) in the sizes whose last tile has 1, 63, 64 and 65 valid lanes in a wave, stage by stage
        (two iterations) and through the render loop -- render(0), where shade folds the sphere tests, answers shadow
        rays in place and retires ghosts, and three launch_kernels, whose second iteration shades class-1 tiles;
    with TYR_FLAG_LIGHT_LIST (flags 1 | 8) the same: there is no dense kernel for the light list (hip/shade.hip), the key
        must change nothing there;
    two tiles without any request (records that end on a LIGHT sphere they do not see) in front of a mixed one;
    two tiles whose every lane holds a sun request, a ghost's request and a shadow candidate (512 + 256 requests a tile):
        zero seeds on the sun-facing cap of the DIFF sphere, where every draw is 0.0 -- the sample goes to the sun, the
        roulette passes, the bounce leaves along the normal and meets nothing; the oracle's trace shows the composition;
    class-1 tiles of a render as well: retire_sky = 0 queues the survivors that cannot enter the tree;
    one render of 64 x 48 at 4 spp, all primaries in the queue, on the small mesh scene.
Not reachable: sunAngularDiameterCos == 1.  The sun's size is a constant of host/sun_setup.cpp (kernel.cu:683) and no entry
point sets it; the shortcut (sunsky.cu:118-119) stays in the lane and makes no request on either path.
"""
import numpy as np
import pytest

import shade_cases as sc
from conftest import bits, built_scene

SIZES = (1, 63, 64, 65, 257, 2049)
SHADOW_FIELDS = ("origin", "direction", "color", "closestDistance", "buffer_index")


def same_records(a, b, fields, what):
    assert len(a) == len(b), what
    for f in fields:
        assert np.array_equal(bits(np.ascontiguousarray(a[f])), bits(np.ascontiguousarray(b[f]))), f"{what}: {f}"


def run_all(hip, flags, rays, W, H, frame, dense, **knobs):
    """the records stage by stage (two iterations), through render(0) and through three launch_kernels"""
    out = {}
    g = hip.Renderer(W, H, len(rays), flags=flags)
    sc.load(g, flags)
    g.set_tuning(shade_dense=dense, **knobs)
    out["staged"] = [sc.staged_iteration(g, i == 0, rays, frame) for i in range(2)]
    g.close()
    g = hip.Renderer(W, H, len(rays), flags=flags)
    sc.load(g, flags)
    g.set_tuning(shade_dense=dense, **knobs)
    sc.prime(g)
    for how in ("render", "launches"):
        out[how] = sc.drive(g, rays, frame, how)
    g.close()
    return out


def assert_same(want, got, what):
    from test_gpu_parity import assert_state_equal

    for i, (w, g) in enumerate(zip(want["staged"], got["staged"])):
        tag = f"{what} staged iteration {i}"
        for f in ("n_live", "ns", "nh", "n_survive", "total_shadow_rays", "visible", "rank_check"):
            assert w[f] == g[f], (tag, f, w[f], g[f])
        assert g["device_error"] == 0, tag
        assert_state_equal(w["survivors"], g["survivors"], tag + ": survivors")
        same_records(w["shadows"], g["shadows"], SHADOW_FIELDS, tag + ": shadow queue")
        assert np.array_equal(bits(w["accum_shade"]), bits(g["accum_shade"])), tag + ": per-ray colours"
        assert np.array_equal(bits(w["accum"]), bits(g["accum"])), tag + ": after connect"
    for how in ("render", "launches"):
        w, g = want[how], got[how]
        tag = f"{what} {how}"
        assert g["device_error"] == 0, tag
        for f in ("iterations", "left", "frame") + sc.RENDER_FIELDS:
            assert w[f] == g[f], (tag, f, w[f], g[f])
        assert np.array_equal(bits(w["accum"]), bits(g["accum"])), f"{tag}: {np.count_nonzero(np.any(bits(w['accum']) != bits(g['accum']), axis=1))} pixels differ"
        if how == "launches":
            assert_state_equal(w["queue"], g["queue"], tag + ": work queue")


def check(hip, flags, rays, W, H, frame, what, **knobs):
    want = run_all(hip, flags, rays, W, H, frame, 0, **knobs)
    assert_same(want, run_all(hip, flags, rays, W, H, frame, 1, **knobs), what)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (0, 1 | 8, 1 | 8 | 16))
def test_crafted_batches_bit_equal(orc, hip, flags):
    for n in SIZES:
        for order in ("shuffled", "sorted") if n == SIZES[-1] else ("shuffled",):
            b = sc.batch(flags, n, "one", order)
            check(hip, flags, b["rays"], b["W"], b["H"], 1, f"flags {flags} {order} {n}")


def aimed_at_sphere(which, normals, n_pixels_step, direct, last_specular):
    """records that meet sphere `which` head-on where its normal is normals[i], one per pixel i * n_pixels_step"""
    sp = sc.spheres()
    n = len(normals)
    r = np.zeros(n, dtype=sc.scenes.RAY_DTYPE)
    p = sp["position"][which].astype(np.float64) + normals * float(sp["radius"][which])
    r["origin"] = (p + normals * 6.0).astype(np.float32)
    d = (-normals).astype(np.float32)
    r["direction"] = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    r["direct"] = direct
    r["distance"] = sc.VERY_FAR
    r["bounces"] = 0
    r["lastSpecular"] = last_specular
    r["geometry_type"] = 1
    r["index"] = np.arange(n) * n_pixels_step
    return r


def oracle_first(rays, W, H, frame):
    """the oracle on a batch made here, before any GPU sees it (what does not end on the CPU must not reach a GPU): two staged
    iterations with the branch trace, and the unbounded drive"""
    from oracle import pyorc

    scene, nodes, prims = sc.scene(0)
    its = []
    for how in ("staged", "render"):
        o = pyorc.Oracle(W, H, len(rays), flags=0)
        o.load_scene(scene, nodes, prims)
        if how == "staged":
            o.set_shade_trace(True)
            its = [sc.staged_iteration(o, True, rays, frame, trace=True), sc.staged_iteration(o, False, trace=True)]
        else:
            sc.prime(o)
            sc.drive(o, rays, frame, "render")
        o.close()
    return its


@pytest.mark.gpu
def test_tiles_without_a_request(orc, hip):
    """512 records that end on the LIGHT sphere without seeing it (no sample, no survivor, nothing for the dense phase: its
    loops run zero times and its barriers are still met), then 40 records of the mixed batch"""
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(512, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    dark = aimed_at_sphere(4, nrm, 1, 1.0, False)
    mixed, _ = sc.make_rays(40, 77, negative_ok=True, all_safe=True)
    mixed["index"] = 512 + np.arange(40)
    rays = np.concatenate([dark, mixed])
    oracle_first(rays, 640, 1, 1)
    want = check(hip, 0, rays, 640, 1, 1, "no requests")
    assert want["staged"][0]["n_live"] == 552 and want["staged"][0]["ns"] <= 40 and want["staged"][0]["nh"] <= 40


@pytest.mark.gpu
def test_tiles_with_two_requests_and_a_candidate_in_every_lane(orc, hip):
    n, frame = 512, sc.ZERO_SEED_FRAME
    rng = np.random.default_rng(6)
    nrm = sc.sun_direction() + 0.15 * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rays = aimed_at_sphere(0, nrm, 2, (1.0, 1.0, 1.0), False)  # even pixels at frame 2^31: every seed is 0
    assert (sc.seeds(rays, frame) == 0).all()
    first, second = oracle_first(rays, 2 * n, 1, frame)
    for name in ("NEE_SUN_DIFF", "SHADOW_RAY", "SURVIVED"):  # a sun request and a shadow candidate in every lane ...
        assert sc.has(first["trace"], name).all(), name
    assert second["n_live"] == n and sc.has(second["trace"], "MISS").all()  # ... whose survivor meets nothing: a ghost where they are retired
    want = check(hip, 0, rays, 2 * n, 1, frame, "two requests a lane")
    assert want["render"]["n_survive"] == n and want["render"]["total_shadow_rays"] == n
    check(hip, 0, rays, 2 * n, 1, frame, "two requests a lane, ghosts queued as class 1", retire_sky=0)


@pytest.mark.gpu
def test_class_1_tiles_of_a_render(orc, hip):
    b = sc.batch(1, 2049, "one", "sorted")
    check(hip, 1, b["rays"], b["W"], b["H"], 1, "retire_sky 0", retire_sky=0)
    check(hip, 1, b["rays"], b["W"], b["H"], 1, "resolve_shadows 0", resolve_shadows=0)


@pytest.mark.gpu
def test_small_render_same_counters_and_radiance(orc, hip):
    from test_gpu_parity import assert_accum_close

    scene, nodes, prims = built_scene("mesh32")
    W, H, spp = 64, 48, 4
    res = {}
    for d in (0, 1):
        g = hip.Renderer(W, H, W * H * spp, flags=1 if scene.triangle_materials else 0)
        g.load_scene(scene, nodes, prims)
        g.set_tuning(shade_dense=d)
        it = g.render(spp)
        k = g.counters()
        res[d] = (it, {f: k[f] for f in ("device_error", "total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible")}, g.blit_buffer())
        g.close()
    assert res[0][1]["device_error"] == 0 and res[0][1]["total_shadow_rays"] > 0
    assert res[1][0] == res[0][0] and res[1][1] == res[0][1], (res[1][:2], res[0][:2])
    assert_accum_close(res[0][2], res[1][2], "shade_dense 1 against 0")
