"""Specular-chain guides (tyr_render_aov_chain, tyr_render_motion_chain; include/tyr_c.h "Specular-chain guides"): the AOV
guides taken at the end of each sample's deterministic mirror / glass chain, and the motion of the virtual image point.

CPU: the restatement (tests/specular_ref.py) pinned to the oracle's own shade, so that it and not the GPU is the specification;
the coverage of the test scenes below; what the compiler made of the chain kernel; the committed bench figures.  GPU: the pass
against the restatement bit for bit on every pixel; max_chain 0 against tyr_render_aov; the motion pass; isolation, arguments,
streams; the example's switch; the quality the guides buy (tools/specular_guides_bench.py).

Quality figures measured on an MI355X (profiles/specular_guides_bench.json), chain guides over first-hit guides on the chain
pixels: see test_quality_of_the_chain_guides."""
import ctypes as C
import dataclasses
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_ref
import specular_ref as sr
import test_aov
import test_temporal
from conftest import ROOT, bits, built_scene
from kernel_resources import kernel_resources

CSRC = os.path.join(ROOT, "tyrant_amd", "csrc")
BENCH = os.path.join(ROOT, "profiles", "specular_guides_bench.json")
VERY_FAR = np.float32(1e20)
SENTINEL = test_aov.SENTINEL
W, H = 96, 64
AOV_KEYS = ("albedo", "normal", "depth", "prim", "geom")
EXT_KEYS = ("chain", "end_prim", "end_geom", "length0", "depth_first")
MARGIN = 1.2  # the project's margin for the renders' float atomics (tests/test_temporal.py)


# ---- the test scenes: what the default fixtures at their default cameras do not reach ----------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, nodes, prims), the tree by the oracle's builder
    table         the reference's sphere table (a SPEC and a REFR sphere) seen from close by
    strip         cornell_colored aimed at its grey mirror strip: a palette-coloured mirror
    hall          two facing SPEC quads in the Cornell room seen at a grazing angle: chains that reach the cap
    inside_glass  a camera inside a large REFR sphere looking near-tangentially: leaving refraction and total internal reflection"""
    from oracle import pyorc
    from tyrant_amd import scenes

    cam = lambda p, d: scenes.Camera(position=p, direction=d, up=(0.0, 0.0, 1.0), focalDistance=1.0, lensRadius=0.0)  # noqa: E731
    if name == "table":
        sc = dataclasses.replace(scenes.tyrant_default(), camera=cam((0.0, -130.0, 35.0), (0.0, 1.0, -0.1)))
    elif name == "strip":
        sc = dataclasses.replace(scenes.cornell_colored(), camera=cam((0.0, -60.0, 70.0), (0.0, 1.0, 0.0)))
    elif name == "hall":
        a = scenes._quad((-20, -50, 0), (-20, 50, 0), (-20, 50, 100), (-20, -50, 100), (1, 0, 0))
        b = scenes._quad((20, 50, 0), (20, -50, 0), (20, -50, 100), (20, 50, 100), (-1, 0, 0))
        a["materialType"] = scenes.SPEC
        b["materialType"] = scenes.SPEC
        sc = scenes.SceneData("hall", np.concatenate([scenes.room_walls(), a, b]), scenes.cornell_spheres(), cam((0.0, -45.0, 50.0), (1.0, 0.15, 0.0)), triangle_materials=True)
    elif name == "inside_glass":
        spheres = scenes.cornell_spheres(light_z=300.0)
        spheres[0] = (40.0, (0.0, 0.0, 50.0), (0.02, 0.01, 0.01), (0.0, 0.0, 0.0), scenes.REFR)
        sc = scenes.SceneData("inside_glass", scenes.room_walls(), spheres, cam((0.0, -35.0, 50.0), (1.0, 0.0, 0.2)))
    else:
        raise KeyError(name)
    nodes, prims = pyorc.bvh_build(sc.triangles, scenes.triangle_bboxes(sc.triangles))
    return sc, nodes, prims


SCENES = ("table", "strip", "hall", "inside_glass")


def oracle_queue(orc, sc, nodes, prims, spp, frame=None, rank=0, nranks=1, w=W, h=H):
    return aov_ref.oracle_queue(orc, sc, nodes, prims, spp, w, h, frame=frame, rank=rank, nranks=nranks)


def restated(orc, name, spp, max_chain, **kw):
    sc, nodes, prims = scene(name) if name in SCENES else built_scene(name)
    o, q = oracle_queue(orc, sc, nodes, prims, spp, **kw)
    res = sr.expected_chain(o, q, sc, prims, np.ascontiguousarray(sc.spheres), spp, max_chain)
    o.close()
    return res


# ---- CPU: the restatement against the oracle's own shade ------------------------------------------------------------------------
def shade_survivors(orc, name):
    """the first wavefront at 1 spp, its surfaces by the restatement, and the survivor that the oracle's shade wrote per pixel"""
    sc, nodes, prims = scene(name)
    o, q = oracle_queue(orc, sc, nodes, prims, 1)
    o.stage("shade")
    surv = o.ray_queue(1, o.counters()["primary_ray_cnt"])
    lib = o.L
    o.close()
    hit = q["distance"] < VERY_FAR
    s = sr.surface(lib, q[hit], sc, prims, np.ascontiguousarray(sc.spheres))
    by_pixel = {int(r["index"]): r for r in surv}  # 1 spp: one ray per pixel
    return lib, q[hit], s, by_pixel


def test_spec_step_equals_the_oracles_shade(orc):
    """rays whose first hit is SPEC: the step's (o', d') are the survivor record's origin and direction bit for bit (shade draws
    no random number for SPEC; a ray that Russian roulette ended has no record)"""
    checked = {"sphere": 0, "triangle": 0}
    for name in ("table", "strip", "hall"):
        lib, q, s, surv = shade_survivors(orc, name)
        o2, d2 = sr.spec_step(lib, s)
        for i in np.flatnonzero(s["material"] == sr.SPEC):
            r = surv.get(int(q["index"][i]))
            if r is None:
                continue
            assert np.array_equal(bits(r["origin"]), bits(o2[i])) and np.array_equal(bits(r["direction"]), bits(d2[i])), (name, i)
            checked["sphere" if q["geometry_type"][i] == 0 else "triangle"] += 1
    assert checked["sphere"] >= 50 and checked["triangle"] >= 50, checked


def test_refr_step_candidates_are_the_oracles_shade(orc):
    """every survivor of a REFR hit is the step's reflect candidate or its transmit candidate bit for bit; both occur, entering
    and leaving, and so does total internal reflection (where shade's survivor is the reflect candidate)"""
    seen = {"reflect": 0, "transmit_in": 0, "transmit_out": 0, "tir": 0}
    for name in ("table", "inside_glass"):
        lib, q, s, surv = shade_survivors(orc, name)
        (o_r, d_r), (o_t, d_t), tir = sr.refr_step(lib, s)
        for i in np.flatnonzero(s["material"] == sr.REFR):
            r = surv.get(int(q["index"][i]))
            if r is None:
                continue
            same = lambda o, d: np.array_equal(bits(r["origin"]), bits(o[i])) and np.array_equal(bits(r["direction"]), bits(d[i]))  # noqa: E731
            refl, trans = same(o_r, d_r), same(o_t, d_t)
            assert refl or trans, (name, i)
            if tir[i]:
                assert refl, (name, i)
                seen["tir"] += 1
            elif refl:
                seen["reflect"] += 1
            else:
                seen["transmit_in" if s["outside"][i] else "transmit_out"] += 1
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("name", ["cornell36", "cornell_colored", "glass_dof48", "mesh128"])
def test_restatement_without_chains_is_the_first_hit_definition(orc, name):
    """max_chain = 0: the restatement equals test_aov.expected_aov on the oracle's first wavefront; chain 0, the end ids the
    first ids, length0 sample 0's t, depth_first the depth"""
    hip = aov_ref.OracleMath(orc.lib())
    sc, nodes, prims = built_scene(name)
    spp = 3
    o, q = oracle_queue(orc, sc, nodes, prims, spp)
    pix, got, _ = sr.expected_chain(o, q, sc, prims, np.ascontiguousarray(sc.spheres), spp, 0)
    o.close()
    pix2, want = test_aov.expected_aov(hip, q, sc, prims, np.ascontiguousarray(sc.spheres), spp, W, H, sc.triangle_colors)
    assert np.array_equal(pix, pix2)
    for k in ("albedo", "normal", "depth"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(got["prim"], want["prim"]) and np.array_equal(got["geom"], want["geom"])
    assert not got["chain"].any() and np.array_equal(got["end_prim"], want["prim"]) and np.array_equal(got["end_geom"], want["geom"])
    assert np.array_equal(bits(got["depth_first"]), bits(want["depth"]))
    t0 = q[: W * H]["distance"]
    assert np.array_equal(bits(got["length0"]), bits(np.where(t0 < VERY_FAR, t0, VERY_FAR)))


def test_the_test_scenes_cover_every_branch(orc):
    """over the scenes the GPU comparison runs (8 spp, max_chain 8): at least 50 samples each of a SPEC sphere, a SPEC triangle,
    REFR entering, REFR leaving a sphere, total internal reflection, a chain that leaves the scene after a bounce, a chain stopped
    by max_chain, a chain of three or more bounces, and a palette-coloured mirror with T != 1"""
    total, long3 = {}, 0
    for name in SCENES:
        sc, nodes, prims = scene(name)
        o, q = oracle_queue(orc, sc, nodes, prims, 8)
        c = sr.chain_samples(o, q, sc, prims, np.ascontiguousarray(sc.spheres), 8)
        o.close()
        for k, v in c["events"].items():
            total[k] = total.get(k, 0) + v
        long3 += int((c["chain"] >= 3).sum())
    total["chain_of_3"] = long3
    assert all(v >= 50 for v in total.values()), total


def test_chain_kernel_keeps_registers_and_lds_in_budget():
    """k_render_chain as the build reports it: 103 VGPRs, which is four waves per SIMD (k_render_aov: 75 and five); no vector
    spill; scratch no larger than the LdsStack's private spill arrays (k_render_aov's 432 bytes); LDS that admits five blocks per
    CU.  k_render_aov is the same body without the chain (aov_body<false>): test_aov's own test holds its five."""
    res = kernel_resources("aov")
    names = [n for n in res if "k_render_chain" in n]
    assert len(names) == 1, list(res)
    k = res[names[0]]
    assert k["VGPRs Spill"] == 0, k
    assert k["ScratchSize [bytes/lane]"] <= 432, k
    assert k["VGPRs"] <= 104 and k["Occupancy [waves/SIMD]"] >= 4, k
    per_block = -(-k["LDS Size [bytes/block]"] // test_aov.LDS_GRANULE) * test_aov.LDS_GRANULE
    assert test_aov.LDS_PER_CU // per_block >= 5, k
    m = kernel_resources("temporal")
    names = [n for n in m if "k_motion_chain" in n]
    assert len(names) == 1, list(m)
    k = m[names[0]]
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["ScratchSize [bytes/lane]"] == 0 and k["LDS Size [bytes/block]"] == 0 and k["Occupancy [waves/SIMD]"] >= 8, k


def committed():
    with open(BENCH) as f:
        return json.load(f)["quality"]


def bound(ratio):
    """the committed ratio with the margin, never above 1: at 1 the guides buy nothing"""
    return min(ratio * MARGIN, 1.0)


def test_bench_ratios_back_the_bounds():
    """profiles/specular_guides_bench.json holds the figures the GPU tests bound, measured with the defaults on a frame where at
    least a fifth of the pixels have a chain; both chain-pixel ratios are below 1"""
    q = committed()
    assert "128x72" in q["workload"] and "1024 spp" in q["workload"] and q["chain_share"] >= 0.2
    for recipe in ("still", "pan"):
        r = q[recipe]
        assert r["chain_pixels"] >= 0.2 * 128 * 72 * 0.9
        assert abs(r["ratio_chain_pixels"] - r["mse_chain_chain_pixels"] / r["mse_first_chain_pixels"]) < 1e-12
        assert 0 < r["ratio_chain_pixels"] < 1.0, (recipe, r)
    assert 0 < q["mirror_reprojection"]["share_within_depth_tolerance"] <= 1.0 and q["mirror_reprojection"]["mirror_pixels"] > 500


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def chain_into(hip, g, spp, max_chain, which=AOV_KEYS + EXT_KEYS, stream=None, fill=SENTINEL):
    """tyr_render_aov_chain into buffers pre-filled with `fill`: (status, dict of numpy arrays, flattened per pixel)"""
    import torch

    dev = torch.device("cuda", g.device)
    n = g.H * g.W
    floats = {"albedo": 3, "normal": 3, "depth": 1, "length0": 1, "depth_first": 1}
    bufs = {k: torch.full((n, floats[k]) if floats.get(k, 1) == 3 else (n,), fill, dtype=torch.float32 if k in floats else torch.int32, device=dev) for k in AOV_KEYS + EXT_KEYS}
    out = hip.AovOut(*(bufs[k].data_ptr() if k in which else None for k in AOV_KEYS))
    ext = hip.AovChainOut(*(bufs[k].data_ptr() if k in which else None for k in EXT_KEYS))
    s = stream if stream is not None else torch.cuda.current_stream(g.device)
    torch.cuda.synchronize(g.device)
    rc = g.L.tyr_render_aov_chain(g.h, spp, max_chain, C.byref(out), C.byref(ext), s.cuda_stream if s.cuda_stream else None)
    torch.cuda.synchronize(g.device)
    return rc, {k: v.cpu().numpy() for k, v in bufs.items()}


def assert_chain_equal(got, pix, want, what):
    for k in ("albedo", "normal", "depth", "length0", "depth_first"):
        g = got[k].reshape(got[k].shape[0], -1)[pix]
        w = want[k].reshape(want[k].shape[0], -1)
        bad = (bits(g) != bits(w)).any(axis=-1)
        assert not bad.any(), f"{what} {k}: {int(bad.sum())} pixels differ, first {int(pix[np.flatnonzero(bad)[0]])}"
    for k in ("prim", "geom", "chain", "end_prim", "end_geom"):
        bad = got[k][pix] != want[k]
        assert not bad.any(), f"{what} {k}: {int(bad.sum())} pixels differ"


def renderer(hip, name, w=W, h=H, **kw):
    sc, nodes, prims = scene(name) if name in SCENES else built_scene(name)
    g = hip.Renderer(w, h, 4096, flags=test_aov.flags_of(sc) | kw.pop("flags", 0), **kw)
    g.load_scene(sc, nodes, prims)
    return g, sc, nodes, prims


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_chain_aov_equals_the_restatement(orc, hip, name):
    """every pixel of every test scene, every output, bit for bit: spp 1, 3, 8 x max_chain 1, 4, 8; and the Python entry point"""
    g, sc, nodes, prims = renderer(hip, name)
    chained = 0
    for spp in (1, 3, 8):
        for mc in (1, 4, 8):
            pix, want, _ = restated(orc, name, spp, mc)
            assert pix.size == W * H
            rc, got = chain_into(hip, g, spp, mc)
            assert rc == 0, rc
            assert_chain_equal(got, pix, want, f"{name} spp {spp} max_chain {mc}")
            chained += int((want["chain"] > 0).sum())
    assert chained > 9 * 50, chained
    res = g.render_aov(8, max_chain=8)
    assert set(res) == set(AOV_KEYS + EXT_KEYS) and tuple(res["albedo"].shape) == (H, W, 3) and tuple(res["chain"].shape) == (H, W)
    for k in AOV_KEYS + EXT_KEYS:  # (pix, want: the last case above)
        assert res[k].cpu().numpy().reshape(W * H, -1)[pix].tobytes() == want[k].tobytes(), k
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_chain_aov_at_another_frame_and_on_a_shard(orc, hip):
    """set_frame(7) on a scene with a thin lens is another set of rays; a ctx with nranks = 2, rank = 1 against an oracle ctx of
    that rank, and the other rank's rows keep their contents"""
    g, sc, nodes, prims = renderer(hip, "glass_dof48")
    g.set_frame(7)
    pix, want, _ = restated(orc, "glass_dof48", 3, 4, frame=7)
    rc, got = chain_into(hip, g, 3, 4)
    assert rc == 0 and g.counters()["frame"] == 7
    assert_chain_equal(got, pix, want, "frame 7")
    pix1, want1, _ = restated(orc, "glass_dof48", 3, 4)
    assert not np.array_equal(bits(want1["depth"]), bits(want["depth"]))
    g.close()
    for name in ("hall", "table"):
        h, sc, nodes, prims = renderer(hip, name, rank=1, nranks=2)
        pix, want, _ = restated(orc, name, 3, 8, rank=1, nranks=2)
        rc, got = chain_into(hip, h, 3, 8)
        assert rc == 0 and np.all(pix // W % 2 == 1) and pix.size == W * H // 2
        assert_chain_equal(got, pix, want, f"{name} rank 1 of 2")
        other = (np.arange(H * W) // W) % 2 == 0
        for k in AOV_KEYS + EXT_KEYS:
            assert np.all(got[k][other] == (np.float32(SENTINEL) if got[k].dtype == np.float32 else int(SENTINEL))), k
        assert h.query_error() == 0
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell36", "cornell_colored", "glass_dof48", "mesh128"])
def test_chain_aov_without_chains_equals_render_aov(hip, name):
    """max_chain = 0: every output shared with tyr_render_aov is its bits; chain 0, the end ids the first ids, depth_first the
    depth; 1 spp: length0 the depth"""
    g, sc, nodes, prims = renderer(hip, name)
    for spp in (1, 3, 8):
        rc, want = test_aov.aov_into(hip, g, spp)
        rc2, got = chain_into(hip, g, spp, 0)
        assert rc == 0 and rc2 == 0
        for k in AOV_KEYS:
            assert got[k].tobytes() == want[k].tobytes(), (spp, k)
        assert not got["chain"].any() and np.array_equal(got["end_prim"], want["prim"]) and np.array_equal(got["end_geom"], want["geom"])
        assert got["depth_first"].tobytes() == want["depth"].tobytes()
        if spp == 1:
            assert got["length0"].tobytes() == want["depth"].tobytes()
    g.close()


# ---- motion ------------------------------------------------------------------------------------------------------------------
def mirror_room():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import specular_guides_bench as sgb

    return sgb


@pytest.mark.gpu
def test_motion_chain_follows_the_virtual_point(orc, hip):
    """a translated and turned camera on the strip, hall and table scenes: where chain == 0 the bits of tyr_render_motion; where
    chain > 0 the float64 projection of o + d * length0 through both cameras within check_motion's tolerance, (0, 0) and VERY_FAR
    where the chain left the scene; an unchanged camera gives exactly (0, 0) everywhere"""
    seen = 0
    for name in ("strip", "hall", "table"):
        g, sc, nodes, prims = renderer(hip, name)
        prev = sc.camera
        cur = test_temporal.moved_camera(prev, -0.3)
        g.set_camera(cur)
        aov = g.render_aov(1, max_chain=8)
        plain = g.render_motion(aov["prim"], aov["geom"], prev)
        got = g.render_motion(aov["prim"], aov["geom"], prev, chain=aov["chain"], length0=aov["length0"])
        chain = aov["chain"].cpu().numpy().reshape(-1)
        length0 = aov["length0"].cpu().numpy().reshape(-1)
        for k in ("motion", "prev_depth"):
            a, b = got[k].cpu().numpy().reshape(W * H, -1), plain[k].cpu().numpy().reshape(W * H, -1)
            assert np.array_equal(bits(a[chain == 0]), bits(b[chain == 0])), (name, k)
        q = test_temporal.sample0_rays(orc, sc, nodes, prims, cur, W, H)
        q = q[chain[q["index"]] > 0]
        reach = length0[q["index"]]
        X = q["origin"].astype(np.float64) + q["direction"].astype(np.float64) * reach.astype(np.float64)[:, None]
        xc, yc, fc = test_temporal.project64(X, cur, W, H)
        xp, yp, fp = test_temporal.project64(X, prev, W, H)
        valid = (reach < VERY_FAR) & (fc > 0) & (fp > 0)
        want = (q["index"], np.stack([xp - xc, yp - yc], 1), np.linalg.norm(X - np.array(prev.position, np.float64), axis=1), valid)
        inframe = test_temporal.check_motion(got, want, W, H, name)
        seen += int(inframe.sum())
        assert (~valid).sum() > 0 or name != "strip"  # the strip mirrors the room's open side: chains that leave the scene
        same = g.render_motion(aov["prim"], aov["geom"], cur, chain=aov["chain"], length0=aov["length0"])
        assert np.all(bits(same["motion"].cpu().numpy()) == 0)
        pd = same["prev_depth"].cpu().numpy().reshape(-1)
        assert np.all(pd[(chain > 0) & (length0 == VERY_FAR)] == VERY_FAR) and np.all(pd[(chain > 0) & (length0 < VERY_FAR)] < VERY_FAR)
        g.close()
    assert seen > 300, seen


@pytest.mark.gpu
def test_motion_chain_finds_the_previous_depth_in_a_planar_mirror(hip):
    """the mirror room's planar mirrors under a camera moved by eight pan steps: at the reprojected pixel the previous frame's
    chain depth agrees with prev_depth within tyr_temporal's default depth_tolerance on (nearly) every mirror pixel -- the
    share recorded in profiles/specular_guides_bench.json, with the project's margin"""
    sgb = mirror_room()
    got = sgb.mirror_reprojection()
    rec = committed()["mirror_reprojection"]
    print("mirror reprojection:", got, "recorded:", rec)
    assert got["mirror_pixels"] > 500
    assert got["share_within_depth_tolerance"] >= rec["share_within_depth_tolerance"] / MARGIN, (got, rec)


# ---- state, arguments, streams -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_passes_leave_the_render_and_filter_state_alone(hip):
    """counters, frame, accumulation, both queue exports before and after the two passes are the same; a temporal / svgf / taa
    call after them gives what it gives without them (their histories are untouched)"""
    import torch

    def run(with_chain):
        g, sc, nodes, prims = renderer(hip, "hall")
        g.render(1, 2)  # mid-render: survivors in the queue
        aov = g.render_aov(1)
        mot = g.render_motion(aov["prim"], aov["geom"], sc.camera)
        ins = (aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"])
        first = (g.temporal(*ins), g.svgf(*ins), g.taa(g.svgf(*ins, resolve=True), aov["depth"], mot["motion"], mot["prev_depth"]))
        before = (g.counters(), g.blit_buffer(), g.ray_queue(0), g.ray_queue(1))
        if with_chain:
            ch = g.render_aov(3, max_chain=8)
            g.render_motion(ch["prim"], ch["geom"], test_temporal.moved_camera(sc.camera, 0.2), chain=ch["chain"], length0=ch["length0"])
            torch.cuda.synchronize()
        after = (g.counters(), g.blit_buffer(), g.ray_queue(0), g.ray_queue(1))
        assert before[0] == after[0]
        for x, y in zip(before[1:], after[1:]):
            assert x.tobytes() == y.tobytes()
        second = (g.temporal(*ins), g.svgf(*ins), g.taa(g.svgf(*ins, resolve=True), aov["depth"], mot["motion"], mot["prev_depth"]))
        torch.cuda.synchronize()
        out = [t.cpu().numpy() for t in first + second]
        assert g.query_error() == 0
        g.close()
        return out

    for a, b in zip(run(True), run(False)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_chain_arguments_partial_outputs_and_streams(hip):
    """every TYR_ERR_INVALID case and TYR_ERR_NO_SCENE; an output left NULL is not written, ext may be NULL; a side stream gives
    the same answer; tyr_query_error stays 0"""
    import torch

    sc, nodes, prims = scene("table")
    g = hip.Renderer(W, H, 4096)
    dev = torch.device("cuda", 0)
    buf = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    ibuf = torch.zeros(W * H, dtype=torch.int32, device=dev)
    one = hip.AovOut(buf.data_ptr(), None, None, None, None)
    only_ext = hip.AovChainOut(ibuf.data_ptr(), None, None, None, None)
    call = g.L.tyr_render_aov_chain
    assert call(g.h, 1, 1, C.byref(one), None, None) == hip.TYR_ERR_NO_SCENE
    g.load_scene(sc, nodes, prims)
    assert call(g.h, 1, hip.AOV_CHAIN_MAX + 1, C.byref(one), None, None) == hip.TYR_ERR_INVALID
    assert call(g.h, 1, 1, None, C.byref(only_ext), None) == hip.TYR_ERR_INVALID
    assert call(g.h, 1, 1, C.byref(hip.AovOut()), None, None) == hip.TYR_ERR_INVALID
    assert call(g.h, 1, 1, C.byref(hip.AovOut()), C.byref(hip.AovChainOut()), None) == hip.TYR_ERR_INVALID
    assert call(g.h, 0, 1, C.byref(one), None, None) == hip.TYR_ERR_INVALID
    assert call(g.h, (1 << 32) // (W * H) + 1, 1, C.byref(one), None, None) == hip.TYR_ERR_INVALID
    assert call(None, 1, 1, C.byref(one), None, None) == hip.TYR_ERR_INVALID
    assert call(g.h, 1, hip.AOV_CHAIN_MAX, C.byref(one), None, None) == 0
    assert call(g.h, 1, 1, C.byref(hip.AovOut()), C.byref(only_ext), None) == 0  # ext alone is an output
    torch.cuda.synchronize()
    full = chain_into(hip, g, 3, 8)[1]
    assert np.array_equal(ibuf.cpu().numpy(), chain_into(hip, g, 1, 1)[1]["chain"])
    for which in (("albedo",), ("normal", "prim", "chain"), ("depth", "geom", "length0"), ("end_prim", "end_geom", "depth_first")):
        rc, part = chain_into(hip, g, 3, 8, which=which)
        assert rc == 0
        for k in part:
            if k in which:
                assert part[k].tobytes() == full[k].tobytes(), (which, k)
            else:
                assert np.all(part[k] == (np.float32(SENTINEL) if part[k].dtype == np.float32 else int(SENTINEL))), (which, k)
    side = torch.cuda.Stream(dev)
    rc, on_side = chain_into(hip, g, 3, 8, stream=side)
    assert rc == 0
    for k in full:
        assert on_side[k].tobytes() == full[k].tobytes(), k
    res = g.render_aov(3, max_chain=8, stream=side)
    assert np.array_equal(bits(res["depth"].cpu().numpy().reshape(-1)), bits(full["depth"]))
    with pytest.raises(hip.TyrError):
        g.render_aov(1, max_chain=9)

    # the motion pass
    aov = g.render_aov(1, max_chain=8)
    cam = hip.CameraC((C.c_float * 3)(*sc.camera.position), (C.c_float * 3)(*sc.camera.direction), (C.c_float * 3)(*sc.camera.up), 1.0, 0.0)
    mi = hip.MotionIn(aov["prim"].data_ptr(), aov["geom"].data_ptr(), C.cast(C.pointer(cam), C.c_void_p), None)
    via = hip.MotionChainIn(aov["chain"].data_ptr(), aov["length0"].data_ptr())
    m = torch.full((W * H, 2), SENTINEL, dtype=torch.float32, device=dev)
    d = torch.full((W * H,), SENTINEL, dtype=torch.float32, device=dev)
    mcall = g.L.tyr_render_motion_chain
    both = hip.MotionOut(m.data_ptr(), d.data_ptr())
    assert mcall(g.h, C.byref(mi), None, C.byref(both), None) == hip.TYR_ERR_INVALID
    assert mcall(g.h, C.byref(mi), C.byref(hip.MotionChainIn(aov["chain"].data_ptr(), None)), C.byref(both), None) == hip.TYR_ERR_INVALID
    assert mcall(g.h, C.byref(mi), C.byref(hip.MotionChainIn(None, aov["length0"].data_ptr())), C.byref(both), None) == hip.TYR_ERR_INVALID
    assert mcall(g.h, None, C.byref(via), C.byref(both), None) == hip.TYR_ERR_INVALID
    assert mcall(g.h, C.byref(mi), C.byref(via), None, None) == hip.TYR_ERR_INVALID
    assert mcall(g.h, C.byref(mi), C.byref(via), C.byref(hip.MotionOut()), None) == hip.TYR_ERR_INVALID
    assert mcall(None, C.byref(mi), C.byref(via), C.byref(both), None) == hip.TYR_ERR_INVALID
    assert mcall(g.h, C.byref(mi), C.byref(via), C.byref(hip.MotionOut(m.data_ptr(), None)), side.cuda_stream) == 0
    side.synchronize()
    assert np.all(d.cpu().numpy() == np.float32(SENTINEL))
    want = g.render_motion(aov["prim"], aov["geom"], sc.camera, chain=aov["chain"], length0=aov["length0"])
    torch.cuda.synchronize()
    assert m.cpu().numpy().tobytes() == want["motion"].cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        g.render_motion(aov["prim"], aov["geom"], sc.camera, chain=aov["chain"])
    empty = hip.Renderer(W, H, 4096)
    assert empty.L.tyr_render_motion_chain(empty.h, C.byref(mi), C.byref(via), C.byref(both), None) == hip.TYR_ERR_NO_SCENE
    empty.close()
    assert g.query_error() == 0
    g.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_example_with_and_without_specular_guides(hip, tmp_path):
    """denoised_flythrough: without the switch its frames are what they were (the same bytes as a second run without it); with
    --specular-guides the frames are written too, say so on stdout, and differ"""
    exe = os.path.join(ROOT, "tyrant_amd", "bin", "denoised_flythrough")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, "example"], check=True)

    def run(tag, *extra):
        d = tmp_path / tag
        d.mkdir()
        p = subprocess.run([exe, "0", "3", "1", str(d / "f"), "320", "180", *extra], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}, p.stdout

    plain, out0 = run("a")
    again, _ = run("b")
    guided, out1 = run("c", "--specular-guides")
    capped, out2 = run("d", "--specular-guides=2")
    assert plain and plain == again
    assert sorted(guided) == sorted(plain) == sorted(capped)
    assert "specular guides" not in out0 and "specular guides: max_chain 8" in out1 and "specular guides: max_chain 2" in out2
    assert any(guided[n] != plain[n] for n in plain)


# ---- quality -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_quality_of_the_chain_guides(hip):
    """the mirror room at 128 x 72 against 1024-spp renders, chain guides over first-hit guides on the pixels with a chain: a
    4-spp still frame through tyr_denoise, and the last of 16 panned 1-spp frames through motion + tyr_svgf, each at most the
    committed ratio x 1.2 and never above 1 (measured on an MI355X: still 0.225, pan 0.481 -- profiles/specular_guides_bench.json)"""
    sgb = mirror_room()
    q = sgb.quality()
    rec = committed()
    print("quality:", json.dumps({k: q[k] for k in ("chain_share", "still", "pan")}), "recorded:", json.dumps({k: rec[k] for k in ("chain_share", "still", "pan")}))
    assert q["chain_share"] >= 0.2 and q["still"]["chain_pixels"] >= 0.2 * 128 * 72 * 0.9
    assert q["still"]["ratio_chain_pixels"] <= bound(rec["still"]["ratio_chain_pixels"]), (q["still"], rec["still"])
    assert q["pan"]["ratio_chain_pixels"] <= bound(rec["pan"]["ratio_chain_pixels"]), (q["pan"], rec["pan"])
