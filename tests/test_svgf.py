"""Variance-guided spatiotemporal filtering (tyr_svgf, hip/svgf.hip; Renderer.svgf): tyr_temporal's reprojected running mean
extended to the luminance moments, a per-pixel variance from them, and an a-trous filter whose luminance term that variance
scales, with the first pass fed back as the next frame's history -- the per-frame recipe render_aov -> render_motion -> render
-> svgf.

CPU: the numpy restatement's own properties (tests/svgf_ref.py); what the compiler made of the kernels (make asm); the
committed measurement behind the quality bound.
GPU: bit for bit against the restatement on seeded inputs and on a rendered sequence; the resolve flag against tyr_resolve;
isolation from tyr_temporal / tyr_denoise and from the render state; arguments and streams; quality over a panning sequence
against temporal -> denoise."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

import denoise_ref
import svgf_ref as ref
import test_temporal
from conftest import ROOT, bits, built_scene
from kernel_resources import kernel_resources

VERY_FAR = ref.VERY_FAR
F = np.float32
# test_svgf_quality_on_a_panning_cornell_sequence: SVGF's MSE over temporal -> denoise's, both with their defaults, against a
# 1024-spp render (profiles/svgf_bench_c3.json "quality" "svgf_over_temporal_denoised", with the 1.2 margin of
# tests/test_temporal.py for the renders' float atomics)
QUALITY_BOUND = 1.0


def flat_inputs(W, H, u, depth=None, normal=None, A=1.0):
    """accum with rgb = u * A (albedo 1), unit normals (0, 0, 1) and depth 10 unless given; zero motion, prev_depth = depth"""
    n = W * H
    u = np.asarray(u, F).reshape(n, 3)
    accum = np.concatenate([(u * F(A)).astype(F), np.full((n, 1), A, F)], 1)
    albedo = np.ones((n, 3), F)
    normal = np.tile(np.array([0, 0, 1], F), (n, 1)) if normal is None else np.asarray(normal, F).reshape(n, 3)
    depth = np.full(n, 10.0, F) if depth is None else np.asarray(depth, F).reshape(n)
    return accum, albedo, normal, depth, np.zeros((n, 2), F), depth.copy()


def lum64(u):
    u = np.asarray(u, np.float64)
    return 0.2126 * u[..., 0] + 0.7152 * u[..., 1] + 0.0722 * u[..., 2]


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------
def test_restatement_variance_is_the_temporal_variance_of_the_moments():
    """zero motion, every tap accepted, K >= 4 frames within max_history: the variance is mean(l^2) - mean(l)^2 of the frames"""
    W, H, K = 8, 6, 6
    rng = np.random.default_rng(1)
    frames = rng.random((K, W * H, 3)).astype(F)
    hist = None
    for k in range(K):
        _, var, hist = ref.svgf(*flat_inputs(W, H, frames[k]), hist, W, H, max_history=16)
        assert np.all(hist.hu[:, 3] == k + 1)
    l = lum64(frames)
    want = (l * l).mean(0) - l.mean(0) ** 2
    assert want.min() > 1e-3
    assert np.allclose(var, want, rtol=1e-4, atol=2e-6), np.abs(var - want).max()


def test_restatement_of_a_constant_frame():
    """a constant frame: variance 0 on every call, and the output is the frame within 1 ulp, for 1, 5 and 8 passes"""
    W, H = 23, 17
    u = np.tile(np.array([0.5, 0.5, 0.5], F), (W * H, 1))
    for passes in (1, 5, 8):
        hist = None
        for k in range(5):
            out, var, hist = ref.svgf(*flat_inputs(W, H, u), hist, W, H, passes=passes)
            assert np.all(var == 0), (passes, k)
            ulp = np.spacing(u)
            assert np.all(np.abs(out[:, :3] - u) <= ulp), (passes, k)


def test_restatement_spatial_variance_on_the_first_frame():
    """frame 1 (n = 1): 4 x the 7 x 7 estimate weighted by the normal and depth terms (float64)"""
    W, H = 13, 11
    rng = np.random.default_rng(2)
    u = rng.random((W * H, 3)).astype(F)
    z = (F(10) + rng.random(W * H).astype(F) * F(0.3)).astype(F)
    v = np.tile(np.array([0, 0, 1], np.float64), (W * H, 1)) + rng.normal(scale=0.05, size=(W * H, 3))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    _, var, hist = ref.svgf(*flat_inputs(W, H, u, depth=z, normal=nrm), None, W, H)
    assert np.all(hist.hu[:, 3] == 1)
    kz = 1.0 / (0.02 * 0.02)
    l = lum64(u)
    n64, z64 = nrm.astype(np.float64), z.astype(np.float64)
    want = np.zeros(W * H)
    for p in range(W * H):
        y, x = divmod(p, W)
        s1 = s2 = ws = 0.0
        for qy in range(max(0, y - 3), min(H, y + 4)):
            for qx in range(max(0, x - 3), min(W, x + 4)):
                q = qy * W + qx
                if q == p:
                    w = 1.0
                else:
                    g = max(0.0, float(n64[p] @ n64[q])) ** 128
                    r = (z64[q] - z64[p]) / z64[p]
                    w = g / (1.0 + r * r * kz)
                s1, s2, ws = s1 + w * l[q], s2 + w * l[q] ** 2, ws + w
        want[p] = 4.0 * max(0.0, s2 / ws - (s1 / ws) ** 2)
    assert want.min() > 1e-3
    assert np.allclose(var, want, rtol=1e-3, atol=1e-5), np.abs(var - want).max()


def test_restatement_does_not_filter_across_a_depth_step():
    """left half at depth 1, right half at depth 1000: adding 1 to one side's colours moves the other side's output by at most
    1e-3 (relative) for 1, 5 and 8 passes, while at one depth it moves it by more than 10 %"""
    W, H = 24, 12
    rng = np.random.default_rng(3)
    y, x = np.divmod(np.arange(W * H), W)
    left = x < W // 2
    step = np.where(left, F(1.0), F(1000.0)).astype(F)
    flat = np.full(W * H, 1.0, F)
    a = rng.random((W * H, 3)).astype(F)
    for passes in (1, 5, 8):
        for side in (left, ~left):
            b = np.where(side[:, None], a, (a + F(1)).astype(F)).astype(F)
            moved = {}
            for name, z in (("step", step), ("flat", flat)):
                o = [ref.svgf(*flat_inputs(W, H, uu, depth=z), None, W, H, passes=passes)[0][:, :3].astype(np.float64) for uu in (a, b)]
                moved[name] = (np.abs(o[1] - o[0]) / np.abs(o[0]))[side].max()
            assert moved["step"] <= 1e-3 and moved["flat"] > 0.1, (passes, moved)


def test_restatement_feeds_back_the_first_pass():
    """the history's colour is pass 0's output whatever the pass count, so the next call does not depend on the later passes"""
    W, H = 16, 12
    rng = np.random.default_rng(4)
    f0, f1 = rng.random((2, W * H, 3)).astype(F)
    out1, _, h1 = ref.svgf(*flat_inputs(W, H, f0), None, W, H, passes=1)
    out5, _, h5 = ref.svgf(*flat_inputs(W, H, f0), None, W, H, passes=5)
    assert np.array_equal(bits(h1.hu), bits(h5.hu)) and np.array_equal(bits(h1.hm), bits(h5.hm))
    assert np.array_equal(bits(h5.hu[:, :3]), bits(out1[:, :3]))  # albedo 1: pass 0's output is the one-pass frame
    assert not np.array_equal(bits(out5[:, :3]), bits(out1[:, :3]))
    # the moments stay unfiltered: (l, l^2) of the frame
    l = ref.luminance(f0)
    assert np.array_equal(bits(h5.hm[:, 0]), bits(l)) and np.array_equal(bits(h5.hm[:, 1]), bits((l * l).astype(F)))
    a, _, _ = ref.svgf(*flat_inputs(W, H, f1), h1, W, H)
    b, _, _ = ref.svgf(*flat_inputs(W, H, f1), h5, W, H)
    assert np.array_equal(bits(a), bits(b))


# ---- CPU: resources of the kernels -------------------------------------------------------------------------------------
def test_svgf_kernels_keep_registers_in_budget():
    """k_svgf_reproject, k_svgf_variance and the three pass kernels: no spills, no scratch, no LDS, eight waves per SIMD"""
    res = kernel_resources("svgf")
    names = [n for n in res if "k_svgf_" in n]
    assert len(names) == 5, list(res)
    for n in names:
        k = res[n]
        assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
        assert k["ScratchSize [bytes/lane]"] == 0, (n, k)
        assert k["LDS Size [bytes/block]"] == 0, (n, k)
        assert k["Occupancy [waves/SIMD]"] >= 8, (n, k)


def svgf_profile():
    return json.load(open(os.path.join(ROOT, "profiles", "svgf_bench_c3.json")))


def test_svgf_bench_ratios_back_the_bounds():
    """the committed measurement holds the ratio the quality bound is taken from, measured with the defaults, and its grid"""
    q = svgf_profile()["quality"]
    d = q["defaults"]
    from tyrant_amd import binding

    assert (d["max_history"], d["passes"], d["sigma_luminance"], d["sigma_depth"], d["normal_power_log2"]) == (binding.SVGF_MAX_HISTORY, binding.SVGF_PASSES, binding.SVGF_SIGMA_LUMINANCE,
                                                                                                             binding.SVGF_SIGMA_DEPTH, binding.SVGF_NORMAL_POWER_LOG2)
    assert q["svgf_over_temporal_denoised"] * 1.2 <= QUALITY_BOUND
    assert {g["max_history"] for g in q["grid"]} >= {4, 8, 16}
    # the defaults are within 5 % of the grid's best
    assert q["svgf_mse"] <= min(g["svgf_mse"] for g in q["grid"]) * 1.05


# ---- GPU: bit for bit against the restatement --------------------------------------------------------------------------
def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def seeded_frame(W, H, rng, prev_z):
    """a random frame (tests/test_temporal.py's mix): background pixels, A == 0 pixels, albedo channels 0, depth near the
    previous frame's with some jumps, normals near (0, 0, 1) with some turned, motions integer, fractional, out of the frame and
    NaN, prev_depth VERY_FAR on some"""
    n = W * H
    A = rng.integers(1, 5, n).astype(F)
    A[rng.random(n) < 0.06] = 0
    rgb = (rng.random((n, 3)) * A[:, None] * rng.choice([0.3, 1.0, 4.0], (n, 1))).astype(F)
    accum = np.concatenate([rgb, A[:, None]], 1).astype(F)
    alb = rng.random((n, 3)).astype(F)
    alb[rng.random((n, 3)) < 0.08] = 0
    v = np.tile(np.array([0, 0, 1], np.float64), (n, 1)) + rng.normal(scale=0.05, size=(n, 3))
    turned = rng.random(n) < 0.05
    v[turned] = rng.normal(size=(int(turned.sum()), 3))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    z = (prev_z * (1 + rng.normal(scale=0.01, size=n))).astype(F)
    z[rng.random(n) < 0.05] *= F(1.5)
    bg = rng.random(n) < 0.08
    z[bg] = VERY_FAR
    alb[bg] = 0
    m = rng.uniform(-1.5, 1.5, (n, 2)).astype(F)
    integer = rng.random(n) < 0.2
    m[integer] = np.round(m[integer])
    m[rng.random(n) < 0.03] = F(1e6)
    m[rng.random(n) < 0.01] = F("nan")
    pdz = (prev_z * (1 + rng.normal(scale=0.01, size=n))).astype(F)
    pdz[rng.random(n) < 0.03] = VERY_FAR
    return accum, alb, nrm, z, m, pdz


def plane_depth(W, H):
    """a tilted plane 10 .. 13 units away: reprojected taps land on neighbours of about the same depth, so histories grow"""
    y, x = np.divmod(np.arange(W * H), W)
    return (F(10) + F(2) * (x / max(W, 1)).astype(F) + F(1) * (y / max(H, 1)).astype(F)).astype(F)


def gpu_svgf(g, ins, **kw):
    accum, alb, nrm, z, m, pdz = ins
    out, var = g.svgf(dev(alb), dev(nrm), dev(z), dev(m), dev(pdz), accum=dev(accum), want_variance=True, **kw)
    return out, var.cpu().numpy().reshape(-1)


def assert_bits(got, want, what):
    bad = bits(got) != bits(want)
    if bad.ndim > 1:
        bad = bad.any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first {np.flatnonzero(bad)[:5]}"


def tyr_resolve_of(hip, lin, W, H):
    """tyr_resolve of a linear frame (a device tensor) bound as a fresh ctx's blit buffer"""
    import torch

    torch.cuda.synchronize()
    r = hip.Renderer(W, H, 4096, blit_buffer=lin.data_ptr())
    want = torch.zeros_like(lin)
    torch.cuda.synchronize()  # the fill runs on torch's stream, tyr_resolve on the ctx's
    r.resolve_into(want.data_ptr())
    torch.cuda.synchronize()
    r.close()
    return want.cpu().numpy().reshape(-1, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(61, 37), (1, 29), (40, 1)])
def test_svgf_equals_the_restatement_on_seeded_inputs(hip, W, H):
    """nine calls with different parameters and a reset in the middle: output and variance bit for bit; a second ctx run
    with TYR_SVGF_RESOLVE on some calls gives tyr_resolve of the linear frame there and the same history everywhere"""
    rng = np.random.default_rng(100 * W + H)
    g = hip.Renderer(W, H, 4096)
    gr = hip.Renderer(W, H, 4096)
    settings = [{}, dict(passes=1), {}, dict(passes=8), dict(max_history=4), dict(reset=True), dict(passes=3, sigma_luminance=1.0),
                dict(max_history=1024, normal_cos=0.5, depth_tolerance=0.1, passes=8), {}]
    resolve_on = {1, 3, 8}
    z0 = plane_depth(W, H)
    hist = None
    short = long = 0
    for k, kw in enumerate(settings):
        ins = seeded_frame(W, H, rng, z0)
        rkw = {kk: v for kk, v in kw.items() if kk != "reset"}
        want, want_var, nxt = ref.svgf(*ins, None if kw.get("reset") else hist, W, H, **rkw)
        out, got_var = gpu_svgf(g, ins, **kw)
        got = out.cpu().numpy().reshape(-1, 4)
        assert_bits(got, want, f"{W}x{H} call {k} {kw}")
        assert_bits(got_var, want_var, f"{W}x{H} call {k} {kw} variance")
        tm, _ = gpu_svgf(gr, ins, resolve=k in resolve_on, **kw)
        tm = tm.cpu().numpy().reshape(-1, 4)
        seen = ins[0][:, 3] != 0
        if k in resolve_on:
            assert_bits(tm[seen], tyr_resolve_of(hip, out, W, H)[seen], f"{W}x{H} call {k} resolve")
            assert np.all(tm[~seen] == 0)
        else:
            assert_bits(tm, want, f"{W}x{H} call {k} after resolved calls")
        n = nxt.hu[:, 3]
        short += int(((n > 0) & (n < 4)).sum())
        long += int((n >= 4).sum())
        hist = nxt
    assert short > 0 and long > 0, (short, long)
    g.close()
    gr.close()


@pytest.mark.gpu
def test_svgf_equals_the_restatement_on_a_rendered_sequence(hip):
    """six frames of a moving camera through render_aov -> render_motion -> render -> svgf: every frame's output and variance
    bit for bit against the restatement fed the same device inputs"""
    sc, nodes, prims = built_scene("cornell36")
    sc = dataclasses.replace(sc, camera=hip.scenes.FRAMED_CAMERA)
    W, H = 96, 54
    g = hip.Renderer(W, H, 8192)
    g.load_scene(sc, nodes, prims)
    hist = None
    prev = None
    long = 0
    for k in range(6):
        cam = test_temporal.moved_camera(sc.camera, 0.1 * k)
        g.set_camera(cam)
        aov = g.render_aov(1)
        mot = g.render_motion(aov["prim"], aov["geom"], prev or cam)
        g.render(1)
        out, var = g.svgf(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], reset=(k == 0), want_variance=True)
        accum = g.blit_buffer()
        assert np.any(accum[:, 3] > 0)
        a, n, z = (aov[x].cpu().numpy() for x in ("albedo", "normal", "depth"))
        m, pd = mot["motion"].cpu().numpy(), mot["prev_depth"].cpu().numpy()
        want, want_var, hist = ref.svgf(accum, a, n, z, m, pd, None if k == 0 else hist, W, H)
        assert_bits(out.cpu().numpy().reshape(-1, 4), want, f"frame {k}")
        assert_bits(var.cpu().numpy().reshape(-1), want_var, f"frame {k} variance")
        long += int((hist.hu[:, 3] >= 4).sum())
        prev = cam
    assert long > W * H // 2, long
    g.close()


@pytest.mark.gpu
def test_svgf_is_isolated_from_temporal_and_denoise(hip):
    """tyr_temporal, tyr_denoise and tyr_svgf interleaved on one ctx give the bits of the same calls on three ctxs"""
    W, H = 64, 40
    rng = np.random.default_rng(9)
    z0 = plane_depth(W, H)
    frames = [[dev(a) for a in seeded_frame(W, H, rng, z0)] for _ in range(4)]
    one = hip.Renderer(W, H, 4096)
    sep = {k: hip.Renderer(W, H, 4096) for k in ("temporal", "denoise", "svgf")}

    def calls(ctx, which, f, k):
        accum, alb, nrm, z, m, pdz = f
        res = {}
        if which in ("temporal", None):
            res["temporal"] = ctx["temporal"].temporal(alb, nrm, z, m, pdz, accum=accum, reset=(k == 0))
        if which in ("svgf", None):
            res["svgf"] = ctx["svgf"].svgf(alb, nrm, z, m, pdz, accum=accum, reset=(k == 0))
        if which in ("denoise", None):
            res["denoise"] = ctx["denoise"].denoise(alb, nrm, z, accum=accum)
        return {kk: v.cpu().numpy() for kk, v in res.items()}

    for k, f in enumerate(frames):
        got = calls({x: one for x in sep}, None, f, k)
        for which in sep:
            want = calls(sep, which, f, k)[which]
            assert_bits(got[which].reshape(-1, 4), want.reshape(-1, 4), f"frame {k} {which}")
    one.close()
    for g in sep.values():
        g.close()


@pytest.mark.gpu
def test_svgf_leaves_the_render_state_alone(orc, hip):
    """mid-render, tyr_svgf changes no counter, frame, budget, accumulation or queue; the render then goes on to the oracle's
    result"""
    sc, nodes, prims = built_scene("cornell36")
    W, H, N = 96, 64, 8192
    g = hip.Renderer(W, H, N)
    g.load_scene(sc, nodes, prims)
    aov = g.render_aov(1)
    mot = g.render_motion(aov["prim"], aov["geom"], test_temporal.moved_camera(sc.camera))
    g.render(1, 2)  # mid-render: survivors in the queue
    before = (g.counters(), g.timings(), g.blit_buffer(), g.ray_queue(0), g.ray_queue(1))
    for resolve in (False, True):
        out = g.svgf(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], resolve=resolve)
    out.cpu()
    after = (g.counters(), g.timings(), g.blit_buffer(), g.ray_queue(0), g.ray_queue(1))
    assert before[0] == after[0] and before[1] == after[1]
    for x, y in zip(before[2:], after[2:]):
        assert x.tobytes() == y.tobytes()
    g.render(2)
    o = orc.Oracle(W, H, N)
    o.load_scene(sc, nodes, prims)
    o.render(1, 2)
    o.render(2)
    kg, ko = g.counters(), o.counters()
    for f in ("frame", "total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible", "budget_remaining"):
        assert kg[f] == ko[f], (f, kg[f], ko[f])
    bg, bo = g.blit_buffer(), o.blit_buffer()
    assert np.array_equal(bg[:, 3], bo[:, 3]) and np.allclose(bg[:, :3], bo[:, :3], rtol=1e-5, atol=1e-6)
    o.close()
    g.close()


@pytest.mark.gpu
def test_svgf_arguments_and_streams(hip):
    """every TYR_ERR_INVALID case; accum NULL reads the blit buffer; calls on two side streams after work on the caller's
    stream read its inputs and share the ctx's history in call order"""
    import torch

    W, H = 64, 48
    L = hip.lib()
    g = hip.Renderer(W, H, 4096)
    d0 = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    z0 = plane_depth(W, H)
    ins = seeded_frame(W, H, rng, z0)
    accum, alb, nrm, z, m, pdz = (dev(a) for a in ins)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device=d0)
    full = hip.SvgfIn(accum.data_ptr(), alb.data_ptr(), nrm.data_ptr(), z.data_ptr(), m.data_ptr(), pdz.data_ptr())

    def call(sin=full, prm=None, ctx=g.h, dst=out.data_ptr()):
        return L.tyr_svgf(ctx, None if sin is None else C.byref(sin), None if prm is None else C.byref(prm), dst, None, None)

    def Pm(mh=16, dt=0.05, nc=0.9, passes=5, sl=4.0, sd=0.02, npl=7, flags=0):
        return hip.SvgfParams(mh, dt, nc, passes, sl, sd, npl, flags)

    assert call() == 0 and call(prm=Pm(flags=hip.TYR_SVGF_RESET | hip.TYR_SVGF_RESOLVE)) == 0
    bad = [dict(sin=None), dict(ctx=None), dict(dst=None)]
    ptrs = [accum.data_ptr(), alb.data_ptr(), nrm.data_ptr(), z.data_ptr(), m.data_ptr(), pdz.data_ptr()]
    for j in range(1, 6):
        p = list(ptrs)
        p[j] = None
        bad.append(dict(sin=hip.SvgfIn(*p)))
    bad += [dict(prm=Pm(mh=0)), dict(prm=Pm(mh=1025)), dict(prm=Pm(flags=4)), dict(prm=Pm(passes=0)), dict(prm=Pm(passes=9)), dict(prm=Pm(npl=11))]
    bad += [dict(prm=Pm(dt=v)) for v in (0.0, -1.0, float("inf"), float("nan"))]
    bad += [dict(prm=Pm(nc=v)) for v in (-1.01, 1.01, float("nan"))]
    bad += [dict(prm=Pm(sl=v)) for v in (0.0, -1.0, float("inf"), float("nan"), 1e20)]
    bad += [dict(prm=Pm(sd=v)) for v in (0.0, -1.0, float("inf"), float("nan"), 1e-30)]
    for kw in bad:
        assert call(**kw) == hip.TYR_ERR_INVALID, kw
    assert call(prm=Pm(mh=1024, dt=1e30, nc=-1.0, passes=8, npl=10)) == 0 and call(prm=Pm(mh=1, nc=1.0, passes=1, npl=0)) == 0
    # accum NULL: the ctx's blit buffer (a ctx always has one, so TYR_ERR_NO_BUFFER cannot be reached from here)
    sc, nodes, prims = built_scene("cornell36")
    g.load_scene(sc, nodes, prims)
    g.render(1)
    o, var = g.svgf(alb, nrm, z, m, pdz, reset=True, want_variance=True)
    w, wv, _ = ref.svgf(g.blit_buffer(), *ins[1:], None, W, H)
    assert_bits(o.cpu().numpy().reshape(-1, 4), w, "accum NULL")
    assert_bits(var.cpu().numpy().reshape(-1), wv, "accum NULL variance")

    frames = [seeded_frame(W, H, rng, z0) for _ in range(4)]
    hist = None
    wants = []
    for k, f in enumerate(frames):
        w, wv, hist = ref.svgf(*f, None if k == 0 else hist, W, H)
        wants.append((w, wv))
    s1, s2 = torch.cuda.Stream(d0), torch.cuda.Stream(d0)
    got = []
    for k, f in enumerate(frames):
        busy = torch.randn(1 << 22, device=d0)
        for _ in range(8):
            busy = busy * 1.0001  # the caller's stream is busy ...
        t = [dev(a) + busy[:1] * 0 for a in f]  # ... and writes the inputs behind that work
        got.append(g.svgf(*t[1:], accum=t[0], reset=(k == 0), want_variance=True, stream=s1 if k % 2 == 0 else s2))
    torch.cuda.synchronize()
    for k, ((o, var), (w, wv)) in enumerate(zip(got, wants)):
        assert_bits(o.cpu().numpy().reshape(-1, 4), w, f"stream call {k}")
        assert_bits(var.cpu().numpy().reshape(-1), wv, f"stream call {k} variance")
    g.close()


# ---- GPU: quality ------------------------------------------------------------------------------------------------------
def mse(a, b):
    return float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())


@pytest.mark.gpu
def test_svgf_quality_on_a_panning_cornell_sequence(hip):
    """16 frames at 1 spp of the slowly panning framed Cornell view (tools/temporal_bench.py's sequence): against a 1024-spp
    render at the last camera, SVGF with its defaults has at most QUALITY_BOUND of the MSE of temporal -> denoise with theirs,
    computed here on the same frames"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    sc = dataclasses.replace(sc, camera=hip.scenes.FRAMED_CAMERA)
    Wq, Hq, frames = 128, 72, 16
    cams = [test_temporal.pan(sc.camera, k) for k in range(frames)]
    g = hip.Renderer(Wq, Hq, 1 << 16)
    g.load_scene(sc, nodes, prims)
    prev = cams[0]
    for k, cam in enumerate(cams):
        g.set_camera(cam)
        aov = g.render_aov(1)
        mot = g.render_motion(aov["prim"], aov["geom"], prev)
        g.render(1)
        acc = torch.from_numpy(g.blit_buffer()).to("cuda:0")
        gd = (aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"])
        sv = g.svgf(*gd, accum=acc, reset=(k == 0))
        tm = g.temporal(*gd, accum=acc, reset=(k == 0))
        prev = cam
    td = g.denoise(aov["albedo"], aov["normal"], aov["depth"], accum=tm)
    noisy = acc.cpu().numpy().reshape(-1, 4)
    g.close()
    r = hip.Renderer(Wq, Hq, 1 << 18)
    r.load_scene(sc, nodes, prims)
    r.set_camera(cams[-1])
    r.render(1024)
    conv = r.blit_buffer()
    r.close()
    seen = (noisy[:, 3] > 0) & (conv[:, 3] > 0)
    want = conv[seen, :3].astype(np.float64) / conv[seen, 3:]
    m_svgf = mse(sv.cpu().numpy().reshape(-1, 4)[seen, :3], want)
    m_td = mse(td.cpu().numpy().reshape(-1, 4)[seen, :3], want)
    assert m_svgf <= QUALITY_BOUND * m_td, (m_svgf, m_td, m_svgf / m_td)
