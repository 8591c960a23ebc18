"""Temporal anti-aliasing of the resolved frame (tyr_taa, hip/taa.hip; Renderer.taa): the frame behind the tone map is blended
into the ctx's reprojected history of its own outputs, sampled with the motion of the nearest surface of the 3 x 3
neighbourhood (Catmull-Rom, or tyr_temporal's bilinear taps) and clamped to the neighbourhood's YCoCg box -- the last stage of
the per-frame recipe render_aov -> render_motion -> render -> svgf(resolve) -> taa.

CPU: the numpy restatement's own properties (tests/taa_ref.py); that the seeded inputs of the GPU tests reach every path;
what the compiler made of the kernel (make asm); the committed measurement behind the quality bounds; the ABI.
GPU: bit for bit against the restatement on seeded inputs and on a rendered sequence; isolation from the other filters and
from the render state; arguments, streams and devices; flicker and error over a panning and a still sequence; the C++ example
of the whole recipe."""
import ctypes as C
import dataclasses
import json
import os
import re
import subprocess

import numpy as np
import pytest

import taa_ref as ref
import test_svgf
import test_temporal
from conftest import ROOT, bits, built_scene
from test_svgf import assert_bits, dev, kernel_resources, plane_depth

CSRC = os.path.join(ROOT, "tyrant_amd", "csrc")
VERY_FAR = ref.VERY_FAR
F = np.float32
SIZES = [(61, 37), (1, 29), (40, 1)]
# the margin tests/test_temporal.py gives to the renders' float atomics, on the ratios profiles/taa_bench_c3.json holds
ATOMICS_MARGIN = 1.2
TAIL = 8  # the quality figures are taken over the last 8 of 16 frames


def still_inputs(W, H, rgb, depth=10.0):
    """a seen frame of the given colours at one depth: zero motion, prev_depth = depth"""
    n = W * H
    color = np.concatenate([np.asarray(rgb, F).reshape(n, 3), np.ones((n, 1), F)], 1)
    z = np.full(n, depth, F)
    return color, z, np.zeros((n, 2), F), z.copy()


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------
def test_restatement_returns_a_constant_frame():
    """a constant frame comes back bit for bit on every call, both samplers, several gammas, at sizes with every kind of
    border.  The colours are dyadic, so that their YCoCg transform and its inverse are exact: the contract blends in YCoCg,
    and for a colour whose transform rounds the fixed point is the transform's round trip of it -- still reached at the second
    call and kept bit for bit from then on, within 2 ulp of the colour (the last loop)."""
    for W, H in [(9, 7), (1, 6), (5, 1), (1, 1)]:
        for rgb in ((0.5, 0.5, 0.5), (0.5, 0.25, 0.75), (1.0, 0.0, 0.125)):
            for kw in ({}, dict(bilinear=True), dict(gamma=0.0), dict(gamma=4.0, alpha=1.0)):
                ins = still_inputs(W, H, np.tile(np.array(rgb, F), (W * H, 1)))
                hist = None
                for k in range(5):
                    out, hist = ref.taa(*ins, hist, W, H, **kw)
                    assert_bits(out, ins[0], f"{W}x{H} {rgb} {kw} call {k}")
    W, H = 9, 7
    rng = np.random.default_rng(11)
    for _ in range(8):
        rgb = rng.random(3).astype(F)
        ins = still_inputs(W, H, np.tile(rgb, (W * H, 1)))
        hist = None
        outs = []
        for k in range(5):
            out, hist = ref.taa(*ins, hist, W, H)
            outs.append(out)
        for k in range(2, 5):
            assert_bits(outs[k], outs[1], f"{rgb} call {k}")
        assert np.all(np.abs(outs[1][:, :3] - rgb) <= 2 * np.spacing(np.maximum(rgb, F(0.25))))


def anchored_frames(W, H, K, rng):
    """K frames whose history can never leave the neighbourhood box: on a checkerboard, every other pixel is an anchor that
    never changes -- (1, 1, 0), the largest Y, Co and Cg, in odd columns and (0, 0, 1), the smallest, in even ones (dyadic:
    their transform is exact) -- so every free pixel has both kinds among its horizontal and vertical neighbours, at the
    borders too; the free pixels hold fresh random colours in [0.4, 0.6] every frame, well inside the anchors' box"""
    y, x = np.divmod(np.arange(W * H), W)
    anchor = (x + y) % 2 == 1
    frames = (F(0.4) + F(0.2) * rng.random((K, W * H, 3)).astype(F)).astype(F)
    frames[:, anchor & (x % 2 == 1)] = np.array([1, 1, 0], F)
    frames[:, anchor & (x % 2 == 0)] = np.array([0, 0, 1], F)
    return frames, anchor


def test_restatement_is_the_exponential_mean_of_a_still_camera():
    """still camera, zero motion, a gamma so large that the box is [mn, mx], and frames whose history stays inside it
    (anchored_frames; the restatement's clamp counts are asserted to be 0): after K frames the output is
    sum_{j < K-1} alpha (1 - alpha)^j c_{K-j} + (1 - alpha)^(K-1) c_1 (the first frame is taken whole), the transform being
    linear.  Tolerance: a call rounds at most R = 12 times per channel on values of magnitude <= 1 (three operations for each
    of the two forward transforms, the subtraction, the product and the sum of the blend, two operations of the inverse,
    and one for the Catmull-Rom sum, whose other terms are zeros), each by at most 2^-24; an earlier call's error is scaled
    by (1 - alpha) < 1 by each later one, so after K calls the error is below K * R * 2^-24."""
    W, H, K = 12, 10, 12
    for alpha in (0.1, 0.4):
        for bilinear in (False, True):
            frames, anchor = anchored_frames(W, H, K, np.random.default_rng(21))
            hist = None
            for k in range(K):
                info = {}
                out, hist = ref.taa(*still_inputs(W, H, frames[k]), hist, W, H, alpha=alpha, gamma=1e6, bilinear=bilinear, info=info)
                assert info["clamp_lo"].sum() == 0 and info["clamp_hi"].sum() == 0, k
                assert info["no_history"].sum() == (W * H if k == 0 else 0)
            a = float(F(alpha))
            want = (1 - a) ** (K - 1) * frames[0].astype(np.float64)
            for j in range(K - 1):
                want += a * (1 - a) ** j * frames[K - 1 - j].astype(np.float64)
            err = np.abs(out[:, :3].astype(np.float64) - want)
            assert err.max() <= K * 12 * 2.0 ** -24, (alpha, bilinear, err.max())
            assert_bits(out[anchor], np.concatenate([frames[0], np.ones((W * H, 1), F)], 1)[anchor], "anchors")
            assert np.abs(out[~anchor, :3].astype(np.float64) - frames[K - 1][~anchor]).max() > 1e-3  # it is a mean, not the last frame


def test_restatement_clamps_a_far_history_into_the_neighbourhood():
    """a history far above, or far below, every colour of a neighbourhood lands inside [mn, mx] of that neighbourhood in every
    YCoCg channel, whatever gamma, and the output stays between it and the current colour"""
    W, H = 17, 13
    rng = np.random.default_rng(31)
    cur = (F(0.2) + F(0.6) * rng.random((W * H, 3)).astype(F)).astype(F)
    # (Co and Cg are differences: a history is far outside their boxes on both sides only with unequal channels)
    for far in ((40.0, 40.0, 40.0), (-40.0, -40.0, -40.0), (40.0, 0.0, -40.0), (-40.0, 40.0, -40.0), (0.0, -40.0, 40.0)):
        for gamma in (0.0, 1.0, 100.0):
            for bilinear in (False, True):
                _, hist = ref.taa(*still_inputs(W, H, np.tile(np.array(far, F), (W * H, 1))), None, W, H)
                info = {}
                out, _ = ref.taa(*still_inputs(W, H, cur), hist, W, H, alpha=0.1, gamma=gamma, bilinear=bilinear, info=info)
                assert info["no_history"].sum() == 0
                hc, mn, mx = info["clamped"], info["mn"], info["mx"]
                assert np.all((hc >= mn) & (hc <= mx)), (far, gamma)
                assert np.all(info["lo"] >= mn) and np.all(info["hi"] <= mx) and np.all(info["lo"] <= info["hi"])
                moved = info["clamp_lo"] | info["clamp_hi"]
                assert moved.any(axis=1).all(), (far, gamma)
                ck = ref.ycocg(cur)
                ok = ref.ycocg(out[:, :3])
                tol = 4 * np.spacing(F(1))
                assert np.all(ok >= np.minimum(hc, ck) - tol) and np.all(ok <= np.maximum(hc, ck) + tol)


def test_restatement_follows_an_integer_translation():
    """a pattern translated by whole pixels per frame, with the matching integer motion and alpha -> 0+ (2^-60: the blend's
    product is below half an ulp of the history) and a gamma that leaves the box at [mn, mx] (at gamma 1 a pixel's own colour
    can lie outside mean +- sd of its neighbourhood), follows the motion exactly: at integer positions Catmull-Rom's weights are
    (-0, 1, 0, -0) and the bilinear ones (1, 0, 0, 0), so every output is the pattern's pixel bit for bit (the pattern is
    dyadic, so its YCoCg round trip is exact) -- where the history came from inside the frame through either sampler, and
    where it came from outside through "no history".  With the motion left out the same frames do not come out."""
    W, H, K = 24, 18, 5
    rng = np.random.default_rng(41)
    for d in ((1, 0), (-2, 1), (3, -2)):
        canvas = (rng.integers(0, 65, (H + 40, W + 40, 3)) / 64.0).astype(F)
        frame = lambda k: canvas[20 - k * d[1]:20 - k * d[1] + H, 20 - k * d[0]:20 - k * d[0] + W].reshape(-1, 3)  # noqa: E731
        motion = np.tile(np.array([-d[0], -d[1]], F), (W * H, 1))
        for bilinear in (False, True):
            hist = hist0 = None
            took = 0
            for k in range(K):
                color, z, _, pz = still_inputs(W, H, frame(k))
                info = {}
                out, hist = ref.taa(color, z, motion, pz, hist, W, H, alpha=2.0 ** -60, gamma=1e6, bilinear=bilinear, info=info)
                assert_bits(out, color, f"{d} frame {k}")
                took += int(info["bilinear" if bilinear else "catmull_rom"].sum())
                if k:
                    y, x = np.divmod(np.arange(W * H), W)
                    inner = (x - d[0] >= 1) & (x - d[0] + 2 < W) & (y - d[1] >= 1) & (y - d[1] + 2 < H)
                    assert np.all(info["bilinear" if bilinear else "catmull_rom"][inner])
                out0, hist0 = ref.taa(color, z, np.zeros_like(motion), pz, hist0, W, H, alpha=2.0 ** -60, gamma=1e6, bilinear=bilinear)
                if k:
                    assert (bits(out0) != bits(color)).any(axis=1).mean() > 0.5
            assert took > (K - 1) * W * H // 2


def test_restatement_dilates_the_motion_at_a_depth_step():
    """a moving foreground (depth 5, motion (2, 0)) left of x = 8, a still wall (depth 50) and then the background (VERY_FAR)
    behind it: the wall's and the background's pixels next to the foreground take the foreground's motion, every other pixel
    its own; a background pixel among background pixels has zero motion and a history"""
    W, H = 16, 9
    n = W * H
    y, x = np.divmod(np.arange(n), W)
    rng = np.random.default_rng(51)
    color = np.concatenate([rng.random((n, 3)).astype(F), np.ones((n, 1), F)], 1)
    fg = x < 8
    wall = ~fg & (y < 5)
    z = np.where(fg, F(5), np.where(wall, F(50), VERY_FAR)).astype(F)
    motion = np.where(fg[:, None], np.array([2, 0], F), np.array([0, 0], F)).astype(F)
    motion[~fg & (y >= 6)] = np.array([7, 7], F)  # never read where every tap is background: the background does not move
    pz = np.where(z < VERY_FAR, z, VERY_FAR).astype(F)
    _, hist = ref.taa(color, z, motion, pz, None, W, H)
    info = {}
    ref.taa(color, z, motion, pz, hist, W, H, info=info)
    edge = x == 8
    assert np.all(info["m"][edge] == np.array([2, 0], F)) and np.all(z[info["taken"][edge]] == 5)
    assert np.all(info["dilated"][edge]) and not info["dilated"][~edge].any()
    rest = ~fg & ~edge
    assert np.all(info["m"][rest] == 0)
    deep = rest & ~wall & (y >= 6)  # every tap is background
    assert deep.any() and np.all(info["background"][deep]) and not info["background"][fg | wall].any()
    assert not info["no_history"].any()


def test_restatement_bilinear_flag_equals_the_fallback():
    """where the default call falls back from the 16 taps to the bilinear ones, TYR_TAA_BILINEAR gives the same bits"""
    hit = 0
    for W, H in SIZES:
        rng = np.random.default_rng(7 * W + H)
        z0 = plane_depth(W, H)
        _, hist = ref.taa(*seeded_frame(W, H, rng, z0), None, W, H)
        for k in range(3):
            ins = seeded_frame(W, H, rng, z0)
            info = {}
            a, nxt = ref.taa(*ins, hist, W, H, info=info)
            b, _ = ref.taa(*ins, hist, W, H, bilinear=True)
            fb = info["bilinear"]
            assert_bits(a[fb], b[fb], f"{W}x{H} call {k}")
            hit += int(fb.sum())
            if W >= 4 and H >= 4:
                cr = info["catmull_rom"]
                assert cr.any() and (bits(a[cr]) != bits(b[cr])).any()
            hist = nxt
    assert hit > 100


def test_restatement_has_no_history_where_it_cannot_be_found():
    """a NaN, huge or infinite motion, prev_depth VERY_FAR on a surface: the pixel -- and every neighbour that takes its
    motion, for it is the nearest -- has no history and outputs its own colour.  An unseen pixel outputs zeros whatever
    its rgb holds and is no tap of anything.  No NaN reaches any output."""
    W, H = 30, 20
    n = W * H
    y, x = np.divmod(np.arange(n), W)
    rng = np.random.default_rng(61)
    base = np.concatenate([rng.random((n, 3)).astype(F), np.ones((n, 1), F)], 1)
    _, hist = ref.taa(*still_inputs(W, H, base[:, :3]), None, W, H)
    color = np.concatenate([rng.random((n, 3)).astype(F), np.ones((n, 1), F)], 1)
    z = np.full(n, 10.0, F)
    motion = np.zeros((n, 2), F)
    pz = z.copy()
    special = {}
    for j, kind in enumerate(("nan", "huge", "inf", "prev_far", "unseen")):
        p = 5 * W + 3 + 5 * j
        special[kind] = p
        z[p] = 1.0  # the nearest of its neighbourhood
    motion[special["nan"]] = F("nan")
    motion[special["huge"]] = F(1e6)
    motion[special["inf"], 1] = F("inf")
    pz[special["prev_far"]] = VERY_FAR
    color[special["unseen"]] = np.array([np.nan, np.nan, np.nan, 0], F)
    info = {}
    out, nxt = ref.taa(color, z, motion, pz, hist, W, H, info=info)
    assert np.isfinite(out).all() and np.isfinite(nxt.h).all()
    for kind in ("nan", "huge", "inf", "prev_far"):
        p = special[kind]
        around = (np.abs(x - x[p]) <= 1) & (np.abs(y - y[p]) <= 1)
        assert np.all(info["no_history"][around]), kind
        assert_bits(out[around], color[around], kind)
    p = special["unseen"]
    assert np.all(out[p] == 0) and np.all(nxt.h[p] == 0)
    around = (np.abs(x - x[p]) <= 1) & (np.abs(y - y[p]) <= 1) & (np.arange(n) != p)
    assert not info["no_history"][around].any() and np.all(info["taken"][around] != p)
    far = np.ones(n, bool)
    for p in special.values():
        far &= ~((np.abs(x - x[p]) <= 1) & (np.abs(y - y[p]) <= 1))
    assert not info["no_history"][far].any()
    # the next call: the unseen pixel's history is invalid, so the 16 taps around it fall back and skip it
    info = {}
    out2, _ = ref.taa(*still_inputs(W, H, base[:, :3]), nxt, W, H, info=info)
    assert np.isfinite(out2).all()
    p = special["unseen"]
    near = (x - x[p] >= -2) & (x - x[p] <= 1) & (y - y[p] >= -2) & (y - y[p] <= 1)
    assert not info["catmull_rom"][near].any() and info["bilinear"][near & (np.arange(n) != p)].all() and info["no_history"][p]


# ---- CPU: the seeded inputs of the GPU tests reach every path ------------------------------------------------------------
def seeded_frame(W, H, rng, prev_z):
    """tests/test_svgf.py's seeded_frame (depths near the previous frame's with some jumps, background pixels, A == 0 pixels,
    motions integer, fractional, out of the frame and NaN, prev_depth VERY_FAR on some) turned into tyr_taa's inputs:
    resolved-looking colours in [0, 1] around a smooth picture, alpha 1 where the frame was seen and (0, 0, 0, 0) elsewhere,
    and a block of background pixels, so that some neighbourhoods hold nothing else"""
    accum, _, _, z, m, pdz = test_svgf.seeded_frame(W, H, rng, prev_z)
    n = W * H
    y, x = np.divmod(np.arange(n), W)
    smooth = np.stack([0.5 + 0.4 * np.sin(0.3 * x + 0.1 * y), 0.5 + 0.4 * np.cos(0.2 * y), 0.5 + 0.3 * np.sin(0.15 * (x + y))], 1)
    rgb = np.clip(smooth + rng.normal(scale=rng.choice([0.02, 0.2]), size=(n, 3)), 0, 1).astype(F)
    seen = accum[:, 3] != 0
    color = np.concatenate([rgb, np.ones((n, 1), F)], 1)
    color[~seen] = 0
    block = (x >= W // 2) & (x < W // 2 + 6) & (y >= H // 3) & (y < H // 3 + 6)
    z = z.copy()
    z[block] = VERY_FAR
    return color, z, m, pdz


SETTINGS = [{}, dict(alpha=0.3), dict(bilinear=True), dict(gamma=0.0), dict(alpha=1.0, gamma=3.0), dict(reset=True), dict(in_place=True), dict(alpha=0.05, gamma=1.5, bilinear=True),
            dict(gamma=100.0), {}]
COVERED = ("catmull_rom", "bilinear", "no_history", "clamp_lo", "clamp_hi", "unclamped", "dilated", "background")


def seeded_calls(W, H):
    """the calls of test_taa_equals_the_restatement_on_seeded_inputs: (inputs, keywords, expected output, masks) per call"""
    rng = np.random.default_rng(100 * W + H)
    z0 = plane_depth(W, H)
    hist = None
    calls = []
    for kw in SETTINGS:
        ins = seeded_frame(W, H, rng, z0)
        rkw = {k: v for k, v in kw.items() if k not in ("reset", "in_place")}
        info = {}
        want, hist = ref.taa(*ins, None if kw.get("reset") else hist, W, H, info=info, **rkw)
        calls.append((ins, kw, want, info))
    return calls


@pytest.mark.parametrize("W,H", SIZES)
def test_seeded_inputs_reach_every_path(W, H):
    """counted from the restatement alone: over the seeded calls of each size, a non-zero number of pixels takes the
    Catmull-Rom kernel (where the frame is wide enough for one), the bilinear fallback and no history, is clamped from below,
    from above and not at all, takes a neighbour's motion instead of its own, and is background with zero motion"""
    count = dict.fromkeys(COVERED, 0)
    for _, kw, _, info in seeded_calls(W, H):
        if kw.get("bilinear"):
            assert not info["catmull_rom"].any()
        for k in COVERED:
            count[k] += int(info[k].sum())
    for k in COVERED:
        if k == "catmull_rom" and (W < 4 or H < 4):
            assert count[k] == 0
        else:
            assert count[k] > 0, (k, count)


# ---- CPU: resources of the kernel, the committed measurement, the ABI ---------------------------------------------------
def test_taa_kernel_keeps_registers_in_budget():
    """k_taa: no spills, no scratch, no LDS (the taps go through L1 / L2: DESIGN.md "Temporal anti-aliasing"), eight waves
    per SIMD"""
    res = kernel_resources("taa")
    names = [n for n in res if "k_taa" in n]
    assert len(names) == 1, list(res)
    for n in names:
        k = res[n]
        assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
        assert k["ScratchSize [bytes/lane]"] == 0, (n, k)
        assert k["LDS Size [bytes/block]"] == 0, (n, k)
        assert k["Occupancy [waves/SIMD]"] >= 8, (n, k)


def taa_profile():
    return json.load(open(os.path.join(ROOT, "profiles", "taa_bench_c3.json")))


def quality_bounds():
    """what test_taa_quality_on_a_panning_and_a_still_sequence bounds, from the committed ratios"""
    q = taa_profile()["quality"]
    return {"panning_flicker": q["panning"]["flicker_ratio"] * ATOMICS_MARGIN, "panning_mse": q["panning"]["mse_ratio"] * ATOMICS_MARGIN, "still_mse": 1.0}


def test_taa_bench_ratios_back_the_bounds():
    """the committed measurement was made with the shipped defaults, these are the grid point its selection rule picks (the
    lowest panning flicker among the points whose panning MSE is within 5 % of the grid's best), TAA lowers the flicker of
    the panning sequence and the error of the still one, and the time is reported next to tyr_temporal's and tyr_svgf's"""
    from tyrant_amd import binding

    p = taa_profile()
    q = p["quality"]
    assert q["defaults"] == {"alpha": binding.TAA_ALPHA, "gamma": binding.TAA_GAMMA, "bilinear": False}
    grid = q["grid"]
    assert {(g["alpha"], g["gamma"], g["bilinear"]) for g in grid} == {(a, gm, b) for a in (0.05, 0.1, 0.2, 0.4) for gm in (0.75, 1.0, 1.25, 1.5) for b in (False, True)}
    best = min(g["panning"]["taa_mse"] for g in grid)
    sel = min((g for g in grid if g["panning"]["taa_mse"] <= 1.05 * best), key=lambda g: g["panning"]["taa_flicker"])
    assert (sel["alpha"], sel["gamma"], sel["bilinear"]) == (binding.TAA_ALPHA, binding.TAA_GAMMA, False), sel
    at = next(g for g in grid if (g["alpha"], g["gamma"], g["bilinear"]) == (binding.TAA_ALPHA, binding.TAA_GAMMA, False))
    for seq in ("panning", "still"):
        assert q[seq] == at[seq]
        for k in ("mse_ratio", "flicker_ratio"):
            assert np.isclose(q[seq][k], q[seq]["taa_" + k[:-6]] / q["svgf"][seq][k[:-6]], rtol=1e-12)
    assert q["panning"]["flicker_ratio"] < 1.0
    assert q["still"]["mse_ratio"] < 1.0
    b = quality_bounds()
    assert b["panning_flicker"] == q["panning"]["flicker_ratio"] * 1.2 and b["panning_mse"] == q["panning"]["mse_ratio"] * 1.2
    t = p["timing"]
    for k in ("taa", "taa_bilinear", "temporal", "svgf"):
        assert t[k]["n"] == 200 and t[k]["p10_ms"] <= t[k]["median_ms"] <= t[k]["p90_ms"]


def test_taa_is_declared_and_exported():
    """include/tyr_c.h declares tyr_taa, its records and flags; the built library exports it; the ABI version stays 5"""
    from tyrant_amd import binding

    h = open(os.path.join(ROOT, "include", "tyr_c.h")).read()
    assert re.search(r"^int tyr_taa\(tyr_ctx\* ctx, const tyr_taa_in\* in, const tyr_taa_params\* params, void\* device_rgba_out, void\* stream\);", h, re.M)
    assert re.search(r"#define TYR_TAA_RESET 1u", h) and re.search(r"#define TYR_TAA_BILINEAR 2u", h) and re.search(r"#define TYR_ABI_VERSION 5 ", h)
    assert "} tyr_taa_in;" in h and "} tyr_taa_params;" in h
    L = binding.lib()
    assert L.tyr_taa is not None and L.tyr_abi_version() == 5
    assert (binding.TYR_TAA_RESET, binding.TYR_TAA_BILINEAR) == (1, 2)
    assert C.sizeof(binding.TaaIn) == 4 * C.sizeof(C.c_void_p) and C.sizeof(binding.TaaParams) == 12


# ---- GPU: bit for bit against the restatement --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_taa_equals_the_restatement_on_seeded_inputs(hip, W, H):
    """ten calls with different alpha and gamma, both samplers, a reset in the middle and one call in place: every pixel's
    four floats equal the restatement's, the history carried from call to call"""
    g = hip.Renderer(W, H, 4096)
    for k, (ins, kw, want, _) in enumerate(seeded_calls(W, H)):
        color, z, m, pdz = (dev(a) for a in ins)
        gkw = {kk: v for kk, v in kw.items() if kk != "in_place"}
        out = g.taa(color, z, m, pdz, out=color if kw.get("in_place") else None, **gkw)
        if kw.get("in_place"):
            assert out.data_ptr() == color.data_ptr()
        assert_bits(out.cpu().numpy().reshape(-1, 4), want, f"{W}x{H} call {k} {kw}")
    g.close()


def recipe_frame(g, cam, prev, first, spp=1):
    """one frame of the recipe up to svgf(resolve=True): (resolved frame, depth, motion, prev_depth, seen)"""
    g.set_camera(cam)
    g.reset_accum()
    aov = g.render_aov(1)
    mot = g.render_motion(aov["prim"], aov["geom"], prev or cam)
    g.render(spp)
    acc = g.blit_buffer()
    # (a copy of the accumulation: the filter runs on torch's stream, and the next frame's reset_accum on the ctx's would
    # otherwise clear the buffer under it)
    sv = g.svgf(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], accum=dev(acc), reset=first, resolve=True)
    return sv, aov["depth"], mot["motion"], mot["prev_depth"], acc[:, 3] > 0


@pytest.mark.gpu
def test_taa_equals_the_restatement_on_a_rendered_sequence(hip):
    """six frames of a moving camera through render_aov -> render_motion -> render -> svgf(resolve) -> taa: every frame bit
    for bit against the restatement fed the same device inputs; most pixels find their history through the Catmull-Rom kernel"""
    sc, nodes, prims = built_scene("cornell36")
    sc = dataclasses.replace(sc, camera=hip.scenes.FRAMED_CAMERA)
    W, H = 96, 54
    g = hip.Renderer(W, H, 8192)
    g.load_scene(sc, nodes, prims)
    hist = prev = None
    cr = 0
    for k in range(6):
        cam = test_temporal.moved_camera(sc.camera, 0.1 * k)
        sv, z, m, pd, _ = recipe_frame(g, cam, prev, k == 0)
        out = g.taa(sv, z, m, pd, reset=(k == 0))
        info = {}
        want, hist = ref.taa(sv.cpu().numpy(), z.cpu().numpy(), m.cpu().numpy(), pd.cpu().numpy(), None if k == 0 else hist, W, H, info=info)
        assert_bits(out.cpu().numpy().reshape(-1, 4), want, f"frame {k}")
        cr += int(info["catmull_rom"].sum())
        prev = cam
    assert cr > 5 * W * H // 2, cr
    g.close()


# ---- GPU: isolation ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_taa_is_isolated_from_the_other_filters(hip):
    """tyr_taa interleaved with tyr_temporal, tyr_denoise and tyr_svgf on one ctx gives the bits of the same calls on
    separate ctxs, and leaves theirs alone"""
    W, H = 64, 40
    rng = np.random.default_rng(9)
    z0 = plane_depth(W, H)
    names = ("taa", "temporal", "denoise", "svgf")
    one = hip.Renderer(W, H, 4096)
    sep = {k: hip.Renderer(W, H, 4096) for k in names}

    def calls(ctx, which, f, t, k):
        accum, alb, nrm, z, m, pdz = f
        res = {}
        if which in ("temporal", None):
            res["temporal"] = ctx["temporal"].temporal(alb, nrm, z, m, pdz, accum=accum, reset=(k == 0))
        if which in ("taa", None):
            res["taa"] = ctx["taa"].taa(*t, reset=(k == 0))
        if which in ("svgf", None):
            res["svgf"] = ctx["svgf"].svgf(alb, nrm, z, m, pdz, accum=accum, reset=(k == 0))
        if which in ("denoise", None):
            res["denoise"] = ctx["denoise"].denoise(alb, nrm, z, accum=accum)
        return {kk: v.cpu().numpy() for kk, v in res.items()}

    for k in range(4):
        f = [dev(a) for a in test_svgf.seeded_frame(W, H, rng, z0)]
        t = [dev(a) for a in seeded_frame(W, H, rng, z0)]
        got = calls({x: one for x in names}, None, f, t, k)
        for which in names:
            want = calls(sep, which, f, t, k)[which]
            assert_bits(got[which].reshape(-1, 4), want.reshape(-1, 4), f"frame {k} {which}")
    one.close()
    for g in sep.values():
        g.close()


@pytest.mark.gpu
def test_taa_leaves_the_render_state_alone(orc, hip):
    """mid-render, tyr_taa changes no counter, timing, accumulation or queue; the render then goes on to the oracle's counters"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    W, H, N = 96, 64, 8192
    g = hip.Renderer(W, H, N)
    g.load_scene(sc, nodes, prims)
    aov = g.render_aov(1)
    mot = g.render_motion(aov["prim"], aov["geom"], test_temporal.moved_camera(sc.camera))
    g.render(1, 2)  # mid-render: survivors in the queue
    color = torch.rand((H, W, 4), dtype=torch.float32, device="cuda:0")
    before = (g.counters(), g.timings(), g.blit_buffer(), g.ray_queue(0), g.ray_queue(1))
    for kw in ({}, dict(bilinear=True), dict(reset=True)):
        out = g.taa(color, aov["depth"], mot["motion"], mot["prev_depth"], **kw)
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


# ---- GPU: arguments, streams, devices ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_taa_arguments_streams_and_devices(hip):
    """every TYR_ERR_INVALID case; a call on a caller's stream behind work that writes its inputs is ordered with the next call
    on the ctx's stream (they share the history); the caller's current device comes back"""
    import torch

    W, H = 64, 48
    L = hip.lib()
    g = hip.Renderer(W, H, 4096)
    d0 = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    z0 = plane_depth(W, H)
    color, z, m, pdz = (dev(a) for a in seeded_frame(W, H, rng, z0))
    out = torch.zeros((H, W, 4), dtype=torch.float32, device=d0)
    ptrs = [color.data_ptr(), z.data_ptr(), m.data_ptr(), pdz.data_ptr()]
    full = hip.TaaIn(*ptrs)

    def call(tin=full, prm=None, ctx=g.h, dst=out.data_ptr()):
        return L.tyr_taa(ctx, None if tin is None else C.byref(tin), None if prm is None else C.byref(prm), dst, None)

    Pm = lambda alpha=0.1, gamma=1.0, flags=0: hip.TaaParams(alpha, gamma, flags)  # noqa: E731
    assert call() == 0 and call(prm=Pm(flags=hip.TYR_TAA_RESET | hip.TYR_TAA_BILINEAR)) == 0
    bad = [dict(tin=None), dict(ctx=None), dict(dst=None)]
    for j in range(4):
        p = list(ptrs)
        p[j] = None
        bad.append(dict(tin=hip.TaaIn(*p)))
    bad += [dict(prm=Pm(alpha=v)) for v in (0.0, -0.5, 1.0001, float("inf"), float("nan"))]
    bad += [dict(prm=Pm(gamma=v)) for v in (-1e-3, float("inf"), float("nan"))]
    bad += [dict(prm=Pm(flags=v)) for v in (4, 8 | 1, 0x80000000)]
    for kw in bad:
        assert call(**kw) == hip.TYR_ERR_INVALID, kw
    assert call(prm=Pm(alpha=1.0, gamma=0.0)) == 0 and call(prm=Pm(alpha=1e-30, gamma=1e30)) == 0
    torch.cuda.synchronize()

    frames = [seeded_frame(W, H, rng, z0) for _ in range(4)]
    hist = None
    wants = []
    for k, f in enumerate(frames):
        w, hist = ref.taa(*f, None if k == 0 else hist, W, H)
        wants.append(w)
    side = torch.cuda.Stream(d0)
    got = []
    for k, f in enumerate(frames):
        if k % 2 == 0:  # on the caller's stream, behind the work that writes the inputs there ...
            with torch.cuda.stream(side):
                busy = torch.randn(1 << 22, device=d0)
                for _ in range(8):
                    busy = busy * 1.0001
                t = [dev(a) + busy[:1] * 0 for a in f]
            got.append(g.taa(*t, reset=(k == 0), stream=side))
            for x in t:
                x.record_stream(side)
        else:  # ... and straight behind it on the ctx's own stream (handle NULL), which must wait for that call's history
            t = [dev(a) for a in f]
            torch.cuda.current_stream(d0).synchronize()  # the ctx's stream is not torch's: the inputs are there before the call
            o = torch.empty((H, W, 4), dtype=torch.float32, device=d0)
            tin = hip.TaaIn(*[x.data_ptr() for x in t])
            assert L.tyr_taa(g.h, C.byref(tin), None, o.data_ptr(), None) == 0
            assert L.tyr_sync(g.h) == 0
            got.append(o)
    torch.cuda.synchronize()
    for k, (o, w) in enumerate(zip(got, wants)):
        assert_bits(o.cpu().numpy().reshape(-1, 4), w, f"stream call {k}")
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert call() == 0
            assert torch.cuda.current_device() == 1
    g.close()


# ---- GPU: quality ------------------------------------------------------------------------------------------------------
def figures(outs, refs):
    """tools/taa_bench.py's two figures over the last TAIL frames: (mean MSE, flicker = the mean over pixels and consecutive
    frame pairs of ((out_k - ref_k) - (out_{k-1} - ref_{k-1}))^2), in display space over the pixels both saw"""
    err, ok = [], []
    for o, (r, seen) in zip(outs[-TAIL:], refs[-TAIL:]):
        o = o.astype(np.float64)
        ok.append(seen & (o[:, 3] != 0))
        err.append(o[:, :3] - r[:, :3])
    m = float(np.mean([(e[s] ** 2).mean() for e, s in zip(err, ok)]))
    num = cnt = 0.0
    for k in range(1, TAIL):
        s = ok[k] & ok[k - 1]
        d = (err[k] - err[k - 1])[s]
        num += float((d ** 2).sum())
        cnt += d.size
    return m, num / cnt


@pytest.mark.gpu
def test_taa_quality_on_a_panning_and_a_still_sequence(hip):
    """16 frames at 1 spp of tools/temporal_bench.py's slowly panning framed Cornell view, and 16 of a still camera, through the
    recipe ending in svgf(resolve) -> taa with the shipped defaults, against a 1024-spp render per frame resolved by
    tyr_resolve.  Over the last 8 frames: the flicker of svgf -> taa over svgf alone's stays within the committed ratio
    (itself below 1: test_taa_bench_ratios_back_the_bounds) x 1.2, the MSE ratio within its committed value x 1.2, and on
    the still camera the MSE ratio is below 1."""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    sc = dataclasses.replace(sc, camera=hip.scenes.FRAMED_CAMERA)
    Wq, Hq, frames = 128, 72, 16
    bounds = quality_bounds()
    got = {}
    for name, cams in (("panning", [test_temporal.pan(sc.camera, k) for k in range(frames)]), ("still", [sc.camera] * frames)):
        g = hip.Renderer(Wq, Hq, 1 << 16)
        g.load_scene(sc, nodes, prims)
        sv_outs, taa_outs, seens = [], [], []
        prev = None
        for k, cam in enumerate(cams):
            sv, z, m, pd, seen = recipe_frame(g, cam, prev, k == 0)
            taa_outs.append(g.taa(sv, z, m, pd, reset=(k == 0)).cpu().numpy().reshape(-1, 4))
            sv_outs.append(sv.cpu().numpy().reshape(-1, 4))
            seens.append(seen)
            prev = cam
        g.close()
        refs, cache = [], {}
        for k, cam in enumerate(cams):
            if k < frames - TAIL:
                refs.append(None)
                continue
            key = (tuple(cam.position), tuple(cam.direction))
            if key not in cache:
                r = hip.Renderer(Wq, Hq, 1 << 18)
                r.load_scene(sc, nodes, prims)
                r.set_camera(cam)
                r.reset_accum()
                r.render(1024)
                dst = torch.zeros((Hq, Wq, 4), dtype=torch.float32, device="cuda:0")
                torch.cuda.synchronize()
                r.resolve_into(dst.data_ptr())
                torch.cuda.synchronize()
                cache[key] = (dst.cpu().numpy().reshape(-1, 4).astype(np.float64), r.blit_buffer()[:, 3] > 0)
                r.close()
            refs.append((cache[key][0], cache[key][1] & seens[k]))
        (ms, fs), (mt, ft) = figures(sv_outs, refs), figures(taa_outs, refs)
        got[name] = {"mse_ratio": mt / ms, "flicker_ratio": ft / fs}
        print(name, got[name], "svgf", (ms, fs), "taa", (mt, ft))
    assert got["panning"]["flicker_ratio"] <= bounds["panning_flicker"], (got, bounds)
    assert got["panning"]["mse_ratio"] <= bounds["panning_mse"], (got, bounds)
    assert got["still"]["mse_ratio"] < bounds["still_mse"], (got, bounds)


# ---- GPU: the C++ caller of the whole recipe ---------------------------------------------------------------------------
def read_ppm(path):
    data = open(path, "rb").read()
    m = re.match(rb"P6\s+(\d+)\s+(\d+)\s+(\d+)\s", data)
    w, h = int(m.group(1)), int(m.group(2))
    px = np.frombuffer(data[m.end():], np.uint8)
    return w, h, px


@pytest.mark.gpu
def test_denoised_flythrough_example(tmp_path):
    """examples/denoised_flythrough (built by `make example`) runs the whole recipe for six frames at 160 x 90 -- the camera parked for the
    first three, walked after them: it exits 0, its pictures have the right size and are not empty, and a frame after the walk
    began differs from a parked one by more than two parked ones differ"""
    exe = os.path.join(ROOT, "tyrant_amd", "bin", "denoised_flythrough")
    if not os.path.exists(exe):  # build() makes it (make example)
        subprocess.run(["make", "-s", "-C", CSRC, "example"], check=True, capture_output=True, timeout=900)
    W, H = 160, 90
    prefix = str(tmp_path / "fly")
    r = subprocess.run([exe, "0", "6", "1", prefix, str(W), str(H), "1", "3"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    for name in ("render_aov", "render_motion", "render", "svgf", "taa"):
        assert re.search(name + r" \d+\.\d+ ms", r.stdout), r.stdout
    assert "device_error 0" in r.stdout
    pics = []
    for f in range(1, 7):
        w, h, px = read_ppm(f"{prefix}_{f}.ppm")
        assert (w, h) == (W, H) and px.size == 3 * W * H
        assert px.max() > 0
        pics.append(px.astype(np.int32))
    diff = lambda a, b: float(np.abs(pics[a] - pics[b]).mean())  # noqa: E731
    assert diff(5, 2) > 0 and diff(5, 2) > diff(2, 1), (diff(5, 2), diff(2, 1))
