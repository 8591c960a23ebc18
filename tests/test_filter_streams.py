"""What the frame passes share on the host (host/driver_internal.hpp FilterLaunch): the caller's device comes back on every way
out, a call refused for its arguments leaves the pass's history as it was, and a ctx starts without one.  A 16x8 frame of seeded
inputs: nothing here is about the filters' answers, only about their being the same answers."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import test_svgf
import test_taa
from test_svgf import dev

F = np.float32
W, H = 16, 8
FILTERS = ("temporal", "svgf", "taa")  # the passes with a history
ENTRIES = ("denoise",) + FILTERS + ("allocate_samples",)


@functools.lru_cache(maxsize=None)
def host_frames():
    """four frames, each tests/test_svgf.py's seeded inputs (accum, albedo, normal, depth, motion, prev_depth) followed by
    tests/test_taa.py's (color, depth, motion, prev_depth)"""
    rng = np.random.default_rng(100 * W + H)
    z0 = test_svgf.plane_depth(W, H)
    return tuple(tuple(test_svgf.seeded_frame(W, H, rng, z0)) + tuple(test_taa.seeded_frame(W, H, rng, z0)) for _ in range(4))


def frames():
    return [[dev(a) for a in f] for f in host_frames()]


def ask(g, entry, f, reset=False):
    """the entry's outputs through the binding, the optional ones included, as a tuple of tensors"""
    import torch

    accum, alb, nrm, z, m, pdz, color, tz, tm, tpdz = f
    if entry == "denoise":
        return (g.denoise(alb, nrm, z, accum=accum),)
    if entry == "temporal":
        return g.temporal(alb, nrm, z, m, pdz, accum=accum, reset=reset, want_history_len=True)
    if entry == "svgf":
        return g.svgf(alb, nrm, z, m, pdz, accum=accum, reset=reset, want_variance=True)
    if entry == "taa":
        return (g.taa(color, tz, tm, tpdz, reset=reset),)
    spp, total = g.allocate_samples(accum[:, 0].contiguous(), 4 * W * H)
    return spp, torch.tensor([total], dtype=torch.int64)


def refused(hip, g, entry, f, how, spare):
    """the entry's status through the C entry with a required pointer missing (how == "pointer") or a parameter out of its
    range (how == "parameter"); spare: device memory for the outputs"""
    L, h = g.L, g.h
    accum, alb, nrm, z, m, pdz, color, tz, tm, tpdz = (x.data_ptr() for x in f)
    ptr = how == "pointer"
    if entry == "denoise":
        din = hip.DenoiseIn(accum, alb, None if ptr else nrm, z)
        return L.tyr_denoise(h, C.byref(din), C.byref(hip.DenoiseParams(5 if ptr else 0, 32.0, 0.02, 7, 0)), spare, None)
    if entry == "temporal":
        tin = hip.TemporalIn(accum, alb, nrm, z, None if ptr else m, pdz)
        return L.tyr_temporal(h, C.byref(tin), C.byref(hip.TemporalParams(16 if ptr else 0, 0.05, 0.9, 0)), spare, None, None)
    if entry == "svgf":
        sin = hip.SvgfIn(accum, alb, nrm, z, None if ptr else m, pdz)
        return L.tyr_svgf(h, C.byref(sin), C.byref(hip.SvgfParams(8, 0.05, 0.9, 3 if ptr else 9, 2.0, 0.02, 7, 0)), spare, None, None)
    if entry == "taa":
        tin = hip.TaaIn(color, None if ptr else tz, tm, tpdz)
        return L.tyr_taa(h, C.byref(tin), C.byref(hip.TaaParams(0.2 if ptr else 0.0, 1.5, 0)), spare, None)
    assert ptr  # (tyr_allocate_samples' parameters are no filter's)
    return L.tyr_allocate_samples(h, None, C.byref(hip.AllocateParams(4 * W * H, 1, 8)), spare, None, None)


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: output {k} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_callers_device_is_restored(hip, entry):
    """a ctx on device 0 called with device 1 current: device 1 is still current after a call that succeeds, after one refused
    for a missing pointer and (the four filters) after one refused for a parameter, and the outputs are those of the same call
    made with device 0 current on a fresh ctx, byte for byte"""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    g, fresh = hip.Renderer(W, H, 1024, device=0), hip.Renderer(W, H, 1024, device=0)
    with torch.cuda.device(0):
        f = frames()[0]
        spare = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        want = ask(fresh, entry, f)
        torch.cuda.synchronize()
    with torch.cuda.device(1):
        got = ask(g, entry, f)
        assert torch.cuda.current_device() == 1
        for how in ("pointer", "parameter")[: 1 if entry == "allocate_samples" else 2]:
            assert refused(hip, g, entry, f, how, spare.data_ptr()) == hip.TYR_ERR_INVALID, how
            assert torch.cuda.current_device() == 1
    same(got, want, entry)
    g.close()
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", FILTERS)
def test_a_refused_call_leaves_the_history_alone(hip, entry):
    """four frames (the first with the reset flag) fed once cleanly, and once with a refused call between every two of them --
    a missing input pointer and a bad parameter in turn: all four outputs, history length and variance included, are the same
    byte for byte"""
    import torch

    fs = frames()
    spare = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    clean, mixed = hip.Renderer(W, H, 1024), hip.Renderer(W, H, 1024)
    for k, f in enumerate(fs):
        want = ask(clean, entry, f, reset=(k == 0))
        got = ask(mixed, entry, f, reset=(k == 0))
        same(got, want, f"{entry} frame {k}")
        assert refused(hip, mixed, entry, f, ("pointer", "parameter")[k % 2], spare.data_ptr()) == hip.TYR_ERR_INVALID
    clean.close()
    mixed.close()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", FILTERS)
def test_a_fresh_ctx_has_no_history(hip, entry):
    """the first call of a ctx without the reset flag equals the first call of another with it; and a call with the reset flag
    in the middle of a sequence equals the call of a fresh ctx given the same frame -- byte for byte"""
    fs = frames()
    a, b, c, d = (hip.Renderer(W, H, 1024) for _ in range(4))
    same(ask(a, entry, fs[0]), ask(b, entry, fs[0], reset=True), f"{entry}: a first call")
    for k in range(2):
        ask(c, entry, fs[k], reset=(k == 0))
    same(ask(c, entry, fs[2], reset=True), ask(d, entry, fs[2]), f"{entry}: a reset in the middle")
    for g in (a, b, c, d):
        g.close()
