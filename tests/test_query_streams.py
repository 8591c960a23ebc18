"""What the query-like entries share on the host (host/query.cpp QueryLaunch): the caller's device comes back on every way out, and
every launch on a stream has its ticket word cleared in front of it and the stream's `done` event recorded behind it.  A
12-triangle box and 4 items per call: nothing here is about the kernels' answers, only about their being the same answers."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from query_support import box

F = np.float32
N = 4
ORIGINS = np.array([[0, 0, 60], [0, -40, 15], [3, 2, 15], [40, 40, 40]], F)  # above, beside, inside, off the box
DIRECTIONS = np.array([[0, 0, -1], [0, 1, 0], [0.6, 0, 0.8], [0, 0, 1]], F)
NORMALS = np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0], [0, 1, 0]], F)
RADIUS = np.array([0.0, 0.5, 1.0, 2.0], F)
ENTRIES = ("closest", "any", "nearest", "nearest_k", "hits", "sweep", "occlusion", "winding", "aov", "aov_chain")


def renderer(hip, flags=0):
    from tyrant_amd import scenes

    nodes, prims = hip.bvh_build(box())
    assert prims.shape[0] == 12
    g = hip.Renderer(16, 8, 1024, device=0, flags=flags)
    g.upload(nodes, prims)
    g.set_camera(scenes.cornell_box().camera)
    return g


def ask(g, entry):
    """the entry's answers through the binding, as a tuple of tensors"""
    o, d = ORIGINS.copy(), DIRECTIONS.copy()
    res = {
        "closest": lambda: g.query_closest(o, d),
        "any": lambda: (g.query_any(o, d),),
        "nearest": lambda: g.query_nearest(o),
        "nearest_k": lambda: g.query_nearest_k(o, 2, count=True, max_dist=np.full(N, 100, F)),
        "hits": lambda: g.query_hits(o, d, max_hits=2, two_sided=True),
        "sweep": lambda: g.query_sweep(o, d * F(50), RADIUS.copy(), normal=True),
        "occlusion": lambda: g.query_occlusion(o, NORMALS.copy(), samples=8, mask=True, bent=True),  # (two passes: a second `done` record)
        "winding": lambda: g.query_winding(o, terms=True),
        "aov": lambda: tuple(g.render_aov(1).values()),
        "aov_chain": lambda: tuple(g.render_aov(1, max_chain=2).values()),
    }[entry]()
    return tuple(x for x in res if x is not None)


def refused(hip, g, entry, p):
    """the entry's status with a required pointer missing (p: some device memory for the others)"""
    L, h = g.L, g.h
    return {
        "closest": lambda: L.tyr_query_closest(h, N, None, p, None, 0, p, p, None, None, None),
        "any": lambda: L.tyr_query_any(h, N, p, None, None, 0, p, None),
        "nearest": lambda: L.tyr_query_nearest(h, N, None, None, 0, C.byref(hip.NearestOut(p, p, None, None, None)), None),
        "nearest_k": lambda: L.tyr_query_nearest_k(h, N, p, None, 2, 0, None, None),
        "hits": lambda: L.tyr_query_hits(h, N, p, p, None, 2, 0, C.byref(hip.HitsOut(None, p, p, None, None, None)), None),
        "sweep": lambda: L.tyr_query_sweep(h, N, p, p, None, None, 0, C.byref(hip.SweepOut(p, p, None, None, None, None)), None),
        "occlusion": lambda: L.tyr_query_occlusion(h, N, p, None, None, 8, 1e-3, 0, 0, C.byref(hip.OcclusionOut(p, None, None, None, None)), None),
        "winding": lambda: L.tyr_query_winding(h, N, p, 2.0, None, None, None),
        "aov": lambda: L.tyr_render_aov(h, 1, None, None),
        "aov_chain": lambda: L.tyr_render_aov_chain(h, 1, 2, None, None, None),
    }[entry]()


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: output {k} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_callers_device_is_restored(hip, entry):
    """a ctx on device 0 called with device 1 current: device 1 is still current after a call that succeeds and after one
    refused for a missing pointer, and the answers are those of the same call made with device 0 current, bit for bit"""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    g = renderer(hip, flags=hip.TYR_FLAG_WINDING if entry == "winding" else 0)
    with torch.cuda.device(0):
        want = ask(g, entry)
        spare = torch.zeros(64, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
    with torch.cuda.device(1):
        got = ask(g, entry)
        assert torch.cuda.current_device() == 1
        assert refused(hip, g, entry, spare.data_ptr()) == hip.TYR_ERR_INVALID
        assert torch.cuda.current_device() == 1
        assert g.query_error() == 0
        assert torch.cuda.current_device() == 1
    same(got, want, entry)
    g.close()


@pytest.mark.gpu
def test_back_to_back_launches_on_one_stream(hip):
    """two different queries one behind the other on one stream with nothing between them -- on a stream of the caller's, then
    on the default stream, which the binding serves from its side stream: each launch starts from a cleared ticket word (it
    would deal no items otherwise and leave the sentinels), both give the answers of the same queries run alone, bit for
    bit, and tyr_query_error is 0"""
    import torch

    g = renderer(hip)
    L = g.L
    dev = torch.device("cuda", 0)
    o, d = torch.from_numpy(ORIGINS).to(dev), torch.from_numpy(DIRECTIONS).to(dev)
    t0, prim0 = g.query_closest(o, d)[:2]
    dist0, near0 = g.query_nearest(o)[:2]
    assert (prim0.cpu().numpy() >= 0).any() and (near0.cpu().numpy() >= 0).all()
    for what, stream in (("a stream of the caller's", torch.cuda.Stream(dev)), ("the default stream", None)):
        t, dist = torch.full((N,), 7.0, dtype=torch.float32, device=dev), torch.full((N,), 7.0, dtype=torch.float32, device=dev)
        prim, near = torch.full((N,), 7, dtype=torch.int32, device=dev), torch.full((N,), 7, dtype=torch.int32, device=dev)
        out = hip.NearestOut(dist.data_ptr(), near.data_ptr(), None, None, None)
        torch.cuda.synchronize()
        g._on_stream(stream, lambda h: L.tyr_query_closest(g.h, N, o.data_ptr(), d.data_ptr(), None, 0, t.data_ptr(), prim.data_ptr(), None, None, h), False, "tyr_query_closest")
        g._on_stream(stream, lambda h: L.tyr_query_nearest(g.h, N, o.data_ptr(), None, 0, C.byref(out), h), False, "tyr_query_nearest")
        (stream if stream is not None else torch.cuda.current_stream(dev)).synchronize()
        same((t, prim, dist, near), (t0, prim0, dist0, near0), what)
        assert g.query_error() == 0
    g.close()
