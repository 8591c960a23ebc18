"""What the query-like entries share on the host (host/query.cpp QueryLaunch): the caller's device comes back on every way out, and
every launch on a stream has its ticket word cleared in front of it and the stream's `done` event recorded behind it; with
more streams than ticket words, the least recently used word changes hands behind that event.  A 12-triangle box and 4 to 64
items per call: nothing here is about the kernels' answers, only about their being the same answers."""
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
BOX_LO, BOX_HI = (ORIGINS - F(12)).astype(F), (ORIGINS + F(12)).astype(F)
ENTRIES = ("closest", "any", "nearest", "nearest_k", "hits", "sweep", "occlusion", "winding", "aov", "aov_chain", "box", "tri", "segment")


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
        "box": lambda: g.query_box(BOX_LO.copy(), BOX_HI.copy(), max_prims=2),
        "tri": lambda: g.query_tri(o, o + d * F(30), o + NORMALS * F(30), max_prims=2),
        "segment": lambda: g.query_segment(o, o + d * F(50)),
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
        "box": lambda: L.tyr_query_box(h, N, p, None, 2, 0, C.byref(hip.BoxOut(p, p)), None),
        "tri": lambda: L.tyr_query_tri(h, N, p, p, None, 2, 0, C.byref(hip.TriOut(p, p)), None),
        "segment": lambda: L.tyr_query_segment(h, N, p, p, None, 0, C.byref(hip.SegmentOut(p, None, None, None, None, None, None)), None),
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


# ---- launches with nothing waiting behind them: the C calls on pre-filled outputs ----------------------------------------------
SENTINEL = {"float32": -7.25, "int32": -7, "uint8": 249}  # values no answer holds: dist2 >= 0, prim >= -1, count >= 0, region and feature <= 6
RAW = {  # kind -> (the C entry, the binding's out struct, its outputs' names, their trailing shapes and dtypes)
    "nearest": ("tyr_query_nearest", "NearestOut", ("dist2", "prim", "uv", "region", "point"), (((), "float32"), ((), "int32"), ((2,), "float32"), ((), "uint8"), ((3,), "float32"))),
    "box": ("tyr_query_box", "BoxOut", ("count", "prim"), (((), "int32"), ((2,), "int32"))),
    "tri": ("tyr_query_tri", "TriOut", ("count", "prim"), (((), "int32"), ((2,), "int32"))),
    "segment": ("tyr_query_segment", "SegmentOut", ("dist2", "prim", "s", "feature", "region", "on_segment", "on_triangle"),
                (((), "float32"), ((), "int32"), ((), "float32"), ((), "uint8"), ((), "uint8"), ((3,), "float32"), ((3,), "float32"))),
}


def sentinels(kind, n, dev):
    """the kind's outputs for n items, every value a sentinel"""
    import torch

    return [torch.full((n, *shape), SENTINEL[dtype], dtype=getattr(torch, dtype), device=dev) for shape, dtype in RAW[kind][3]]


def launch(hip, g, kind, ins, outs, stream):
    """the kind's C call on its input tensors `ins` into `outs`, on `stream`, returning as soon as it is enqueued"""
    L, n = g.L, ins[0].shape[0]
    i = [t.data_ptr() for t in ins]
    out = getattr(hip, RAW[kind][1])(*(t.data_ptr() for t in outs))
    call = {
        "nearest": lambda h: L.tyr_query_nearest(g.h, n, i[0], None, 0, C.byref(out), h),
        "box": lambda h: L.tyr_query_box(g.h, n, i[0], i[1], 2, 0, C.byref(out), h),
        "tri": lambda h: L.tyr_query_tri(g.h, n, i[0], i[1], i[2], 2, 0, C.byref(out), h),
        "segment": lambda h: L.tyr_query_segment(g.h, n, i[0], i[1], None, 0, C.byref(out), h),
    }[kind]
    g._on_stream(stream, call, False, RAW[kind][0])


def restated(kind, ins, prims):
    """the kind's numpy restatement for the numpy inputs `ins`"""
    import box_ref
    import nearest_ref
    import segment_ref
    import tri_ref

    return {"nearest": lambda: nearest_ref.nearest(*ins, prims), "box": lambda: box_ref.box(*ins, prims, 2), "tri": lambda: tri_ref.tri(*ins, prims, 2),
            "segment": lambda: segment_ref.segment(*ins, prims)}[kind]()


@pytest.mark.gpu
def test_back_to_back_launches_on_one_stream(hip):
    """different queries one behind the other on one stream with nothing between them -- closest, nearest, box, tri and segment
    on a stream of the caller's, then on the default stream, which the binding serves from its side stream: each launch starts
    from a cleared ticket word (it would deal no items otherwise and leave the sentinels), every one gives the answers of the
    same query run alone, bit for bit, and tyr_query_error is 0"""
    import torch

    g = renderer(hip)
    L = g.L
    dev = torch.device("cuda", 0)
    o, d = torch.from_numpy(ORIGINS).to(dev), torch.from_numpy(DIRECTIONS).to(dev)
    t0, prim0 = g.query_closest(o, d)[:2]
    dist0, near0 = g.query_nearest(o)[:2]
    assert (prim0.cpu().numpy() >= 0).any() and (near0.cpu().numpy() >= 0).all()
    more = {"box": (torch.from_numpy(BOX_LO).to(dev), torch.from_numpy(BOX_HI).to(dev)), "tri": (o, o + d * 30, o + torch.from_numpy(NORMALS).to(dev) * 30), "segment": (o, o + d * 50)}
    alone = {"box": g.query_box(*more["box"], max_prims=2), "tri": g.query_tri(*more["tri"], max_prims=2), "segment": g.query_segment(*more["segment"])}
    assert all((alone[k][0].cpu().numpy() > 0).any() for k in ("box", "tri")) and (alone["segment"][1].cpu().numpy() >= 0).all()
    for what, stream in (("a stream of the caller's", torch.cuda.Stream(dev)), ("the default stream", None)):
        t, dist = torch.full((N,), 7.0, dtype=torch.float32, device=dev), torch.full((N,), 7.0, dtype=torch.float32, device=dev)
        prim, near = torch.full((N,), 7, dtype=torch.int32, device=dev), torch.full((N,), 7, dtype=torch.int32, device=dev)
        out = hip.NearestOut(dist.data_ptr(), near.data_ptr(), None, None, None)
        outs = {k: sentinels(k, N, dev) for k in more}
        torch.cuda.synchronize()
        g._on_stream(stream, lambda h: L.tyr_query_closest(g.h, N, o.data_ptr(), d.data_ptr(), None, 0, t.data_ptr(), prim.data_ptr(), None, None, h), False, "tyr_query_closest")
        g._on_stream(stream, lambda h: L.tyr_query_nearest(g.h, N, o.data_ptr(), None, 0, C.byref(out), h), False, "tyr_query_nearest")
        for k in more:
            launch(hip, g, k, more[k], outs[k], stream)
        (stream if stream is not None else torch.cuda.current_stream(dev)).synchronize()
        same((t, prim, dist, near), (t0, prim0, dist0, near0), what)
        for k in more:
            same(outs[k], alone[k], f"{what}: {k}")
        assert g.query_error() == 0
    g.close()


# ---- more streams than ticket words -------------------------------------------------------------------------------------------
def ticket_words():
    """kQueryTickets of host/query.cpp: the streams a ctx serves before a ticket word changes hands"""
    import os
    import re

    from conftest import ROOT

    src = open(os.path.join(ROOT, "tyrant_amd", "csrc", "host", "query.cpp")).read()
    return int(re.search(r"constexpr uint32_t kQueryTickets = (\d+);", src).group(1))


class Streams:
    """n streams with n different handles, kept alive until close().  torch.cuda.Stream() deals its handles from a pool of 32 per
    priority, round robin: 72 of them are 32 streams to the library, which knows a stream by its handle, and would never use up
    its ticket words.  These are streams of the HIP runtime the library's own calls are bound to (hipStreamCreateWithFlags,
    non-blocking, looked up through the library's handle: the process holds one runtime, tests/conftest.py) as
    torch.cuda.ExternalStream, which is a torch.cuda.Stream."""

    def __init__(self, hip, n, dev):
        import torch

        self.rt = hip.lib()
        self.rt.hipStreamCreateWithFlags.argtypes, self.rt.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p), C.c_uint], [C.c_void_p]
        self.handles = []
        with torch.cuda.device(dev):
            for _ in range(n):
                h = C.c_void_p()
                assert self.rt.hipStreamCreateWithFlags(C.byref(h), 1) == 0 and h.value  # hipStreamNonBlocking
                self.handles.append(h.value)
        self.streams = [torch.cuda.ExternalStream(h, device=dev) for h in self.handles]
        assert len({s.cuda_stream for s in self.streams}) == n and all(isinstance(s, torch.cuda.Stream) for s in self.streams)

    def close(self):
        self.streams = []
        for h in self.handles:
            assert self.rt.hipStreamDestroy(h) == 0
        self.handles = []


def job(kind, rng, prims, n):
    """seeded inputs of one launch of `kind` round the box: numpy arrays"""
    from query_support import box_points

    if kind == "nearest":
        return (box_points(rng, prims, n),)
    if kind == "segment":
        return box_points(rng, prims, n), box_points(rng, prims, n)
    c, half = box_points(rng, prims, n), rng.uniform(0.5, 6.0, (n, 3))
    return (c - half).astype(F), (c + half).astype(F)


@pytest.mark.gpu
def test_ticket_words_change_hands(hip):
    """one ctx, 72 streams of its device with 72 different handles, a query of 4 to 64 items on each -- nearest, box and segment
    in turn, each into sentinel-filled outputs of its own -- on streams 0 .. 71 and then on 71 .. 0 without a wait: the last eight
    of round one take the ticket words of the eight least recently used streams behind an event, and in round two the streams that
    lost theirs take them back, so whose word is oldest matters.  A word two launches share deals items twice or not at all.
    After one synchronize every output of both rounds is the numpy restatement's bit for bit -- no sentinel is left -- and
    tyr_query_error is 0.  Then an upload of the same scene, which waits for every word's last launch, and a query on a 73rd
    stream: right as well."""
    import torch

    from query_support import same as same_outputs

    words, n_streams = ticket_words(), 72
    assert words == 64 and n_streams == words + 8
    g = renderer(hip)
    nodes, prims = hip.bvh_build(box())
    dev = torch.device("cuda", 0)
    made = Streams(hip, n_streams + 1, dev)
    streams = made.streams
    rng = np.random.default_rng(72)
    kinds = [("nearest", "box", "segment")[i % 3] for i in range(n_streams + 1)]
    sizes = [4 + (7 * i) % 61 for i in range(n_streams + 1)]
    assert min(sizes) == 4 and max(sizes) == 64
    ins = [job(kinds[i], rng, prims, sizes[i]) for i in range(n_streams + 1)]
    want = [restated(kinds[i], ins[i], prims) for i in range(n_streams + 1)]
    assert all((w[1] >= 0).any() for w in want)  # (answers, not misses)
    on_dev = [tuple(torch.from_numpy(a).to(dev) for a in x) for x in ins]
    outs = {(r, i): sentinels(kinds[i], sizes[i], dev) for r in (1, 2, 3) for i in range(n_streams + 1)}
    torch.cuda.synchronize()
    for i in range(n_streams):
        launch(hip, g, kinds[i], on_dev[i], outs[1, i], streams[i])
    for i in reversed(range(n_streams)):
        launch(hip, g, kinds[i], on_dev[i], outs[2, i], streams[i])
    torch.cuda.synchronize()

    def check(r, i):
        got = tuple(t.cpu().numpy() for t in outs[r, i])
        same_outputs(RAW[kinds[i]][2], got, want[i], f"round {r}, stream {i} ({kinds[i]}, {sizes[i]} items)")
        for name, a in zip(RAW[kinds[i]][2], got):
            if name in ("dist2", "prim", "count"):
                assert not (a == SENTINEL[str(a.dtype)]).any(), (r, i, name)

    for r in (1, 2):
        for i in range(n_streams):
            check(r, i)
    assert g.query_error() == 0
    g.upload(nodes, prims)
    launch(hip, g, kinds[n_streams], on_dev[n_streams], outs[3, n_streams], streams[n_streams])
    torch.cuda.synchronize()
    check(3, n_streams)
    assert g.query_error() == 0
    g.close()
    torch.cuda.synchronize()
    made.close()
