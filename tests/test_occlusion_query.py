"""Batched ambient-occlusion queries on the uploaded scene (tyr_query_occlusion, hip/occlusion.hip; Renderer.query_occlusion):
`samples` cosine-weighted any-hit rays per point, made on the device, answered as a count, a bit mask and a bent sum per point
-- include/tyr_c.h "Occlusion queries", bit for bit against its numpy restatement (tests/occlusion_ref.py), whose any-hit is the
reference's own.

CPU: the restatement by hand, the sampler's statistics, what the fixtures are for, what the compiler made of the kernels, the
ABI.  GPU: every output by bits over sample counts that cross word, wave and chunk boundaries, the sibling tyr_query_any's
answer on the device for the rays the query reports, independence of batch and optional outputs, hostile input, isolation from
the render, streams, refit and argument checks."""
import ctypes as C
import functools

import numpy as np
import pytest

import occlusion_ref as ref
from conftest import bits
from kernel_resources import kernel_resources
from query_support import assert_query_abi, assert_render_undisturbed, build, check_kernel_budget, deformed, no_triangles, on_side_stream, query_exists, renderer, take
from query_support import same as same_outputs

F = np.float32
U = np.uint32
VERY_FAR = F(1e20)
NAMES = ("visible", "mask", "bent", "origin", "direction")
SAMPLE_COUNTS = (1, 7, 32, 33, 64, 100)
# (max_dist: None or the fixture's per-point mix of 10, +inf and VERY_FAR; bias; seed) -- every value of each in the first four.
# A sample count takes as many of them, from the front, as keep its CPU any-hit rays at 64 Ki (512 points x S x combos).
COMBOS = [("mixed", 1e-3, 0x9E3779B9), (None, 0.0, 7), ("mixed", 1e-2, 7), (None, 1e-3, 0x9E3779B9), ("mixed", 0.0, 0x9E3779B9), (None, 1e-2, 7),
          (None, 1e-3, 7), ("mixed", 1e-3, 7), (None, 0.0, 0x9E3779B9), ("mixed", 1e-2, 0x9E3779B9), (None, 1e-2, 0x9E3779B9), ("mixed", 0.0, 7)]


def combos_for(S, n=512):
    return COMBOS[:max(1, min(len(COMBOS), 65536 // (n * S)))]


_the_query_exists = query_exists("tyr_query_occlusion")  # nothing here means anything without the entry point


# ---- fixtures (numpy only; made once, never changed) ------------------------------------------------------------------
def big_triangle():
    """one triangle in the plane z = 0 facing +z, 2e4 across"""
    from tyrant_amd import scenes

    return scenes.make_triangles(np.array([[-1e4, -1e4, 0]], F), np.array([[1e4, -1e4, 0]], F), np.array([[0, 1e4, 0]], F))


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(nodes, prims, spheres or None, points, normals, mixed max_dist)"""
    from tyrant_amd import scenes

    spheres = None
    if name == "soup":
        n = 4096
        nodes, prims = build(scenes.random_soup(2000, edge=16.0))
        rng = np.random.default_rng(71)
        lo, hi = nodes[0]["bounds"][0].astype(np.float64), nodes[0]["bounds"][1].astype(np.float64)
        p = (lo + (hi - lo) * rng.random((n, 3))).astype(F)
        nr = rng.normal(size=(n, 3)).astype(F)
    elif name in ("heightfield32", "heightfield128"):
        cells, n, seed = (32, 512, 72) if name == "heightfield32" else (128, 2048, 73)
        nodes, prims = build(scenes.heightfield(cells))
        rng = np.random.default_rng(seed)
        t = prims[rng.integers(0, prims.shape[0], n)]
        e1, e2 = t["e1"].astype(F), t["e2"].astype(F)
        p = ((t["vert"] + (e1 * F(0.3)).astype(F)).astype(F) + (e2 * F(0.3)).astype(F)).astype(F)
        nr = np.cross(e1.astype(np.float64), e2.astype(np.float64)).astype(F)  # left unnormalised
    elif name == "cornell":
        n = 2048
        sc = scenes.cornell_box()
        nodes, prims = build(sc.triangles)
        spheres = sc.spheres
        rng = np.random.default_rng(74)
        lo, hi = np.array([-50.0, -120.0, 0.0]), np.array([50.0, 50.0, 100.0])  # the room and the space in front of its opening
        p = (lo + (hi - lo) * rng.random((n, 3))).astype(F)
        nr = rng.normal(size=(n, 3)).astype(F)
    else:
        raise KeyError(name)
    md = np.select([rng.random(n) < 0.5, rng.random(n) < 0.5], [F(10.0), F(np.inf)], VERY_FAR).astype(F)
    for a in (nodes, prims, p, nr, md) + (() if spheres is None else (spheres,)):
        a.setflags(write=False)
    return nodes, prims, spheres, p, nr, md


@functools.lru_cache(maxsize=None)
def reference(name, n, S, md, bias, seed, spheres=False):
    """the restatement's answer for the first n points of a fixture, computed once per process"""
    nodes, prims, sph, p, nr, mixed = fixture(name)
    out = ref.occlusion(nodes, prims, p[:n], nr[:n], S, None if md is None else mixed[:n], bias, seed, sph if spheres else None)
    for a in out:
        a.setflags(write=False)
    return out


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------
def test_hand_cases():
    """one large triangle facing +z: a point above it looking down sees nothing, and everything with max_dist below the gap; the
    same from behind the back face sees everything; a zero or NaN normal gives the invalid row"""
    nodes, prims = build(big_triangle())
    S = 16
    p = np.array([[0, -3000, 1], [0, -3000, 1], [0, -3000, -1], [1, 2, 3], [1, 2, 3], [np.nan, 2, 3]], F)
    nr = np.array([[0, 0, -1], [0, 0, -2], [0, 0, 1], [0, 0, 0], [0, np.nan, 1], [0, 0, 1]], F)
    md = np.array([VERY_FAR, 0.5, VERY_FAR, VERY_FAR, VERY_FAR, VERY_FAR], F)
    visible, mask, bent, origin, d = ref.occlusion(nodes, prims, p, nr, S, md, bias=0.0, seed=3)
    assert visible.tolist() == [0, S, S, 0, 0, 0]
    assert mask[:, 0].tolist() == [0, 0xFFFF, 0xFFFF, 0, 0, 0]
    assert not bent[0].any() and bent[1, 2] < 0 and bent[2, 2] > 0 and not bent[3:].any()
    assert np.array_equal(bits(origin), bits(p)) and not d[3:].any() and (d[0, :, 2] < 0).all() and (d[2, :, 2] > 0).all()
    # the same without max_dist and with a bias: the origin moves along the unit normal
    _, _, _, o2, _ = ref.occlusion(nodes, prims, p[1:2], nr[1:2], 4, None, bias=0.25, seed=3)
    assert o2.tolist() == [[0.0, -3000.0, 0.75]]


def test_sampler_sanity():
    """seed, point index and sample each change the state; over 1 << 16 samples every direction is a unit vector within 2 ulp and
    lies in the normal's hemisphere, and the mean of dot(d, w) is within 4 standard errors of 2/3 (cosine weighting: E = 2/3,
    variance 1/2 - 4/9 = 1/18)"""
    a = ref.states(1, [5], [9])[0, 0]
    assert a != ref.states(2, [5], [9])[0, 0] and a != ref.states(1, [6], [9])[0, 0] and a != ref.states(1, [5], [10])[0, 0]
    assert ref.h([0]).tolist() == [0]
    st = ref.states(1234, np.arange(64), np.arange(1024))
    assert np.unique(st).size > 0.999 * st.size
    n, S = 64, 1024
    nr = np.random.default_rng(75).normal(size=(n, 3)).astype(F)
    valid, o, w, u, v = ref.frames(np.zeros((n, 3), F), nr, 0.0)
    assert valid.all()
    d = ref.directions(w, u, v, 1234, np.arange(n), S).astype(np.float64)
    length = np.sqrt((d * d).sum(axis=2))
    assert np.abs(length - 1.0).max() <= 2 * 2.0 ** -23
    cos = (d * w.astype(np.float64)[:, None, :]).sum(axis=2)
    assert (cos >= 0).all()
    se = np.sqrt((1.0 / 18.0) / (n * S))
    print("mean of dot(d, w):", cos.mean(), "standard error:", se)
    assert abs(cos.mean() - 2.0 / 3.0) <= 4 * se


def test_fixtures_reach_what_they_are_for():
    """256 points, 32 samples, by the restatement alone: on the soup and on heightfield(32) at least half of the points see a part
    of their hemisphere, at least one sees all of it, and on the soup at least one sees nothing"""
    for name, md in (("soup", None), ("soup", "mixed"), ("heightfield32", None)):
        visible = reference(name, 256, 32, md, 1e-3, 0x9E3779B9)[0]  # (with seed 7 no point of the heightfield sees all 32)
        part, full, none = ((visible > 0) & (visible < 32)).mean(), (visible == 32).mean(), (visible == 0).mean()
        print(f"{name}, max_dist {md}: partly visible {part:.3f}, fully visible {full:.3f}, fully blocked {none:.3f}, mean visibility {visible.mean() / 32:.3f}")
        assert part >= 0.5 and full > 0, name
        if name == "soup":
            assert none > 0


def test_occlusion_kernels_keep_registers_and_lds_in_budget():
    """both instantiations of k_occlusion: no vector spills; scratch no larger than the LdsStack's private spill arrays plus
    alignment (as k_query_any); occupancy and LDS that admit the five blocks per CU the launch bounds name; the resolve pass
    without scratch"""
    res = kernel_resources("occlusion")
    for sph in (0, 1):
        check_kernel_budget(res, f"k_occlusionILb{sph}E", 1, (64 - 12) * 4 + 16)
    names = [n for n in res if "k_occlusion_bent" in n]
    assert len(names) == 1, list(res)
    print(names[0], res[names[0]])
    assert res[names[0]]["ScratchSize [bytes/lane]"] == 0 and res[names[0]]["VGPRs Spill"] == 0


def test_abi_declares_and_exports_the_query(hip):
    assert_query_abi(hip, "tyr_query_occlusion", "tyr_occlusion_out", hip.OcclusionOut, 5, (r"TYR_QUERY_OCCLUSION_MAX_SAMPLES\s+1024\b",))
    assert hip.TYR_QUERY_OCCLUSION_MAX_SAMPLES == 1024


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def ask(g, p, nr, S, md=None, bias=1e-3, seed=0, spheres=False, mask=True, bent=True, rays=True, **kw):
    """query_occlusion's tuple as numpy arrays, the integer ones as the library's uint32 (the fixtures' arrays are read-only:
    torch wants its own)"""
    res = g.query_occlusion(np.array(p), np.array(nr), samples=S, max_dist=None if md is None else np.array(md), bias=bias, seed=seed, spheres=spheres, mask=mask, bent=bent,
                            rays=rays, **kw)
    res = [None if x is None else x.cpu().numpy() for x in res]
    return tuple(None if x is None else (x.view(U) if x.dtype == np.int32 else x) for x in res)


same = functools.partial(same_outputs, NAMES)  # (an output that was not asked for is None, and is not compared)


def pack(vis):
    """(n, S) bool -> the contract's (n, W) uint32 mask words"""
    n, S = vis.shape
    by = np.packbits(vis, axis=1, bitorder="little")
    out = np.zeros((n, 4 * ((S + 31) // 32)), dtype=np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u4").astype(U)


# ---- GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S", SAMPLE_COUNTS)
@pytest.mark.parametrize("name", ["soup", "heightfield32", "cornell"])
def test_bit_for_bit_against_the_restatement(hip, name, S):
    """512 points: visible, mask, bent, origin and direction by bits, at sample counts that put a point's samples across mask
    words (33), waves and chunks (7 and 100 divide neither 64 nor the 64 .. 256-item chunks) and one item per point (1), with
    and without a per-point max_dist of 10, +inf and VERY_FAR, bias 0, 1e-3 and 1e-2, two seeds (combos_for: every value at the
    small sample counts, the first of COMBOS at the large ones); the cornell box with its sphere table and TYR_QUERY_SPHERES"""
    nodes, prims, sph, p, nr, mixed = fixture(name)
    g = renderer(hip, nodes, prims, spheres=sph)
    n = 512
    for md, bias, seed in combos_for(S):
        want = reference(name, n, S, md, bias, seed, sph is not None)
        got = ask(g, p[:n], nr[:n], S, None if md is None else mixed[:n], bias, seed, spheres=sph is not None)
        same(got, want, f"{name}, S {S}, max_dist {md}, bias {bias}, seed {seed}")
        assert 0 < want[0].sum() < n * S
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_the_largest_sample_count(hip):
    """S = 1024 on 48 points of the soup: 32 mask words per point"""
    nodes, prims, sph, p, nr, mixed = fixture("soup")
    g = renderer(hip, nodes, prims)
    want = reference("soup", 48, 1024, "mixed", 1e-3, 7)
    same(ask(g, p[:48], nr[:48], 1024, mixed[:48], 1e-3, 7), want, "soup, S 1024")
    assert ((want[0] > 0) & (want[0] < 1024)).sum() > 24
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,S", [("soup", 4096, 64), ("heightfield128", 2048, 100), ("cornell", 2048, 64)])
def test_the_siblings_answer_on_the_device(hip, name, n, S):
    """larger batches, on the device alone: visible is S minus tyr_query_any's count over the rays the query reports, and the
    mask is the complement of its answers by bits -- with and without max_dist, the cornell box with the sphere table"""
    import torch

    nodes, prims, sph, p, nr, mixed = fixture(name)
    g = renderer(hip, nodes, prims, spheres=sph)
    spheres = sph is not None
    for md in (None, mixed[:n]):
        visible, mask, bent, origin, direction = g.query_occlusion(np.array(p[:n]), np.array(nr[:n]), samples=S, max_dist=None if md is None else np.array(md), seed=5,
                                                                   spheres=spheres, mask=True, rays=True)
        o = origin.repeat_interleave(S, dim=0).contiguous()
        d = direction.reshape(-1, 3)
        t = None if md is None else torch.from_numpy(np.array(md)).to(o.device).repeat_interleave(S).contiguous()
        occ = g.query_any(o, d, t, spheres=spheres).view(n, S)
        assert torch.equal(visible, (S - occ.sum(dim=1)).to(torch.int32))
        assert np.array_equal(mask.cpu().numpy().view(U), pack(~occ.cpu().numpy()))
        v = visible.cpu().numpy()
        assert ((v > 0) & (v < S)).mean() > 0.25
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_independence(hip):
    """the first 100 rows of a 4096-point batch are a 100-point batch's; asking or not asking for mask, bent or rays changes no
    other output; batches of 1, 63, 64, 65 and 257 points with 5 samples each, against the restatement"""
    nodes, prims, sph, p, nr, mixed = fixture("soup")
    g = renderer(hip, nodes, prims)
    big = ask(g, p, nr, 33, mixed, 1e-3, 11)
    small = ask(g, p[:100], nr[:100], 33, mixed[:100], 1e-3, 11)
    same(small, take(big, slice(0, 100)), "the first 100 of 4096")
    assert ((big[0] > 0) & (big[0] < 33)).mean() > 0.25
    for use_mask, use_bent, use_rays in ((False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = ask(g, p[:100], nr[:100], 33, mixed[:100], 1e-3, 11, mask=use_mask, bent=use_bent, rays=use_rays)
        assert (got[1] is not None) == (use_mask or use_bent) and (got[2] is not None) == use_bent and (got[3] is not None) == (got[4] is not None) == use_rays
        same(got, small, f"mask {use_mask}, bent {use_bent}, rays {use_rays}")
    want = reference("soup", 257, 5, "mixed", 1e-3, 11)
    for m in (1, 63, 64, 65, 257):
        same(ask(g, p[:m], nr[:m], 5, mixed[:m], 1e-3, 11), take(want, slice(0, m)), f"n = {m}")
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_a_batch_of_more_than_2_31_items(hip):
    """2^21 + 3 points with 1024 samples each are 2^31 + 3072 items: the batch goes out as two launches, the second with the
    last three points.  Rows on both sides of the cut, and the batch's first and last, against the restatement with the points'
    own batch indices (max_dist 10 keeps the 2 Gi rays short)"""
    nodes, prims, sph, p, nr, mixed = fixture("soup")
    g = renderer(hip, nodes, prims)
    n, S = (1 << 21) + 3, 1024
    idx = np.arange(n) % 61
    md = np.full(n, 10.0, F)
    visible = ask(g, p[idx], nr[idx], S, md, 1e-3, 21, mask=False, bent=False, rays=False)[0]
    assert g.query_error() == 0
    for first in (0, (1 << 21) - 2, n - 3):
        rows = slice(first, min(first + 3, n))
        want = ref.occlusion(nodes, prims, p[idx[rows]], nr[idx[rows]], S, md[rows], 1e-3, 21, first=first)[0]
        assert np.array_equal(visible[rows], want), (first, visible[rows].tolist(), want.tolist())
        assert ((want > 0) & (want < S)).any()
    assert not np.array_equal(visible[:61], visible[61:122])  # the same 61 points under other indices: other samples
    g.close()


@pytest.mark.gpu
def test_hostile_input(hip):
    """NaN, infinite, zero, 1e30 and 1e-30 normals, NaN points, max_dist of 0, negative and NaN; a scene that is one triangle; a
    scene without triangles, with and without the spheres -- all against the restatement"""
    from tyrant_amd import scenes

    nodes, prims, sph, p, nr, mixed = fixture("soup")
    rng = np.random.default_rng(76)
    n, S = 384, 8
    p, nr, md = p[:n].copy(), nr[:n].copy(), mixed[:n].copy()
    kind = rng.integers(0, 12, n)
    for i in np.nonzero(kind == 0)[0]:
        nr[i, rng.integers(0, 3)] = (np.nan, np.inf, -np.inf)[rng.integers(0, 3)]
    nr[kind == 1] = 0.0
    nr[kind == 2] *= F(1e30)   # dot(normal, normal) overflows
    nr[kind == 3] *= F(1e-30)  # ... and underflows to 0
    p[kind == 4, 1] = np.nan
    md[kind == 5] = 0.0
    md[kind == 6] = -7.0
    md[kind == 7] = np.nan
    want = ref.occlusion(nodes, prims, p, nr, S, md, 1e-3, 13)
    assert (want[0][kind <= 4] == 0).all() and (want[0][(kind >= 5) & (kind <= 7)] == S).all() and ((want[0] > 0) & (want[0] < S)).any()
    g = renderer(hip, nodes, prims)
    same(ask(g, p, nr, S, md, 1e-3, 13), want, "hostile")
    # one triangle
    n1, p1 = build(big_triangle())
    q = np.array([[0, -3000, 1], [0, -3000, 1], [0, -3000, -1], [3e4, 0, 1]], F)
    qn = np.array([[0, 0, -1], [1, 0, -0.05], [0, 0, 1], [0, 0, -1]], F)
    g.upload(n1, p1)
    want = ref.occlusion(n1, p1, q, qn, 64, None, 0.0, 17)
    assert want[0][0] == 0 and 0 < want[0][1] < 64 and want[0][2] == 64 and want[0][3] == 64
    same(ask(g, q, qn, 64, None, 0.0, 17), want, "one triangle")
    # no triangles: the spheres alone, or everything visible
    sc = scenes.cornell_box()
    none_n, none_p = no_triangles()
    g.upload(none_n, none_p)
    g.set_spheres(sc.spheres)
    _, _, _, cp, cn, cmd = fixture("cornell")
    want = ref.occlusion(none_n, none_p, cp[:256], cn[:256], 16, None, 1e-3, 19, spheres=sc.spheres)
    assert ((want[0] > 0) & (want[0] < 16)).sum() > 64
    same(ask(g, cp[:256], cn[:256], 16, None, 1e-3, 19, spheres=True), want, "spheres alone")
    got = ask(g, cp[:256], cn[:256], 16, None, 1e-3, 19, spheres=False)
    assert (got[0] == 16).all() and (got[1] == 0xFFFF).all()
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_occlusion_queries_leave_the_render_alone(hip):
    """a Cornell-box render (64 x 64, 2 spp) with occlusion queries between its tyr_render calls: the same accumulation buffer,
    counters and queues as without them"""
    nodes, prims, sph, p, nr, mixed = fixture("cornell")  # (the Cornell box's own tree and sphere table: what the render loads)
    want = reference("cornell", 512, 32, "mixed", 1e-3, 0x9E3779B9, True)

    def between(g):
        same(ask(g, p[:512], nr[:512], 32, mixed[:512], 1e-3, 0x9E3779B9, spheres=True), want, "between two renders")
        ask(g, p, nr, 64, None, 1e-2, 1, spheres=False)

    assert_render_undisturbed(between)


@pytest.mark.gpu
def test_refit_side_stream_and_invalid_arguments(hip):
    """a refit between two queries changes the second to the refitted scene's answer; a torch side stream works; bad arguments
    are refused before any launch; tyr_query_error stays 0"""
    import torch

    nodes, prims, sph, p, nr, mixed = fixture("heightfield32")
    n, S = 256, 32
    p, nr, md = p[:n], nr[:n], mixed[:n]
    g = renderer(hip, nodes, prims, flags=64)  # TYR_FLAG_REFIT
    before = reference("heightfield32", 256, 32, "mixed", 1e-3, 7)
    same(ask(g, p, nr, S, md, 1e-3, 7), before, "before the refit")
    moved = deformed(prims, 2.0)
    new_nodes = g.refit(moved, want_nodes=True)
    want = ref.occlusion(new_nodes, moved, p, nr, S, md, 1e-3, 7)
    assert not np.array_equal(want[0], before[0])
    same(ask(g, p, nr, S, md, 1e-3, 7), want, "after the refit")
    # a side stream, device tensors taken in place
    tp, tn, tm = torch.from_numpy(np.array(p)).cuda(), torch.from_numpy(np.array(nr)).cuda(), torch.from_numpy(np.array(md)).cuda()
    res = on_side_stream(lambda side: g.query_occlusion(tp, tn, samples=S, max_dist=tm, bias=1e-3, seed=7, mask=True, bent=True, rays=True, stream=side))
    res = [x.cpu().numpy() for x in res]
    same((res[0].view(U), res[1].view(U)) + tuple(res[2:]), want, "side stream")

    L, h, P = hip.lib(), g.h, C.c_void_p
    m = 4
    vis, msk, bnt = torch.full((m,), 7, dtype=torch.int32).cuda(), torch.full((m, 1), 7, dtype=torch.int32).cuda(), torch.full((m, 3), 7, dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    ok = hip.OcclusionOut(vis.data_ptr(), msk.data_ptr(), bnt.data_ptr(), None, None)
    pp, pn = P(tp.data_ptr()), P(tn.data_ptr())
    inv = hip.TYR_ERR_INVALID
    call = lambda ctx=h, n=m, a=pp, b=pn, s=S, bias=1e-3, flags=0, out=ok: L.tyr_query_occlusion(ctx, n, a, b, None, s, bias, 7, flags, None if out is None else C.byref(out), None)  # noqa: E731
    assert call(ctx=None) == inv
    assert call(a=None) == inv
    assert call(b=None) == inv
    assert call(out=None) == inv
    assert call(out=hip.OcclusionOut(None, msk.data_ptr(), None, None, None)) == inv
    assert call(out=hip.OcclusionOut(vis.data_ptr(), None, bnt.data_ptr(), None, None)) == inv  # bent without mask
    assert call(s=0) == inv
    assert call(s=hip.TYR_QUERY_OCCLUSION_MAX_SAMPLES + 1) == inv
    assert call(flags=hip.TYR_QUERY_TWO_SIDED) == inv
    assert call(flags=hip.TYR_QUERY_SPHERES | 4) == inv
    assert call(n=1 << 31) == inv
    assert call(bias=float("nan")) == inv
    assert call(bias=float("inf")) == inv
    assert L.tyr_query_occlusion(h, 0, None, None, None, S, 1e-3, 7, 0, None, None) == 0  # n == 0: nothing to do
    empty = hip.Renderer(64, 64, 1024)  # no scene uploaded
    assert call(ctx=empty.h) == hip.TYR_ERR_NO_SCENE
    empty.close()
    with pytest.raises(ValueError):
        g.query_occlusion(tp.double(), tn)
    with pytest.raises(ValueError):
        g.query_occlusion(tp, tn[:, :2].contiguous())
    with pytest.raises(ValueError):
        g.query_occlusion(tp, tn, max_dist=tm[:5])
    with pytest.raises(ValueError):
        g.query_occlusion(tp, tn, samples=1025)
    torch.cuda.synchronize()
    assert (vis.cpu().numpy() == 7).all() and (msk.cpu().numpy() == 7).all() and (bnt.cpu().numpy() == 7).all()  # the refused calls wrote nothing
    empty_ans = ask(g, p[:0], nr[:0], 33)
    assert empty_ans[0].shape == (0,) and empty_ans[1].shape == (0, 2) and empty_ans[2].shape == (0, 3) and empty_ans[4].shape == (0, 33, 3)
    assert call(flags=0) == 0
    assert g.query_error() == 0
    w4 = ref.occlusion(new_nodes, moved, p[:m], nr[:m], S, None, 1e-3, 7)
    assert np.array_equal(vis.cpu().numpy().view(U), w4[0]) and np.array_equal(msk.cpu().numpy().view(U), w4[1]) and np.array_equal(bits(bnt.cpu().numpy()), bits(w4[2]))
    g.close()
