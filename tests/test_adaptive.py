"""Adaptive sampling: per-pixel sample-count maps (include/tyr_c.h "Adaptive sampling").

The oracle has no mapped mode, so mapped renders are pinned from three sides: a uniform map must BE tyr_render (and so the
oracle); the pixels of the mapped camera rays must be the ticket list's (tests/adaptive_ref.py); and everything after the
camera rays must match the oracle when it is handed the GPU's post-primary queue.  The allocator is held to its numpy
restatement bit for bit."""
import numpy as np
import pytest

import adaptive_ref as ar
from conftest import bits, built_scene
from kernel_resources import kernel_resources, parse_resources


# ---- CPU: the restatements -----------------------------------------------------------------------


def test_ticket_list_of_a_uniform_map_is_the_raster_order():
    P = 37
    for k in (1, 2, 5):
        L = ar.ticket_list(np.full(P, k))
        assert np.array_equal(L, np.arange(k * P) % P)


def test_ticket_list_skips_zeros_and_orders_its_passes():
    c = np.array([2, 0, 1, 3, 0, 1])
    L = ar.ticket_list(c)
    # pass 0: c > 0, pass 1: c > 1, pass 2: c > 2
    assert L.tolist() == [0, 2, 3, 5, 0, 3, 3]
    assert L.size == c.sum()
    assert ar.ticket_list(np.zeros(9)).size == 0
    rng = np.random.default_rng(3)
    m = rng.integers(0, 6, size=200) * (rng.random(200) < 0.6)
    L = ar.ticket_list(m)
    assert np.array_equal(np.bincount(L, minlength=200), m)
    for first, n in ((0, 10), (57, 100), (L.size - 5, 5)):
        assert np.array_equal(ar.ticket_pixels(m, first, n), L[first:first + n])
    one = np.zeros(50, dtype=np.int64)
    one[7], one[9] = 65535, 2
    assert np.array_equal(ar.ticket_pixels(one, 0, 6), [7, 9, 7, 9, 7, 7])


def test_allocator_restatement_properties():
    rng = np.random.default_rng(5)
    P = 400
    err = rng.random(P).astype(np.float32) ** 3
    err[:7] = [np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, np.float32(1e-30)]
    for total, lo, hi in ((4 * P, 1, 65535), (8 * P, 2, 64), (P // 2, 1, 8), (3 * P + 17, 0, 1000)):
        c, extra = ar.allocate(err, total, lo, hi)
        E = max(total - lo * P, 0)
        assert int(extra.sum()) == E and np.all(extra >= 0)
        assert np.all(c >= min(lo, hi)) and np.all(c <= hi)
        if np.all(lo + extra <= hi):
            assert int(c.sum()) == max(total, lo * P)
    # NaN, inf and negatives count as 0: the same map as with explicit zeros
    clean = err.copy()
    clean[:4] = 0
    assert np.array_equal(ar.allocate(err, 4 * P, 1, 65535)[0], ar.allocate(clean, 4 * P, 1, 65535)[0])
    # an all-zero error: near-uniform
    c, _ = ar.allocate(np.zeros(P, np.float32), 4 * P + 3, 1, 65535)
    assert c.sum() == 4 * P + 3 and c.max() - c.min() <= 1
    # a largest error below ~3.1e-33: 2^20 / m overflows, and every usable error gets the full weight
    assert ar.weights(np.array([0.0, 1e-35, 2e-34, np.nan], np.float32)).tolist() == [0, ar.QUANT, ar.QUANT, 0]
    assert ar.weights(np.array([0.0, 0.5, 1.0], np.float32)).tolist() == [0, ar.QUANT // 2, ar.QUANT]


def test_new_kernels_have_no_spills_and_no_scratch():
    found = kernel_resources("adaptive")
    found.update(parse_resources("frame"))  # k_primary_mapped is one of primary_rays' kernels (hip/frame.hip)
    names = ("k_primary_mapped", "k_map_hist", "k_pass_count", "k_pass_scan_blocks", "k_pass_scatter", "k_pass_repeat", "k_pass_tail", "k_alloc_max", "k_alloc_scan", "k_alloc_scan_blocks", "k_alloc_map")
    for n in names:
        ks = [v for k, v in found.items() if f"{len(n)}{n}E" in k]
        assert len(ks) == 1, (n, list(found))
        r = ks[0]
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (n, r)


# ---- GPU -------------------------------------------------------------------------------------------

gpu = pytest.mark.gpu


def _flags(sc):
    return (1 if sc.triangle_materials else 0) | (8 if sc.light_list else 0) | (16 if sc.triangle_colors else 0)


def _renderer(hip, name, W, H, N, rank=0, nranks=1, flags=0):
    sc, nodes, prims = built_scene(name)
    g = hip.Renderer(W, H, N, rank=rank, nranks=nranks, flags=flags | _flags(sc))
    g.load_scene(sc, nodes, prims)
    return g


def _oracle(orc, name, W, H, N, rank=0, nranks=1):
    sc, nodes, prims = built_scene(name)
    o = orc.Oracle(W, H, N, rank=rank, nranks=nranks, flags=_flags(sc) & 25)
    o.load_scene(sc, nodes, prims)
    return o


COUNTERS = ("total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible", "start_position", "frame", "budget_remaining", "primary_ray_cnt", "shadow_ray_cnt", "n_live")


def _full(H, W, k):
    return np.full((H, W), k, dtype=np.int32)


@gpu
@pytest.mark.parametrize("name,W,H,N,spp", [("cornell36", 128, 128, 16384, 4), ("tyrant_default", 160, 96, 10000, 4), ("cornell_soup10k", 128, 72, 8192, 3), ("mesh128", 96, 96, 8192, 2), ("glass_dof48", 128, 72, 8192, 3), ("cornell_area_light", 128, 96, 8192, 4), ("cornell_colored", 128, 96, 8192, 4)])
def test_uniform_map_is_render(orc, hip, name, W, H, N, spp):
    """render_adaptive(full(k)) on one ctx == render(k) on a fresh twin: iterations, every counter, the count channel and the
    queues afterwards; rgb to 1e-5.  And the oracle's render(k) agrees."""
    a, b = _renderer(hip, name, W, H, N), _renderer(hip, name, W, H, N)
    it_a = a.render_adaptive(_full(H, W, spp))
    it_b = b.render(spp)
    assert it_a == it_b
    ka, kb = a.counters(), b.counters()
    assert ka["device_error"] == 0 and kb["device_error"] == 0
    for f in COUNTERS:
        assert ka[f] == kb[f], f
    ba, bb = a.blit_buffer(), b.blit_buffer()
    assert np.array_equal(ba[:, 3], bb[:, 3]) and np.all(ba[:, 3] == spp)
    assert np.allclose(ba[:, :3], bb[:, :3], rtol=1e-5, atol=1e-6)
    n = ka["primary_ray_cnt"]
    qa, qb = a.ray_queue(0, n), b.ray_queue(0, n)
    for f in ("origin", "direction", "direct"):
        assert np.array_equal(bits(qa[f]), bits(qb[f])), f
    nh = ka["shadow_ray_cnt"]
    sa, sb = a.shadow_queue(nh), b.shadow_queue(nh)
    assert sa.tobytes() == sb.tobytes()
    o = _oracle(orc, name, W, H, N)
    assert o.render(spp) == it_a
    ko = o.counters()
    for f in ("total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible", "start_position", "frame"):
        assert ko[f] == ka[f], f
    bo = o.blit_buffer()
    assert np.array_equal(bo[:, 3], ba[:, 3])
    assert np.allclose(ba[:, :3], bo[:, :3], rtol=1e-5, atol=1e-6)


def _assert_queue_equal(qo, qg, what):
    for f in ("origin", "direction", "direct"):
        assert np.array_equal(bits(qo[f]), bits(qg[f])), f"{what}: {f}"
    for f in ("bounces", "index", "lastSpecular"):
        assert np.array_equal(qo[f], qg[f]), f"{what}: {f}"


@gpu
@pytest.mark.parametrize("name,W,H,N", [("cornell36", 64, 64, 6000), ("glass_dof48", 96, 54, 4096), ("cornell_colored", 96, 64, 5000)])
def test_staged_uniform_map_matches_the_oracle_stage_by_stage(orc, hip, name, W, H, N):
    """set_sample_map(full(k)) through the staged API: every stage of every iteration bit for bit against the oracle's raster render"""
    o, g = _oracle(orc, name, W, H, N), _renderer(hip, name, W, H, N)
    assert g.set_sample_map(_full(H, W, 3)) == 3 * W * H
    o.set_budget(3 * W * H)
    for it in range(5):
        tag = f"{name} iteration {it}"
        o.stage("begin"), g.stage("begin")
        o.stage("primary"), g.stage("primary")
        ko, kg = o.counters(), g.counters()
        assert kg["device_error"] == 0
        for f in ("n_live", "start_position", "total_primary_rays", "total_extend_rays", "budget_remaining"):
            assert ko[f] == kg[f], (tag, f)
        n = ko["n_live"]
        _assert_queue_equal(o.ray_queue(0, n), g.ray_queue(0, n), tag + " after primary")
        o.stage("extend"), g.stage("extend")
        o.stage("shade"), g.stage("shade")
        ko, kg = o.counters(), g.counters()
        assert ko["primary_ray_cnt"] == kg["primary_ray_cnt"] and ko["shadow_ray_cnt"] == kg["shadow_ray_cnt"], tag
        _assert_queue_equal(o.ray_queue(1, ko["primary_ray_cnt"]), g.ray_queue(1, kg["primary_ray_cnt"]), tag + " survivors")
        o.stage("connect"), g.stage("connect")
        bo, bg = o.blit_buffer(), g.blit_buffer()
        assert np.array_equal(bo[:, 3], bg[:, 3]), tag
        assert np.allclose(bg[:, :3], bo[:, :3], rtol=1e-5, atol=1e-6), tag
        o.stage("end"), g.stage("end")


def _maps(H, W, rng):
    P = H * W
    rnd = rng.integers(0, 5, size=(H, W)).astype(np.int32) * (rng.random((H, W)) < 0.7)
    sparse = np.zeros((H, W), np.int32)
    sparse.reshape(-1)[rng.choice(P, size=max(P // 50, 3), replace=False)] = rng.integers(1, 9, size=max(P // 50, 3))
    one = np.zeros((H, W), np.int32)
    one[H // 3, W // 2] = 65535
    one[0, 0] = 1
    return {"random": rnd.astype(np.int32), "sparse": sparse, "one_pixel_65535": one}


@pytest.mark.parametrize("name,W,H,N", [("cornell36", 40, 24, 2000), ("glass_dof48", 48, 27, 1500)])
def test_camera_ray_restatement_matches_the_oracles_first_wavefront(orc, name, W, H, N):
    """adaptive_ref.camera_rays (kernel.cu:258-297 in numpy float32 with the oracle library's samplers) against the oracle's own
    first wavefront (raster mapping), bit for bit; glass_dof48 has a lens.  After this it is trusted for the mapped rays."""
    o = _oracle(orc, name, W, H, N)
    o.stage("begin")
    frame, start = o.counters()["frame"], o.counters()["start_position"]
    o.stage("primary")
    n = o.counters()["n_live"]
    q = o.ray_queue(0, n)
    i = np.arange(n)
    origin, direction, index = ar.camera_rays(orc.lib(), built_scene(name)[0].camera, W, H, (start + i) % (W * H), i, frame)
    assert np.array_equal(bits(q["origin"]), bits(origin))
    assert np.array_equal(bits(q["direction"]), bits(direction))
    assert np.array_equal(q["index"], index)


@gpu
@pytest.mark.parametrize("case", ["random", "sparse", "one_pixel_65535", "ragged_queue", "queue_beyond_T", "rank1of2", "odd_97x61", "odd_rank1of2"])
def test_mapped_camera_rays_and_the_oracle_after_them(orc, hip, case):
    """Staged mapped loop: after every primary launch the new records (launch index i, ticket T - b + i) are the restated camera
    rays at L's pixels -- origin, direction and pixel index bit for bit (adaptive_ref.camera_rays); the oracle, handed the GPU's
    post-primary queue (budget 0: begin, import_work_queue, primary), then agrees on the survivors and the shadow queue bit for
    bit, on the accumulation to 1e-5 and on the count channel exactly.  Odd sizes: P odd, whole frame and one shard."""
    rng = np.random.default_rng(11)
    name, W, H, N, rank, nranks = "cornell36", 48, 40, 1000, 0, 1
    key = case
    if case == "ragged_queue":
        N, key = 333, "random"
    elif case == "queue_beyond_T":
        N, key = 4096, "sparse"
    elif case == "rank1of2":
        rank, nranks, key = 1, 2, "random"
    elif case == "odd_97x61":
        name, W, H, N, key = "glass_dof48", 97, 61, 2500, "random"
    elif case == "odd_rank1of2":
        name, W, H, N, rank, nranks, key = "glass_dof48", 97, 62, 2500, 1, 2, "random"
    cam = built_scene(name)[0].camera
    m = _maps(H, W, rng)[key]
    local = ar.local_rows(m, rank, nranks)
    T = int(local.sum())
    g = _renderer(hip, name, W, H, N, rank=rank, nranks=nranks)
    o = _oracle(orc, name, W, H, N, rank=rank, nranks=nranks)
    o.set_budget(0)
    assert g.set_sample_map(m) == T
    W_ = W
    iters = 4 if case != "one_pixel_65535" else 3
    for it in range(iters):
        tag = f"{case} iteration {it}"
        g.stage("begin")
        b = g.counters()["budget_remaining"]
        surv = g.counters()["primary_ray_cnt"] if it else 0
        frame = g.counters()["frame"]
        g.stage("primary")
        kg = g.counters()
        assert kg["device_error"] == 0
        n = kg["n_live"]
        nNew = n - surv
        assert nNew == min(N - surv, b), tag
        q = g.ray_queue(0, n)
        want = ar.ticket_pixels(local, T - b, nNew)
        origin, direction, index = ar.camera_rays(orc.lib(), cam, W_, H, want, np.arange(nNew), frame, rank, nranks)
        assert np.array_equal(q["index"][surv:], index), tag + " pixels"
        assert np.array_equal(bits(q["origin"][surv:]), bits(origin)), tag + " origins"
        assert np.array_equal(bits(q["direction"][surv:]), bits(direction)), tag + " directions"
        o.stage("begin")
        o.import_work_queue(q, n)
        o.stage("primary")
        assert o.counters()["n_live"] == n, tag
        for s in ("extend", "shade"):
            o.stage(s), g.stage(s)
        ko, kg = o.counters(), g.counters()
        assert ko["primary_ray_cnt"] == kg["primary_ray_cnt"] and ko["shadow_ray_cnt"] == kg["shadow_ray_cnt"], tag
        ns, nh = ko["primary_ray_cnt"], ko["shadow_ray_cnt"]
        _assert_queue_equal(o.ray_queue(1, ns), g.ray_queue(1, ns), tag + " survivors")
        so, sg = o.shadow_queue(nh), g.shadow_queue(nh)
        for f in ("origin", "direction", "color", "closestDistance"):
            assert np.array_equal(bits(so[f]), bits(sg[f])), f"{tag} shadow {f}"
        assert np.array_equal(so["buffer_index"], sg["buffer_index"]), tag
        o.stage("connect"), g.stage("connect")
        bo, bg = o.blit_buffer(), g.blit_buffer()
        assert np.array_equal(bo[:, 3], bg[:, 3]), tag + " count channel"
        assert np.allclose(bg[:, :3], bo[:, :3], rtol=1e-5, atol=1e-6), tag
        o.stage("end"), g.stage("end")
        if n == 0:
            break


@gpu
@pytest.mark.parametrize("knobs", [{}, {"run_ahead": 0}, {"fold_prologue": 0, "scan_in_trace": 0}, {"merge_trace": 0}])
@pytest.mark.parametrize("max_iterations", [0xFFFFFFFF, 1000])
@pytest.mark.parametrize("W,H,rank,nranks", [(96, 64, 0, 1), (97, 61, 0, 1), (97, 62, 1, 2)])
def test_render_adaptive_equals_the_staged_mapped_loop(hip, knobs, max_iterations, W, H, rank, nranks):
    """merged / run-ahead / folded forms and the staged loop: the same count channel (== the map on the ctx's rows),
    counters, rgb to 1e-5; odd pixel counts, whole frame and one shard, included"""
    rng = np.random.default_rng(7)
    name, N = "tyrant_default", 3000
    m = _maps(H, W, rng)["random"]
    if nranks > 1:
        m[np.arange(H) % nranks != rank] = 0  # (rows the ctx does not own: never read, never rendered)
    a, b = _renderer(hip, name, W, H, N, rank=rank, nranks=nranks), _renderer(hip, name, W, H, N, rank=rank, nranks=nranks)
    a.set_tuning(**knobs)
    a.render_adaptive(m, max_iterations=max_iterations)
    b.set_sample_map(m)
    while True:
        b.launch_kernels()
        k = b.counters()
        if k["budget_remaining"] == 0 and k["primary_ray_cnt"] == 0:
            break
    ka, kb = a.counters(), b.counters()
    assert ka["device_error"] == 0
    for f in ("total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible", "budget_remaining"):
        assert ka[f] == kb[f], f
    ba, bb = a.blit_buffer(), b.blit_buffer()
    assert np.array_equal(ba[:, 3], m.reshape(-1).astype(np.float32))
    assert np.array_equal(ba[:, 3], bb[:, 3])
    assert np.allclose(ba[:, :3], bb[:, :3], rtol=1e-5, atol=1e-6)


@gpu
def test_full_size_render_adaptive_spends_the_map(hip):
    """1080p, an 8-spp-average map from allocate_samples: the count channel equals the map exactly"""
    W, H = 1920, 1080
    g = _renderer(hip, "tyrant_default", W, H, 1 << 21)
    g.render(1)
    e = ar.two_buffer_error(g.blit_buffer(), np.zeros((W * H, 4), np.float32)).reshape(H, W)  # one sample's brightness as a stand-in error
    m, total = g.allocate_samples(e, 8 * W * H, min_spp=1, max_spp=65535)
    m = m.cpu().numpy()
    assert total == int(m.sum()) == 8 * W * H
    g.reset_accum()
    g.render_adaptive(m)
    assert g.counters()["device_error"] == 0
    assert np.array_equal(g.blit_buffer()[:, 3], m.reshape(-1).astype(np.float32))


@gpu
@pytest.mark.parametrize("rank,nranks", [(0, 1), (1, 2)])
def test_allocator_matches_its_restatement(hip, rank, nranks):
    rng = np.random.default_rng(13 + rank)
    W, H = 64, 48
    g = hip.Renderer(W, H, 1024, rank=rank, nranks=nranks)
    P = W * H // nranks
    fields = {
        "seeded": (rng.random((H, W)) ** 4).astype(np.float32),
        "specials": np.where(rng.random((H, W)) < 0.1, np.float32(np.nan), rng.standard_normal((H, W)).astype(np.float32)),
        "zeros": np.zeros((H, W), np.float32),
        "tiny": np.where(rng.random((H, W)) < 0.2, np.float32(0), (1e-36 + rng.random((H, W)) * 1e-34).astype(np.float32)),  # 2^20 / max overflows
    }
    fields["specials"][0, :4] = [np.inf, -np.inf, 1e30, -0.0]
    for what, err in fields.items():
        for total, lo, hi in ((4 * P, 1, 65535), (P // 3, 1, 65535), (6 * P, 2, 9), (5 * P + 1, 0, 1000)):
            m, got = g.allocate_samples(err, total, min_spp=lo, max_spp=hi)
            m = m.cpu().numpy()
            want, _ = ar.allocate(ar.local_rows(err, rank, nranks), total, lo, hi)
            assert np.array_equal(ar.local_rows(m, rank, nranks), want), (what, total, lo, hi)
            assert got == int(want.sum())
            if nranks > 1:
                other = np.ones(H, bool)
                other[rank::nranks] = False
                assert not np.any(m[other]), "only the ctx's rows are written"


@gpu
def test_mapped_mode_ends_and_errors_leave_the_ctx_unchanged(hip):
    import torch

    name, W, H, N = "cornell36", 32, 32, 2048
    g = _renderer(hip, name, W, H, N)
    rng = np.random.default_rng(1)
    m = rng.integers(0, 4, size=(H, W)).astype(np.int32)
    g.render_adaptive(m)
    before = g.blit_buffer()[:, 3].copy()
    g.render(2)  # the raster mapping is back
    assert np.array_equal(g.blit_buffer()[:, 3], before + 2)
    # set_budget ends mapped mode, too
    g.set_sample_map(m)
    g.set_budget(W * H)
    c0 = g.blit_buffer()[:, 3].copy()
    while True:
        g.launch_kernels()
        k = g.counters()
        if k["budget_remaining"] == 0 and k["primary_ray_cnt"] == 0:
            break
    assert np.array_equal(g.blit_buffer()[:, 3], c0 + 1)
    # errors: the ctx keeps its budget, mode and counters
    g.set_sample_map(_full(H, W, 1))
    k0 = g.counters()
    bad = _full(H, W, 1)
    bad[3, 3] = 65536
    for what, fn in (("value above 65535", lambda: g.set_sample_map(bad)), ("render_adaptive, value above 65535", lambda: g.render_adaptive(bad))):
        with pytest.raises(hip.TyrError):
            fn()
        assert g.counters() == k0, what
    assert g.L.tyr_set_sample_map(g.h, None, None, None) == -1
    assert g.L.tyr_set_sample_map(None, torch.zeros(1, dtype=torch.int32, device=f"cuda:{g.device}").data_ptr(), None, None) == -1
    assert g.counters() == k0
    big = hip.Renderer(1024, 1024, 1024)
    kb0 = big.counters()
    with pytest.raises(hip.TyrError):
        big.set_sample_map(np.full((1024, 1024), 65535, np.int32))  # T = 2^36 - 2^20 >= 2^32
    assert big.counters() == kb0
    big.close()
    e = torch.ones((H, W), dtype=torch.float32, device="cuda")
    for prm in ((100, 5, 4), (100, 1, 0), (100, 1, 65536), (1 << 32, 1, 8)):
        with pytest.raises(hip.TyrError):
            g.allocate_samples(e, *prm)
    assert g.counters() == k0
    # the mapped budget still renders the last good map: every pixel once
    g.reset_accum()
    g.set_sample_map(_full(H, W, 1))
    while True:
        g.launch_kernels()
        k = g.counters()
        if k["budget_remaining"] == 0 and k["primary_ray_cnt"] == 0:
            break
    assert np.all(g.blit_buffer()[:, 3] == 1)
    # an all-zero map behaves like render(0) on a twin
    a, b = _renderer(hip, name, W, H, N), _renderer(hip, name, W, H, N)
    a.render(1), b.render(1)
    assert a.render_adaptive(np.zeros((H, W), np.int32)) == b.render(0)
    ka, kb = a.counters(), b.counters()
    for f in COUNTERS:
        assert ka[f] == kb[f], f
    assert np.array_equal(a.blit_buffer(), b.blit_buffer())


# the bounds are this recipe's measured ratios with margin (profiles/adaptive_bench_c3.json, "test_recipe": the 3 x 3
# box-filtered error, no pixel clamped).  With the raw two-buffer error tyrant_default does not gain (1.01 there).
QUALITY_SCENES = [("tyrant_default", 96, 64, 0.85), ("glass_dof48", 96, 54, 0.75)]


@gpu
@pytest.mark.parametrize("name,W,H,bound", QUALITY_SCENES)
def test_adaptive_beats_uniform_at_equal_samples(hip, name, W, H, bound):
    """8 spp per pixel on average both ways: uniform render(8) against 2 + 2 uniform + 4 allocated by the two-buffer error
    (3 x 3 box filter); linear-rgb MSE against a 1024-spp uniform reference.  The bound is the measured ratio with margin."""
    P = W * H
    N = 1 << 16
    g = _renderer(hip, name, W, H, N)
    g.render(1024)
    ref = g.blit_buffer()
    ref = ref[:, :3] / ref[:, 3:4]

    def mse(buf):
        return float(np.mean((buf[:, :3] / buf[:, 3:4] - ref) ** 2))

    g.set_frame(5000)
    g.reset_accum()
    g.render(8)
    uni = g.blit_buffer()
    g.set_frame(9000)
    g.reset_accum()
    g.render(2)
    a = g.blit_buffer()
    g.reset_accum()
    g.render(2)
    b = g.blit_buffer()
    g.reset_accum()
    err = ar.box3(ar.two_buffer_error(a, b).reshape(H, W))
    m, total = g.allocate_samples(err, 4 * P, min_spp=1, max_spp=65535)
    m = m.cpu().numpy()
    assert m.max() < 65535 and total == 4 * P
    g.render_adaptive(m)
    c = g.blit_buffer()
    ada = a + b + c
    assert ada[:, 3].sum() == uni[:, 3].sum() == 8 * P
    ratio = mse(ada) / mse(uni)
    print(f"{name}: adaptive / uniform MSE at 8 spp = {ratio:.3f}")
    assert ratio < bound, ratio
