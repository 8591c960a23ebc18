"""The edge-avoiding a-trous denoiser (tyr_denoise, hip/denoise.hip; Renderer.denoise): the illumination -- the frame with the
albedo divided out -- filtered in `passes` a-trous passes steered by the AOV guides, then remodulated (and optionally
tone-mapped as tyr_resolve does).

CPU: what the compiler made of the kernels (make asm); the numpy restatement (tests/denoise_ref.py) on a synthetic edge.
GPU: bit-exact against the restatement on seeded and rendered inputs; the resolve flag against tyr_resolve; quality against a
converged render; isolation from the render state; arguments, streams, sharding and the example's denoised image."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as ref
from conftest import ROOT, bits, built_scene
from kernel_resources import kernel_resources

CSRC = os.path.join(ROOT, "tyrant_amd", "csrc")
VERY_FAR = ref.VERY_FAR
# test_denoise_quality_on_cornell: the denoised frame's MSE over the noisy frame's, measured 0.037 with the defaults
# (profiles/denoise_bench_c3.json); the bound leaves room for the renders' float atomics
QUALITY_BOUND = 0.06


# ---- CPU: resources of the denoise kernels -----------------------------------------------------------------------------
def test_denoise_kernels_keep_registers_in_budget():
    """the prepare kernel and the three pass kernels (inner, last linear, last resolve): no spills, no scratch, no LDS, and
    the eight waves per SIMD that __launch_bounds__(256) without a block minimum leaves room for"""
    res = kernel_resources("denoise")
    names = [n for n in res if "k_denoise" in n]
    assert len(names) == 4, list(res)
    assert sum("k_denoise_pass" in n for n in names) == 3 and sum("k_denoise_prepare" in n for n in names) == 1, names
    for n in names:
        k = res[n]
        assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
        assert k["ScratchSize [bytes/lane]"] == 0, (n, k)
        assert k["LDS Size [bytes/block]"] == 0, (n, k)
        assert k["Occupancy [waves/SIMD]"] >= 8, (n, k)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def edge_frame(W=24, H=16):
    """two regions split at x = W / 2: normal (1, 0, 0) with illumination 0 on the left, (0, 1, 0) with illumination 1 on the
    right, albedo (0.5, 0.25, 0.75), 4 samples, depth varying; plus background pixels (A > 0, no hit, albedo 0) and pixels
    without a sample (A == 0).  Returns (accum, albedo, normal, depth, region, background, empty)."""
    y, x = np.mgrid[0:H, 0:W]
    right = x >= W // 2
    alb = np.tile(np.array([0.5, 0.25, 0.75], np.float32), (H, W, 1))
    nrm = np.where(right[..., None], np.array([0, 1, 0], np.float32), np.array([1, 0, 0], np.float32)).astype(np.float32)
    depth = (np.float32(5.0) + np.float32(0.25) * x.astype(np.float32) + np.float32(0.125) * y.astype(np.float32)).astype(np.float32)
    accum = np.zeros((H, W, 4), np.float32)
    accum[..., 3] = 4
    accum[..., :3] = np.where(right[..., None], alb * np.float32(4), np.float32(0))
    background = (x % 7 == 3) & (y % 5 == 1)
    empty = (x % 9 == 5) & (y % 4 == 2) & ~background
    depth[background] = VERY_FAR
    alb[background] = 0
    accum[background] = np.array([0.8, 1.2, 2.0, 4.0], np.float32)
    accum[empty] = 0
    flat = lambda a, c: np.ascontiguousarray(a.reshape(H * W, c) if c > 1 else a.reshape(H * W))
    return flat(accum, 4), flat(alb, 3), flat(nrm, 3), flat(depth, 1), flat(right, 1), flat(background, 1), flat(empty, 1)


def check_edge(out, accum, alb, region, background, empty):
    hit = ~background & ~empty
    assert np.all(out[empty] == 0)
    # a background pixel passes through: albedo 0 divides by 1, so the output is rgb / A
    want_bg = (accum[background, :3] / accum[background, 3:]).astype(np.float32)
    assert np.array_equal(bits(out[background, :3]), bits(want_bg))
    assert np.all(out[~empty, 3] == 1)
    assert np.all(out[hit & ~region, :3] == 0)
    assert np.array_equal(bits(out[hit & region, :3]), bits(alb[hit & region]))  # illumination exactly 1, times the albedo


def test_restatement_keeps_an_edge_exact():
    """no weight crosses the edge between the normals (1, 0, 0) and (0, 1, 0) (g = 0), so each region comes out exactly
    constant after 5 passes; background pixels pass through and A == 0 pixels give 0"""
    W, H = 24, 16
    accum, alb, nrm, depth, region, background, empty = edge_frame(W, H)
    out = ref.denoise(accum, alb, nrm, depth, W, H, passes=5)
    check_edge(out, accum, alb, region, background, empty)
    assert region.any() and (~region).any() and background.any() and empty.any()


def seeded_inputs(W, H, seed):
    """random frames with every case of the contract: background pixels, A == 0 pixels, albedo channels equal to 0, short
    averaged normals (g underflows to 0), depth discontinuities"""
    rng = np.random.default_rng(seed)
    n = W * H
    A = rng.integers(1, 9, n).astype(np.float32)
    A[rng.random(n) < 0.07] = 0
    rgb = (rng.random((n, 3)) * rng.choice([0.2, 1.0, 6.0], (n, 1)) * A[:, None]).astype(np.float32)
    accum = np.concatenate([rgb, A[:, None]], 1).astype(np.float32)
    alb = rng.random((n, 3)).astype(np.float32)
    alb[rng.random((n, 3)) < 0.1] = 0
    v = rng.normal(size=(n, 3)).astype(np.float32)
    v[:, 2] = np.abs(v[:, 2]) + 2
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    short = rng.random(n) < 0.15
    nrm[short] = (nrm[short] * np.float32(0.05)).astype(np.float32)  # |n_p . n_q| <= 0.0025: g^(2^m) underflows
    depth = (np.float32(2.0) + rng.random(n).astype(np.float32) * np.where(rng.random(n) < 0.2, np.float32(30), np.float32(0.5))).astype(np.float32)
    bg = rng.random(n) < 0.1
    depth[bg] = VERY_FAR
    alb[bg] = 0
    nrm[bg] = 0
    return accum, alb, nrm, depth


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def gpu_denoise(g, accum, alb, nrm, depth, **kw):
    out = g.denoise(dev(alb), dev(nrm), dev(depth), accum=None if accum is None else dev(accum), **kw)
    return out.cpu().numpy().reshape(-1, 4)


def assert_bits(got, want, what):
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first {np.flatnonzero(bad)[:5]}"


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(97, 61), (1, 45), (53, 1)])
def test_denoise_equals_the_restatement_on_seeded_inputs(hip, W, H):
    """passes 1..6 with default and non-default sigmas and normal powers, bit for bit"""
    g = hip.Renderer(W, H, 4096)
    accum, alb, nrm, depth = seeded_inputs(W, H, 1000 * W + H)
    settings = [dict(passes=p) for p in range(1, 7)] + [dict(passes=3, sigma_color=0.3, sigma_depth=0.02, normal_power_log2=0),
                                                        dict(passes=4, sigma_color=2.5, sigma_depth=1.5, normal_power_log2=10),
                                                        dict(passes=6, sigma_color=0.05, sigma_depth=0.5, normal_power_log2=3)]
    for kw in settings:
        want = ref.denoise(accum, alb, nrm, depth, W, H, **{("m" if k == "normal_power_log2" else k): v for k, v in kw.items()})
        got = gpu_denoise(g, accum, alb, nrm, depth, **kw)
        assert_bits(got, want, f"{W}x{H} {kw}")
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", [("cornell36", 0), ("cornell_colored", 17), ("glass_dof48", 0)])
def test_denoise_equals_the_restatement_on_renders(hip, name, flags):
    """a render at 1 and 4 spp with its tyr_render_aov guides at the render's starting frame: the ctx's own blit buffer
    (accum = NULL) and the same frame passed explicitly give the restatement's bits"""
    sc, nodes, prims = built_scene(name)
    W, H = 96, 64
    for spp in (1, 4):
        g = hip.Renderer(W, H, 8192, flags=flags)
        g.load_scene(sc, nodes, prims)
        aov = g.render_aov(spp, ids=False)
        g.render(spp)
        accum = g.blit_buffer()
        a, n, z = (aov[k].cpu().numpy() for k in ("albedo", "normal", "depth"))
        want = ref.denoise(accum, a, n, z, W, H)
        got = g.denoise(**{k: aov[k] for k in ("albedo", "normal", "depth")}).cpu().numpy().reshape(-1, 4)
        assert_bits(got, want, f"{name} spp {spp} accum=NULL")
        assert_bits(gpu_denoise(g, accum, a, n, z), want, f"{name} spp {spp}")
        valid = (accum[:, 3] > 0) & (z.reshape(-1) < VERY_FAR)
        assert valid.sum() > W * H // 2
        g.close()


@pytest.mark.gpu
def test_denoise_resolve_equals_tyr_resolve(hip):
    """TYR_DENOISE_RESOLVE: on every pixel with A > 0, tyr_resolve of the linear output bound as a second ctx's blit buffer"""
    import torch

    W, H = 97, 61
    accum, alb, nrm, depth = seeded_inputs(W, H, 7)
    g = hip.Renderer(W, H, 4096)
    lin = g.denoise(dev(alb), dev(nrm), dev(depth), accum=dev(accum), passes=4)
    tm = g.denoise(dev(alb), dev(nrm), dev(depth), accum=dev(accum), passes=4, resolve=True)
    torch.cuda.synchronize()
    r = hip.Renderer(W, H, 4096, blit_buffer=lin.data_ptr())
    want = torch.zeros_like(lin)
    torch.cuda.synchronize()  # the fill runs on torch's stream, tyr_resolve on the ctx's
    r.resolve_into(want.data_ptr())
    seen = accum[:, 3] > 0
    got, want = tm.cpu().numpy().reshape(-1, 4), want.cpu().numpy().reshape(-1, 4)
    assert_bits(got[seen], want[seen], "resolve")
    assert np.all(got[~seen] == 0)
    r.close()
    g.close()


def mse(a, b):
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    return float(d.mean())


def cornell_quality(hip, W=256, H=256, spp=4, ref_spp=2048, **kw):
    """(denoised MSE, noisy MSE) of a `spp` Cornell render against a ref_spp render of the same view, linear rgb"""
    sc, nodes, prims = built_scene("cornell36")
    g = hip.Renderer(W, H, 1 << 18)
    g.load_scene(sc, nodes, prims)
    aov = g.render_aov(spp, ids=False)
    g.render(spp)
    noisy = g.blit_buffer()
    out = g.denoise(**{k: aov[k] for k in ("albedo", "normal", "depth")}, **kw).cpu().numpy().reshape(-1, 4)
    r = hip.Renderer(W, H, 1 << 20)
    r.load_scene(sc, nodes, prims)
    r.render(ref_spp)
    conv = r.blit_buffer()
    g.close(), r.close()
    seen = (noisy[:, 3] > 0) & (conv[:, 3] > 0)
    c_ref = conv[seen, :3] / conv[seen, 3:]
    return mse(out[seen, :3], c_ref), mse(noisy[seen, :3] / noisy[seen, 3:], c_ref)


@pytest.mark.gpu
def test_denoise_quality_on_cornell(hip):
    """Cornell at 256 x 256, 4 spp, guides from tyr_render_aov(4) at the render's starting frame: the denoised frame's MSE
    against a 2048-spp render of the same view is at most QUALITY_BOUND of the noisy frame's (measured 0.037 with the
    defaults, sigma_color 32 and sigma_depth 0.02).  And the synthetic edge frame gives the restatement's exact per-region constants on the GPU."""
    den, noisy = cornell_quality(hip)
    assert noisy > 0 and den <= QUALITY_BOUND * noisy, (den, noisy, den / noisy)

    W, H = 24, 16
    accum, alb, nrm, depth, region, background, empty = edge_frame(W, H)
    g = hip.Renderer(W, H, 4096)
    out = gpu_denoise(g, accum, alb, nrm, depth)
    check_edge(out, accum, alb, region, background, empty)
    g.close()


@pytest.mark.gpu
def test_denoise_leaves_the_render_state_alone(orc, hip):
    """after a render that is not finished, tyr_denoise of the ctx's own blit buffer changes no counter, frame, budget or
    accumulation; the render then goes on to the oracle's result"""
    sc, nodes, prims = built_scene("cornell36")
    W, H, N = 96, 64, 8192
    g = hip.Renderer(W, H, N)
    g.load_scene(sc, nodes, prims)
    aov = g.render_aov(2, ids=False)
    g.render(1, 2)  # mid-render: survivors in the queue
    before = (g.counters(), g.blit_buffer(), g.ray_queue(0), g.ray_queue(1))
    out = g.denoise(**{k: aov[k] for k in ("albedo", "normal", "depth")}, resolve=True)
    out.cpu()
    after = (g.counters(), g.blit_buffer(), g.ray_queue(0), g.ray_queue(1))
    assert before[0] == after[0]
    for x, y in zip(before[1:], after[1:]):
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
def test_denoise_arguments_streams_and_shards(hip):
    """every TYR_ERR_INVALID case; two calls on two streams with different inputs each give their own bits; a sharded ctx
    gives an unsharded one's bits"""
    import torch

    W, H = 64, 48
    accum, alb, nrm, depth = seeded_inputs(W, H, 3)
    g = hip.Renderer(W, H, 4096)
    a_d, n_d, z_d, acc_d = dev(alb), dev(nrm), dev(depth), dev(accum)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    L = g.L
    full = hip.DenoiseIn(acc_d.data_ptr(), a_d.data_ptr(), n_d.data_ptr(), z_d.data_ptr())

    def call(din=full, prm=None, ctx=g.h, dst=out.data_ptr()):
        return L.tyr_denoise(ctx, None if din is None else C.byref(din), None if prm is None else C.byref(prm), dst, None)

    P = lambda passes=5, sc=1.0, sd=0.1, m=7, flags=0: hip.DenoiseParams(passes, sc, sd, m, flags)
    assert call() == 0
    torch.cuda.synchronize()
    bad = [dict(din=None), dict(ctx=None), dict(dst=None),
           dict(din=hip.DenoiseIn(acc_d.data_ptr(), None, n_d.data_ptr(), z_d.data_ptr())),
           dict(din=hip.DenoiseIn(acc_d.data_ptr(), a_d.data_ptr(), None, z_d.data_ptr())),
           dict(din=hip.DenoiseIn(acc_d.data_ptr(), a_d.data_ptr(), n_d.data_ptr(), None))]
    bad += [dict(prm=P(passes=0)), dict(prm=P(passes=9)), dict(prm=P(m=11)), dict(prm=P(flags=2))]
    for s in (0.0, -1.0, float("inf"), float("nan"), 1e-30):  # 1e-30: its square underflows, 1 / 0 is not finite
        bad += [dict(prm=P(sc=s)), dict(prm=P(sd=s))]
    bad += [dict(prm=P(passes=8, sc=1e-18))]  # kc = 1e36 is finite, kc * 4^7 is not
    for kw in bad:
        assert call(**kw) == hip.TYR_ERR_INVALID, kw
    assert call(prm=P(passes=1, sc=1e-18)) == 0  # ... and with one pass it is accepted
    assert call(prm=P(passes=8, m=10, flags=1)) == 0
    torch.cuda.synchronize()

    want = ref.denoise(accum, alb, nrm, depth, W, H)
    acc2, alb2, nrm2, depth2 = seeded_inputs(W, H, 4)
    want2 = ref.denoise(acc2, alb2, nrm2, depth2, W, H)
    s1, s2 = torch.cuda.Stream(torch.device("cuda", 0)), torch.cuda.Stream(torch.device("cuda", 0))
    ins2 = (dev(alb2), dev(nrm2), dev(depth2), dev(acc2))
    o1 = g.denoise(a_d, n_d, z_d, accum=acc_d, stream=s1)
    o2 = g.denoise(*ins2[:3], accum=ins2[3], stream=s2)
    torch.cuda.synchronize()
    assert_bits(o1.cpu().numpy().reshape(-1, 4), want, "stream 1")
    assert_bits(o2.cpu().numpy().reshape(-1, 4), want2, "stream 2")

    h = hip.Renderer(W, H, 4096, rank=1, nranks=2)
    assert_bits(h.denoise(a_d, n_d, z_d, accum=acc_d).cpu().numpy().reshape(-1, 4), want, "rank 1 of 2")
    h.close()
    g.close()


@pytest.mark.gpu
def test_example_writes_the_denoised_frame(hip, tmp_path):
    """render_main with an AOV prefix writes <prefix>.denoised.ppm, a binary PPM of the example's 640 x 360 frame"""
    exe = os.path.join(ROOT, "tyrant_amd", "bin", "render_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, "example"], check=True)
    ply = os.path.join(str(tmp_path), "scene.ply")
    with open(ply, "w") as f:  # a tilted quad of two triangles in front of the example's camera
        f.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
                "-80 -80 -20\n80 -80 -20\n80 80 -5\n-80 80 -5\n4 0 1 2 3\n")
    prefix = os.path.join(str(tmp_path), "guides")
    p = subprocess.run([exe, "0", "2", os.path.join(str(tmp_path), "img.ppm"), ply, prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    data = open(f"{prefix}.denoised.ppm", "rb").read()
    head = b"P6 640 360 255\n"
    assert data.startswith(head) and len(data) == len(head) + 640 * 360 * 3
    px = np.frombuffer(data[len(head):], np.uint8)
    assert px.max() > 0
