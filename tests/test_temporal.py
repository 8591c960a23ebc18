"""Motion vectors and temporal reprojection (tyr_render_motion / tyr_temporal, hip/temporal.hip; Renderer.render_motion and
Renderer.temporal): where each pixel's sample-0 surface was in the previous frame, and a running mean of frames over the
history reprojected from there -- the temporal half of the per-frame pipeline refit -> render_aov -> render_motion -> render
-> temporal -> denoise.

CPU: the numpy restatement's own properties (tests/temporal_ref.py); what the compiler made of the kernels (make asm).
GPU: motion against a float64 restatement from tyr_query_closest on the oracle's camera rays, for a moved camera, a refitted
box and a shard; temporal bit for bit against the restatement on seeded inputs and on a rendered sequence, fed to the
denoiser; disocclusion after a refit; quality over a panning sequence; isolation, arguments and streams."""
import ctypes as C
import dataclasses
import json
import math
import os

import numpy as np
import pytest

import denoise_ref
import temporal_ref as ref
from conftest import ROOT, bits, built_scene
from kernel_resources import kernel_resources

VERY_FAR = ref.VERY_FAR
F = np.float32
# test_temporal_quality_on_a_panning_cornell_sequence: temporal MSE over the last noisy frame's, and temporal + denoise over
# denoise alone, both against a 1024-spp render (profiles/temporal_bench_c3.json "quality": measured 0.039 and 0.56); the
# bounds leave room for the renders' float atomics
QUALITY_BOUND_TEMPORAL = 0.06
QUALITY_BOUND_DENOISED = 0.7


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------
def flat_inputs(W, H, u, depth=None, normal=None, A=1.0):
    """accum with rgb = u * A (albedo 1), unit normals (0, 0, 1) and depth 10 unless given"""
    n = W * H
    u = np.asarray(u, F).reshape(n, 3)
    accum = np.concatenate([(u * F(A)).astype(F), np.full((n, 1), A, F)], 1)
    albedo = np.ones((n, 3), F)
    normal = np.tile(np.array([0, 0, 1], F), (n, 1)) if normal is None else np.asarray(normal, F).reshape(n, 3)
    depth = np.full(n, 10.0, F) if depth is None else np.asarray(depth, F).reshape(n)
    return accum, albedo, normal, depth


def test_restatement_is_the_running_mean_without_motion():
    """zero motion, every tap accepted, max_history >= K: K frames give their mean, history length K"""
    W, H, K = 8, 6, 7
    rng = np.random.default_rng(1)
    frames = rng.random((K, W * H, 3)).astype(F)
    motion, pd = np.zeros((W * H, 2), F), np.full(W * H, 10.0, F)
    hist = None
    for k in range(K):
        accum, alb, nrm, z = flat_inputs(W, H, frames[k])
        out, ln, hist = ref.temporal(accum, alb, nrm, z, motion, pd, hist, W, H, max_history=K)
        assert np.all(ln == k + 1)
    assert np.allclose(out[:, :3], frames.astype(np.float64).mean(0), rtol=2e-6, atol=1e-7)
    assert np.all(out[:, 3] == 1)
    assert np.array_equal(bits(hist.hu[:, :3]), bits(out[:, :3]))  # albedo 1: the history is the frame


def test_restatement_moves_the_history_by_integer_motion():
    """frame 1 is frame 0 shifted by (2, -1) with motion (-2, 1): where the previous position is in the frame the output
    is exactly frame 1 with length 2 (the history holds the same values); elsewhere length 1"""
    W, H = 9, 7
    rng = np.random.default_rng(2)
    f0 = rng.random((H, W, 3)).astype(F)
    f1 = np.roll(np.roll(f0, 2, axis=1), -1, axis=0)  # f1[y, x] = f0[y + 1, x - 2]
    motion = np.tile(np.array([-2.0, 1.0], F), (W * H, 1))
    pd = np.full(W * H, 10.0, F)
    _, _, hist = ref.temporal(*flat_inputs(W, H, f0), motion, pd, None, W, H)
    out, ln, _ = ref.temporal(*flat_inputs(W, H, f1), motion, pd, hist, W, H)
    y, x = np.divmod(np.arange(W * H), W)
    inside = (x - 2 >= 0) & (y + 1 < H)
    assert inside.any() and (~inside).any()
    assert np.all(ln[inside] == 2) and np.all(ln[~inside] == 1)
    assert np.array_equal(bits(out[:, :3]), bits(f1.reshape(-1, 3)))
    # a different current frame blends half-way into the moved history
    g1 = (f1 + F(0.5)).astype(F)
    out, _, _ = ref.temporal(*flat_inputs(W, H, g1), motion, pd, hist, W, H)
    moved = f0.reshape(-1, 3)[np.where(inside, (y + 1) * W + (x - 2), 0)]
    want = (moved + F(0.5) * (g1.reshape(-1, 3) - moved).astype(F)).astype(F)
    assert np.array_equal(bits(out[inside, :3]), bits(want[inside]))


def test_restatement_restarts_on_depth_or_normal_mismatch():
    """a pixel whose expected previous depth or normal does not match the history restarts at n = 1 with the current frame;
    max_history = 1 returns the current frame everywhere"""
    W, H = 6, 5
    rng = np.random.default_rng(3)
    f0, f1 = rng.random((2, W * H, 3)).astype(F)
    motion = np.zeros((W * H, 2), F)
    pd = np.full(W * H, 10.0, F)
    _, _, hist = ref.temporal(*flat_inputs(W, H, f0), motion, pd, None, W, H)
    bad_depth = np.zeros(W * H, bool)
    bad_depth[::4] = True
    pd1 = np.where(bad_depth, F(10.0 * 1.06), pd).astype(F)  # 6 % > the 5 % tolerance
    bad_normal = np.zeros(W * H, bool)
    bad_normal[1::4] = True
    nrm = np.tile(np.array([0, 0, 1], F), (W * H, 1))
    nrm[bad_normal] = np.array([0.6, 0, 0.8], F)  # cos 0.8 < 0.9
    accum, alb, _, z = flat_inputs(W, H, f1)
    out, ln, _ = ref.temporal(accum, alb, nrm, z, motion, pd1, hist, W, H)
    restart = bad_depth | bad_normal
    assert np.all(ln[restart] == 1) and np.all(ln[~restart] == 2)
    assert np.array_equal(bits(out[restart, :3]), bits(f1[restart]))
    out, ln, _ = ref.temporal(accum, alb, nrm, z, motion, pd, hist, W, H, max_history=1)
    assert np.all(ln == 1) and np.array_equal(bits(out[:, :3]), bits(f1))


# ---- CPU: resources of the kernels -------------------------------------------------------------------------------------
def test_temporal_kernels_keep_registers_in_budget():
    """k_render_motion and k_temporal: no spills, no scratch, no LDS, eight waves per SIMD"""
    res = kernel_resources("temporal")
    names = [n for n in res if "k_render_motion" in n or "k_temporal" in n]
    assert len(names) == 2, list(res)
    for n in names:
        k = res[n]
        assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
        assert k["ScratchSize [bytes/lane]"] == 0, (n, k)
        assert k["LDS Size [bytes/block]"] == 0, (n, k)
        assert k["Occupancy [waves/SIMD]"] >= 8, (n, k)


# ---- motion: a float64 restatement -------------------------------------------------------------------------------------
def basis64(cam, W, H):
    """F, R, U of a camera by the render's rule (kernel.cu:699-700), in float64"""
    Fd = np.array(cam.direction, np.float64)
    r = np.cross(Fd, np.array(cam.up, np.float64))
    R = r / np.linalg.norm(r) * 1.5 * (W / H)
    u = np.cross(R, Fd)
    U = u / np.linalg.norm(u) * 1.5
    return np.array(cam.position, np.float64), Fd, R, U


def project64(X, cam, W, H):
    O, Fd, R, U = basis64(cam, W, H)
    w = X - O
    f = w @ Fd
    a = (w @ R) * (Fd @ Fd) / (f * (R @ R))
    b = (w @ U) * (Fd @ Fd) / (f * (U @ U))
    return (a + 0.5) * W, (0.5 - b) * H, f


def expected_motion(hip, g, q, prims, spheres, cur, prev, W, H, old=None):
    """(pixel index, motion (n, 2), prev_depth (n,), valid) of the oracle's sample-0 camera rays q, hit points from
    tyr_query_closest with the spheres on g's scene; old: the previous triangle records (X' at the same barycentrics)"""
    t, prim, geom, uv = (x.cpu().numpy() for x in g.query_closest(q["origin"], q["direction"], spheres=True))
    o, d = q["origin"].astype(np.float64), q["direction"].astype(np.float64)
    X = o + d * t.astype(np.float64)[:, None]
    tri = geom == 1
    rec = prims[prim[tri]]
    u, v = uv[tri, 0:1].astype(np.float64), uv[tri, 1:2].astype(np.float64)
    X[tri] = rec["vert"] + u * rec["e1"] + v * rec["e2"]
    Xp = X.copy()
    if old is not None:
        rp = old[prim[tri]]
        Xp[tri] = rp["vert"] + u * rp["e1"] + v * rp["e2"]
    xc, yc, fc = project64(X, cur, W, H)
    xp, yp, fp = project64(Xp, prev, W, H)
    valid = (geom >= 0) & (fc > 0) & (fp > 0)
    motion = np.stack([xp - xc, yp - yc], 1)
    pdepth = np.linalg.norm(Xp - np.array(prev.position, np.float64), axis=1)
    return q["index"], motion, pdepth, valid


def sample0_rays(orc, sc, nodes, prims, cam, W, H, rank=0, nranks=1):
    o = orc.Oracle(W, H, W * (H // nranks), rank=rank, nranks=nranks)
    o.load_scene(sc, nodes, prims)
    o.set_camera(cam)
    o.stage("begin")
    o.stage("primary")
    q = o.ray_queue(0, W * (H // nranks))
    o.close()
    return q


def moved_camera(cam, k=1.0):
    """translated by (3, 4, -2) k and turned by 0.05 k rad about z and 0.02 k rad up"""
    a, e = 0.05 * k, 0.02 * k
    dx, dy, dz = cam.direction
    c, s = math.cos(a), math.sin(a)
    d = (c * dx - s * dy, s * dx + c * dy, dz + e)
    p = tuple(x + k * y for x, y in zip(cam.position, (3.0, 4.0, -2.0)))
    return dataclasses.replace(cam, position=p, direction=d)


def check_motion(got, want, W, H, what, tol=2e-3):
    pix, m, pd, valid = want
    gm = got["motion"].cpu().numpy().reshape(-1, 2)[pix]
    gd = got["prev_depth"].cpu().numpy().reshape(-1)[pix]
    x, y = pix % W, pix // W
    px, py = x + m[:, 0], y + m[:, 1]
    inframe = valid & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    assert inframe.sum() > len(pix) // 4, (what, int(inframe.sum()))
    err = np.abs(gm[inframe] - m[inframe]).max()
    assert err <= tol, (what, err)
    assert np.allclose(gd[inframe], pd[inframe], rtol=1e-5), what
    assert np.all(gd[valid] < VERY_FAR) and np.all(gd[~valid] == VERY_FAR) and np.all(gm[~valid] == 0), what
    return inframe


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell36", "mesh706"])
def test_motion_is_zero_for_an_unchanged_view(hip, name):
    """the same camera and no moved geometry (prev_prims None or the uploaded records): motion exactly (0, 0) everywhere;
    prev_depth finite on hits (the AOV depth up to rounding for a pinhole camera) and VERY_FAR on misses"""
    import torch

    sc, nodes, prims = built_scene(name)
    W, H = 96, 64
    g = hip.Renderer(W, H, 4096)
    g.load_scene(sc, nodes, prims)
    aov = g.render_aov(1, albedo=False, normal=False)
    for pp in (None, prims, torch.from_numpy(prims.view(np.uint8).reshape(-1)).cuda()):
        res = g.render_motion(aov["prim"], aov["geom"], sc.camera, prev_prims=pp)
        m, pd = res["motion"].cpu().numpy(), res["prev_depth"].cpu().numpy()
        assert np.all(bits(m) == 0), int((bits(m) != 0).sum())
        hit = aov["geom"].cpu().numpy() >= 0
        assert hit.sum() > W * H // 10
        assert np.all(np.isfinite(pd[hit]) & (pd[hit] < VERY_FAR)) and np.all(pd[~hit] == VERY_FAR)
        if sc.camera.lensRadius == 0:
            z = aov["depth"].cpu().numpy()
            assert np.allclose(pd[hit], z[hit], rtol=1e-5)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell36", "mesh706"])
def test_motion_of_a_moved_camera_matches_float64(orc, hip, name):
    """a translated and turned camera: within 2e-3 px of the float64 restatement on every pixel whose previous position is in
    the frame, prev_depth within 1e-5; a sharded ctx (rank 1 of 2) writes its own rows alike and leaves the others"""
    import torch

    sc, nodes, prims = built_scene(name)
    W, H = 96, 64
    prev = sc.camera
    cur = moved_camera(prev, -1.0)
    g = hip.Renderer(W, H, 4096)
    g.load_scene(sc, nodes, prims)
    g.set_camera(cur)
    aov = g.render_aov(1, albedo=False, normal=False, depth=False)
    got = g.render_motion(aov["prim"], aov["geom"], prev)
    q = sample0_rays(orc, sc, nodes, prims, cur, W, H)
    want = expected_motion(hip, g, q, prims, np.ascontiguousarray(sc.spheres), cur, prev, W, H)
    inframe = check_motion(got, want, W, H, name)
    assert np.abs(want[1][inframe]).max() > 1.0  # the camera did move
    g.close()

    h = hip.Renderer(W, H, 4096, rank=1, nranks=2)
    h.load_scene(sc, nodes, prims)
    h.set_camera(cur)
    aov = h.render_aov(1, albedo=False, normal=False, depth=False)
    dev = torch.device("cuda", 0)
    mot = torch.full((H, W, 2), -7.25, dtype=torch.float32, device=dev)
    pd = torch.full((H, W), -7.25, dtype=torch.float32, device=dev)
    cam = hip.CameraC(*((C.c_float * 3)(*v) for v in (prev.position, prev.direction, prev.up)), prev.focalDistance, prev.lensRadius)
    mi = hip.MotionIn(aov["prim"].data_ptr(), aov["geom"].data_ptr(), C.cast(C.pointer(cam), C.c_void_p), None)
    mo = hip.MotionOut(mot.data_ptr(), pd.data_ptr())
    torch.cuda.synchronize()
    assert h.L.tyr_render_motion(h.h, C.byref(mi), C.byref(mo), None) == 0
    torch.cuda.synchronize()
    q = sample0_rays(orc, sc, nodes, prims, cur, W, H, rank=1, nranks=2)
    want = expected_motion(hip, h, q, prims, np.ascontiguousarray(sc.spheres), cur, prev, W, H)
    assert np.all(want[0] // W % 2 == 1)
    check_motion({"motion": mot, "prev_depth": pd}, want, W, H, name + " rank 1 of 2")
    assert np.all(mot.cpu().numpy()[0::2] == F(-7.25)) and np.all(pd.cpu().numpy()[0::2] == F(-7.25))
    h.close()


def tall_box(sc, prims):
    """build-order indices of the Cornell box's tall box (records 22..33 of the scene's triangles)"""
    want = {r.tobytes() for r in sc.triangles[22:34]}
    idx = np.array([i for i, r in enumerate(prims) if r.tobytes() in want])
    assert len(idx) == 12
    return idx


def move_box(prims, idx, by=(-8.0, 15.0, 0.0)):
    """the records idx moved by `by`: the tall box away from the camera and to the left, so that it uncovers what was behind it"""
    new = prims.copy()
    new["vert"][idx] = (new["vert"][idx] + np.array(by, F)).astype(F)
    return new


@pytest.mark.gpu
def test_motion_of_a_refitted_box_matches_float64(orc, hip):
    """the tall box moved by refit with a moved camera: with prev_prims (a device tensor) the old records' barycentric point;
    without, camera motion alone -- both within 2e-3 px of the float64 restatement"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    sc = dataclasses.replace(sc, camera=hip.scenes.FRAMED_CAMERA)
    W, H = 128, 72
    prev = sc.camera
    cur = moved_camera(prev, 0.3)
    idx = tall_box(sc, prims)
    new = move_box(prims, idx)
    g = hip.Renderer(W, H, 4096, flags=hip.TYR_FLAG_REFIT)
    g.load_scene(sc, nodes, prims)
    g.refit(new)
    g.set_camera(cur)
    aov = g.render_aov(1, albedo=False, normal=False, depth=False)
    q = sample0_rays(orc, sc, nodes, prims, cur, W, H)
    old_dev = torch.from_numpy(prims.view(np.uint8).reshape(-1)).cuda()
    got = g.render_motion(aov["prim"], aov["geom"], prev, prev_prims=old_dev)
    want = expected_motion(hip, g, q, new, np.ascontiguousarray(sc.spheres), cur, prev, W, H, old=prims)
    inframe = check_motion(got, want, W, H, "with prev_prims")
    on_box = np.isin(aov["prim"].cpu().numpy().reshape(-1)[want[0]], idx) & (aov["geom"].cpu().numpy().reshape(-1)[want[0]] == 1)
    assert (on_box & inframe).sum() > 50
    cam_only = expected_motion(hip, g, q, new, np.ascontiguousarray(sc.spheres), cur, prev, W, H)
    assert np.abs(want[1][on_box & inframe] - cam_only[1][on_box & inframe]).max() > 1.0  # the box's own motion shows
    got = g.render_motion(aov["prim"], aov["geom"], prev)
    check_motion(got, cam_only, W, H, "without prev_prims")
    g.close()


# ---- temporal: bit for bit against the restatement ---------------------------------------------------------------------
def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def seeded_frame(W, H, rng, prev_z):
    """a random frame: background pixels, A == 0 pixels, albedo channels 0, depth near the previous frame's with some jumps,
    normals near (0, 0, 1) with some turned, motions integer, fractional, out of the frame and NaN, prev_depth VERY_FAR on some"""
    n = W * H
    A = rng.integers(1, 5, n).astype(F)
    A[rng.random(n) < 0.06] = 0
    rgb = (rng.random((n, 3)) * A[:, None] * rng.choice([0.3, 1.0, 4.0], (n, 1))).astype(F)
    accum = np.concatenate([rgb, A[:, None]], 1).astype(F)
    alb = rng.random((n, 3)).astype(F)
    alb[rng.random((n, 3)) < 0.08] = 0
    v = np.tile(np.array([0, 0, 1], np.float64), (n, 1)) + rng.normal(scale=0.1, size=(n, 3))
    turned = rng.random(n) < 0.1
    v[turned] = rng.normal(size=(int(turned.sum()), 3))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    z = (prev_z * (1 + rng.normal(scale=0.02, size=n))).astype(F)
    z[rng.random(n) < 0.1] *= F(1.5)
    bg = rng.random(n) < 0.08
    z[bg] = VERY_FAR
    alb[bg] = 0
    m = rng.uniform(-2.5, 2.5, (n, 2)).astype(F)
    integer = rng.random(n) < 0.2
    m[integer] = np.round(m[integer])
    m[rng.random(n) < 0.03] = F(1e6)
    m[rng.random(n) < 0.01] = F("nan")
    pdz = (prev_z * (1 + rng.normal(scale=0.02, size=n))).astype(F)
    pdz[rng.random(n) < 0.05] = VERY_FAR
    return accum, alb, nrm, z, m, pdz


def gpu_temporal(g, ins, **kw):
    accum, alb, nrm, z, m, pdz = ins
    out, ln = g.temporal(dev(alb), dev(nrm), dev(z), dev(m), dev(pdz), accum=dev(accum), want_history_len=True, **kw)
    return out.cpu().numpy().reshape(-1, 4), ln.cpu().numpy().reshape(-1)


def assert_bits(got, want, what):
    bad = bits(got) != bits(want)
    if bad.ndim > 1:
        bad = bad.any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first {np.flatnonzero(bad)[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(61, 37), (1, 29), (40, 1)])
def test_temporal_equals_the_restatement_on_seeded_inputs(hip, W, H):
    """eight calls with different parameters, a reset in the middle: output and history length bit for bit"""
    rng = np.random.default_rng(100 * W + H)
    g = hip.Renderer(W, H, 4096)
    settings = [{}, {}, dict(max_history=4), dict(max_history=1), dict(reset=True), dict(normal_cos=-1.0, depth_tolerance=0.5),
                dict(max_history=1024, normal_cos=0.99, depth_tolerance=0.01), {}]
    z0 = (F(5) + F(20) * rng.random(W * H).astype(F)).astype(F)
    hist = None
    took = 0
    for k, kw in enumerate(settings):
        ins = seeded_frame(W, H, rng, z0)
        rkw = {kk: v for kk, v in kw.items() if kk != "reset"}
        want, want_len, nxt = ref.temporal(*ins, None if kw.get("reset") else hist, W, H, **rkw)
        got, got_len = gpu_temporal(g, ins, **kw)
        assert_bits(got, want, f"{W}x{H} call {k} {kw}")
        assert_bits(got_len, want_len, f"{W}x{H} call {k} {kw} length")
        hist = nxt
        took += int((want_len > 1).sum())
    assert took > 0
    g.close()


def pan(cam, k):
    """frame k of a slow pan: 0.4 units along x and 0.002 rad about z per frame"""
    a = 0.002 * k
    dx, dy, dz = cam.direction
    c, s = math.cos(a), math.sin(a)
    return dataclasses.replace(cam, position=(cam.position[0] + 0.4 * k, cam.position[1], cam.position[2]), direction=(c * dx - s * dy, s * dx + c * dy, dz))


def run_sequence(g, cams, spp=1, check=None):
    """the per-frame recipe for each camera: set_camera -> render_aov -> render_motion -> render -> temporal -> denoise.
    check(k, inputs, out, history length, denoised) sees every frame."""
    prev = cams[0]
    res = None
    for k, cam in enumerate(cams):
        g.set_camera(cam)
        aov = g.render_aov(spp)
        mot = g.render_motion(aov["prim"], aov["geom"], prev)
        g.render(spp)
        out, ln = g.temporal(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], reset=(k == 0), want_history_len=True)
        den = g.denoise(aov["albedo"], aov["normal"], aov["depth"], accum=out)
        if check is not None:
            check(k, aov, mot, g.blit_buffer(), out, ln, den)
        res = (aov, out, ln, den)
        prev = cam
    return res


@pytest.mark.gpu
def test_temporal_equals_the_restatement_on_a_rendered_sequence(hip):
    """five frames of a moving camera through the recipe: every frame's output and length bit for bit, and the denoiser fed
    the temporal output gives denoise_ref's bits on it"""
    sc, nodes, prims = built_scene("cornell36")
    sc = dataclasses.replace(sc, camera=hip.scenes.FRAMED_CAMERA)
    W, H = 96, 54
    g = hip.Renderer(W, H, 8192)
    g.load_scene(sc, nodes, prims)
    state = {"hist": None, "restarts": 0, "kept": 0}

    def check(k, aov, mot, accum, out, ln, den):
        a, n, z = (aov[x].cpu().numpy() for x in ("albedo", "normal", "depth"))
        m, pd = mot["motion"].cpu().numpy(), mot["prev_depth"].cpu().numpy()
        want, want_len, state["hist"] = ref.temporal(accum, a, n, z, m, pd, None if k == 0 else state["hist"], W, H)
        assert_bits(out.cpu().numpy().reshape(-1, 4), want, f"frame {k}")
        assert_bits(ln.cpu().numpy().reshape(-1), want_len, f"frame {k} length")
        assert_bits(den.cpu().numpy().reshape(-1, 4), denoise_ref.denoise(want, a, n, z, W, H), f"frame {k} denoised")
        if k:
            state["kept"] += int((want_len > 1).sum())
        assert np.any(accum[:, 3] > 0)

    run_sequence(g, [moved_camera(sc.camera, 0.1 * k) for k in range(5)], check=check)
    assert state["kept"] > 4 * W * H // 2
    g.close()


@pytest.mark.gpu
def test_temporal_disocclusion_after_a_refit(hip):
    """the tall box moves away from the camera by refit between two frames of a fixed camera: every pixel it uncovers restarts
    at n = 1; with prev_prims at least 90 % of the pixels that stay on the box keep their history, without it most restart"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    sc = dataclasses.replace(sc, camera=hip.scenes.FRAMED_CAMERA)
    W, H = 128, 72
    idx = tall_box(sc, prims)
    new = move_box(prims, idx)
    old_dev = torch.from_numpy(prims.view(np.uint8).reshape(-1)).cuda()
    lens, motion = {}, {}
    for with_prev in (True, False):
        g = hip.Renderer(W, H, 8192, flags=hip.TYR_FLAG_REFIT)
        g.load_scene(sc, nodes, prims)
        cam = sc.camera
        aov0 = g.render_aov(1)
        mot = g.render_motion(aov0["prim"], aov0["geom"], cam)
        g.render(1)
        g.temporal(aov0["albedo"], aov0["normal"], aov0["depth"], mot["motion"], mot["prev_depth"])
        g.refit(new)
        g.reset_accum()
        aov1 = g.render_aov(1)
        mot = g.render_motion(aov1["prim"], aov1["geom"], cam, prev_prims=old_dev if with_prev else None)
        g.render(1)
        _, ln = g.temporal(aov1["albedo"], aov1["normal"], aov1["depth"], mot["motion"], mot["prev_depth"], want_history_len=True)
        lens[with_prev] = ln.cpu().numpy().reshape(-1)
        box0 = np.isin(aov0["prim"].cpu().numpy().reshape(-1), idx) & (aov0["geom"].cpu().numpy().reshape(-1) == 1)
        box1 = np.isin(aov1["prim"].cpu().numpy().reshape(-1), idx) & (aov1["geom"].cpu().numpy().reshape(-1) == 1)
        hit1 = aov1["depth"].cpu().numpy().reshape(-1) < VERY_FAR
        motion[with_prev] = mot["motion"].cpu().numpy().reshape(-1, 2)
        g.close()
    uncovered = box0 & ~box1 & hit1
    assert uncovered.sum() > 20, int(uncovered.sum())
    for wp in (True, False):
        assert np.all(lens[wp][uncovered] == 1), (wp, int((lens[wp][uncovered] != 1).sum()), int(uncovered.sum()))
    # pixels on the box in both frames at their reprojected position (with prev_prims: the box's own motion)
    m = motion[True]
    assert np.all(motion[False] == 0)  # a fixed camera and no prev_prims
    pix = np.arange(W * H)
    px = np.round(pix % W + m[:, 0]).astype(np.int64)
    py = np.round(pix // W + m[:, 1]).astype(np.int64)
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    stay = box1 & inside
    stay[stay] &= box0[(py * W + px)[stay]]
    assert stay.sum() > 100, int(stay.sum())
    kept = float((lens[True][stay] > 1).mean())
    assert kept >= 0.9, kept
    restarted = float((lens[False][box1] == 1).mean())
    assert restarted > 0.5, restarted


def mse(a, b):
    return float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())


def quality_ratios(hip, W=128, H=72, frames=16, ref_spp=1024):
    """(temporal / noisy, temporal + denoise / denoise alone) MSE ratios of the last frame of a panning Cornell sequence at
    1 spp against a ref_spp render at the last camera (tools/temporal_bench.py measures the same)"""
    sc, nodes, prims = built_scene("cornell36")
    sc = dataclasses.replace(sc, camera=hip.scenes.FRAMED_CAMERA)
    cams = [pan(sc.camera, k) for k in range(frames)]
    g = hip.Renderer(W, H, 1 << 16)
    g.load_scene(sc, nodes, prims)
    aov, out, _, den_t = run_sequence(g, cams)
    noisy = g.blit_buffer()
    den = g.denoise(aov["albedo"], aov["normal"], aov["depth"]).cpu().numpy().reshape(-1, 4)
    g.close()
    r = hip.Renderer(W, H, 1 << 18)
    r.load_scene(sc, nodes, prims)
    r.set_camera(cams[-1])
    r.render(ref_spp)
    conv = r.blit_buffer()
    r.close()
    seen = (noisy[:, 3] > 0) & (conv[:, 3] > 0)
    want = conv[seen, :3].astype(np.float64) / conv[seen, 3:]
    out = out.cpu().numpy().reshape(-1, 4)
    den_t = den_t.cpu().numpy().reshape(-1, 4)
    m_noisy = mse(noisy[seen, :3] / noisy[seen, 3:], want)
    return mse(out[seen, :3], want) / m_noisy, mse(den_t[seen, :3], want) / mse(den[seen, :3], want)


@pytest.mark.gpu
def test_temporal_quality_on_a_panning_cornell_sequence(hip):
    """16 frames at 1 spp of a slowly panning framed Cornell view through the recipe: against a 1024-spp render at the last
    camera, the temporal output's MSE is at most QUALITY_BOUND_TEMPORAL of the last noisy frame's, and temporal + denoise at
    most QUALITY_BOUND_DENOISED of denoise alone"""
    t, d = quality_ratios(hip)
    assert t <= QUALITY_BOUND_TEMPORAL and d <= QUALITY_BOUND_DENOISED, (t, d)


@pytest.mark.gpu
def test_temporal_and_motion_leave_the_render_state_alone(orc, hip):
    """mid-render, both calls change no counter, frame, budget, accumulation or queue; the render then goes on to the
    oracle's result"""
    sc, nodes, prims = built_scene("cornell36")
    W, H, N = 96, 64, 8192
    g = hip.Renderer(W, H, N)
    g.load_scene(sc, nodes, prims)
    aov = g.render_aov(1)
    g.render(1, 2)  # mid-render: survivors in the queue
    before = (g.counters(), g.timings(), g.blit_buffer(), g.ray_queue(0), g.ray_queue(1))
    mot = g.render_motion(aov["prim"], aov["geom"], moved_camera(sc.camera))
    out = g.temporal(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"])
    out = g.temporal(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"])
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
def test_temporal_and_motion_arguments_and_streams(hip):
    """every TYR_ERR_* case of both calls; a call on a side stream reads inputs written on the caller's stream; two
    tyr_temporal calls on two streams of one ctx are ordered (the second sees the first's history)"""
    import torch

    W, H = 64, 48
    L = hip.lib()
    g = hip.Renderer(W, H, 4096)
    d0 = torch.device("cuda", 0)
    ids = torch.zeros((H, W), dtype=torch.int32, device=d0)
    mbuf = torch.zeros((H, W, 2), dtype=torch.float32, device=d0)
    pbuf = torch.zeros((H, W), dtype=torch.float32, device=d0)
    cam = hip.CameraC()
    cp = C.cast(C.pointer(cam), C.c_void_p)
    mi = hip.MotionIn(ids.data_ptr(), ids.data_ptr(), cp, None)
    mo = hip.MotionOut(mbuf.data_ptr(), pbuf.data_ptr())
    assert L.tyr_render_motion(g.h, C.byref(mi), C.byref(mo), None) == hip.TYR_ERR_NO_SCENE
    sc, nodes, prims = built_scene("cornell36")
    g.load_scene(sc, nodes, prims)
    assert L.tyr_render_motion(g.h, C.byref(mi), C.byref(mo), None) == 0
    bad = [(None, C.byref(mi), C.byref(mo)), (g.h, None, C.byref(mo)), (g.h, C.byref(mi), None), (g.h, C.byref(mi), C.byref(hip.MotionOut())),
           (g.h, C.byref(hip.MotionIn(None, ids.data_ptr(), cp, None)), C.byref(mo)), (g.h, C.byref(hip.MotionIn(ids.data_ptr(), None, cp, None)), C.byref(mo)),
           (g.h, C.byref(hip.MotionIn(ids.data_ptr(), ids.data_ptr(), None, None)), C.byref(mo))]
    for args in bad:
        assert L.tyr_render_motion(*args, None) == hip.TYR_ERR_INVALID

    rng = np.random.default_rng(5)
    z0 = (F(5) + F(20) * rng.random(W * H).astype(F)).astype(F)
    ins = seeded_frame(W, H, rng, z0)
    accum, alb, nrm, z, m, pdz = (dev(a) for a in ins)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device=d0)
    full = hip.TemporalIn(accum.data_ptr(), alb.data_ptr(), nrm.data_ptr(), z.data_ptr(), m.data_ptr(), pdz.data_ptr())

    def call(tin=full, prm=None, ctx=g.h, dst=out.data_ptr()):
        return L.tyr_temporal(ctx, None if tin is None else C.byref(tin), None if prm is None else C.byref(prm), dst, None, None)

    Pm = lambda mh=16, dt=0.05, nc=0.9, flags=0: hip.TemporalParams(mh, dt, nc, flags)  # noqa: E731
    assert call() == 0 and call(prm=Pm(flags=hip.TYR_TEMPORAL_RESET)) == 0
    badt = [dict(tin=None), dict(ctx=None), dict(dst=None)]
    ptrs = [accum.data_ptr(), alb.data_ptr(), nrm.data_ptr(), z.data_ptr(), m.data_ptr(), pdz.data_ptr()]
    for j in range(1, 6):
        p = list(ptrs)
        p[j] = None
        badt.append(dict(tin=hip.TemporalIn(*p)))
    badt += [dict(prm=Pm(mh=0)), dict(prm=Pm(mh=1025)), dict(prm=Pm(flags=2))]
    badt += [dict(prm=Pm(dt=v)) for v in (0.0, -1.0, float("inf"), float("nan"))]
    badt += [dict(prm=Pm(nc=v)) for v in (-1.01, 1.01, float("nan"))]
    for kw in badt:
        assert call(**kw) == hip.TYR_ERR_INVALID, kw
    assert call(prm=Pm(mh=1024, dt=1e30, nc=-1.0)) == 0 and call(prm=Pm(mh=1, nc=1.0)) == 0
    # accum NULL: the ctx's blit buffer (a ctx always has one, so TYR_ERR_NO_BUFFER cannot be reached from here)
    g.render(1)
    o, ln = g.temporal(alb, nrm, z, m, pdz, reset=True, want_history_len=True)
    w, wl, _ = ref.temporal(g.blit_buffer(), *ins[1:], None, W, H)
    assert_bits(o.cpu().numpy().reshape(-1, 4), w, "accum NULL")
    assert_bits(ln.cpu().numpy().reshape(-1), wl, "accum NULL length")

    # a side stream after work on the caller's stream; two streams in sequence share the ctx's history
    frames = [seeded_frame(W, H, rng, z0) for _ in range(3)]
    hist = None
    wants = []
    for k, f in enumerate(frames):
        w, wl, hist = ref.temporal(*f, None if k == 0 else hist, W, H)
        wants.append((w, wl))
    s1, s2 = torch.cuda.Stream(d0), torch.cuda.Stream(d0)
    got = []
    for k, f in enumerate(frames):
        busy = torch.randn(1 << 22, device=d0)
        for _ in range(8):
            busy = busy * 1.0001  # the caller's stream is busy ...
        t = [dev(a) + busy[:1] * 0 for a in f]  # ... and writes the inputs behind that work
        o, ln = g.temporal(*t[1:], accum=t[0], reset=(k == 0), want_history_len=True, stream=s1 if k % 2 == 0 else s2)
        got.append((o, ln))
    torch.cuda.synchronize()
    for k, ((o, ln), (w, wl)) in enumerate(zip(got, wants)):
        assert_bits(o.cpu().numpy().reshape(-1, 4), w, f"stream call {k}")
        assert_bits(ln.cpu().numpy().reshape(-1), wl, f"stream call {k} length")
    g.close()


def test_temporal_bench_ratios_back_the_bounds():
    """the committed measurement holds the ratios the quality bounds are taken from, with room to spare"""
    path = os.path.join(ROOT, "profiles", "temporal_bench_c3.json")
    res = json.load(open(path))
    q = res["quality"]
    assert q["temporal_over_noisy"] * 1.2 <= QUALITY_BOUND_TEMPORAL
    assert q["temporal_denoised_over_denoised"] * 1.2 <= QUALITY_BOUND_DENOISED
