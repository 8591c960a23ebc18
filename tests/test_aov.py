"""First-hit AOV buffers for denoisers (tyr_render_aov, hip/aov.hip; Renderer.render_aov): per pixel the average albedo and
face-forwarded normal of spp camera rays, their average hit distance and sample 0's identity.  Sample s of local pixel p is
k_primary's camera ray for ticket s * P + p from an empty queue, traced as extend traces it (intersect_scene).

CPU: what the compiler made of the kernel (make asm).  GPU: the definition against the oracle's first wavefront (begin,
primary, extend) on four scenes and three sample counts, bit for bit; another frame and a sharded ctx against the staged
export; C3's tree at full size against tyr_query_closest on the oracle's camera rays; isolation from the render state;
argument checks, partial outputs and streams; the example's PFM guides."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits, built_scene
from aov_ref import VERY_FAR, assert_aov_equal, expected_aov, first_wavefront, flags_of  # noqa: F401 (other modules take them from here)
from kernel_resources import kernel_resources

CSRC = os.path.join(ROOT, "tyrant_amd", "csrc")
LDS_PER_CU, LDS_GRANULE = 163840, 1280
SENTINEL = -7.25


# ---- CPU: resources of the AOV kernel ----------------------------------------------------------------------------------
def test_aov_kernel_keeps_registers_and_lds_in_budget():
    """no vector spills; scratch no larger than the LdsStack's private spill arrays; LDS and registers that admit the five
    blocks per CU its __launch_bounds__ plans for (as k_query_closest)"""
    res = kernel_resources("aov")
    names = [n for n in res if "k_render_aov" in n]
    assert len(names) == 1, list(res)
    k = res[names[0]]
    assert k["VGPRs Spill"] == 0, k
    assert k["ScratchSize [bytes/lane]"] <= (64 - 12) * 8 + 16, k
    assert k["Occupancy [waves/SIMD]"] >= 5, k
    per_block = -(-k["LDS Size [bytes/block]"] // LDS_GRANULE) * LDS_GRANULE
    assert LDS_PER_CU // per_block >= 5, k


# ---- the definition, restated from a queue of first-wavefront records --------------------------------------------------
def aov_into(hip, g, spp, fill=SENTINEL, which=("albedo", "normal", "depth", "prim", "geom"), stream=None):
    """tyr_render_aov into buffers pre-filled with `fill`: (status, dict of numpy arrays, flattened per pixel)"""
    import torch

    dev = torch.device("cuda", g.device)
    shapes = {"albedo": (g.H * g.W, 3), "normal": (g.H * g.W, 3), "depth": (g.H * g.W,), "prim": (g.H * g.W,), "geom": (g.H * g.W,)}
    bufs = {k: torch.full(shapes[k], fill, dtype=torch.float32 if k in ("albedo", "normal", "depth") else torch.int32, device=dev) for k in shapes}
    out = hip.AovOut(*(bufs[k].data_ptr() if k in which else None for k in ("albedo", "normal", "depth", "prim", "geom")))
    s = stream if stream is not None else torch.cuda.current_stream(g.device)
    torch.cuda.synchronize(g.device)
    rc = g.L.tyr_render_aov(g.h, spp, C.byref(out), s.cuda_stream if s.cuda_stream else None)
    torch.cuda.synchronize(g.device)
    return rc, {k: v.cpu().numpy() for k, v in bufs.items()}


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell36", "cornell_colored", "glass_dof48", "mesh128"])
def test_aov_equals_the_oracle_first_wavefront(orc, hip, name):
    """the definition: the oracle's begin / primary / extend at frame 1 with queue_size = spp * W * H gives every sample's
    record in ticket order; the expected AOVs built from them equal render_aov bit for bit (spp 1, 3, 8)"""
    sc, nodes, prims = built_scene(name)
    W, H = 96, 64
    flags = flags_of(sc)
    g = hip.Renderer(W, H, 4096, flags=flags)
    g.load_scene(sc, nodes, prims)
    spheres = np.ascontiguousarray(sc.spheres)
    geoms = set()
    for spp in (1, 3, 8):
        o = orc.Oracle(W, H, spp * W * H, flags=flags & 25)
        o.load_scene(sc, nodes, prims)
        q = first_wavefront(o, spp * W * H)
        o.close()
        pix, want = expected_aov(hip, q, sc, prims, spheres, spp, W, H, sc.triangle_colors)
        rc, got = aov_into(hip, g, spp)
        assert rc == 0, rc
        assert_aov_equal(got, pix, want, f"{name} spp {spp}")
        geoms |= set(np.unique(want["geom"]).tolist())
        res = g.render_aov(spp)  # the Python entry point: (H, W[, 3]) tensors of the same values
        assert np.array_equal(bits(res["albedo"].cpu().numpy().reshape(-1, 3)[pix]), bits(want["albedo"]))
        assert np.array_equal(res["prim"].cpu().numpy().reshape(-1)[pix], want["prim"])
    assert 1 in geoms and (name == "mesh128" or 0 in geoms), geoms
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_aov_at_another_frame_and_on_a_shard(orc, hip):
    """set_frame(7): the GPU's own staged first wavefront at that frame (pinned to the oracle by the staged-stage tests); a
    ctx with nranks = 2, rank = 1 against an oracle ctx of that rank -- and the other rank's rows keep their contents"""
    sc, nodes, prims = built_scene("glass_dof48")
    W, H, spp = 96, 64, 3
    spheres = np.ascontiguousarray(sc.spheres)
    g = hip.Renderer(W, H, spp * W * H)
    g.load_scene(sc, nodes, prims)
    g.set_tuning(retire_sky=0)
    g.set_frame(7)
    rc, got = aov_into(hip, g, spp)
    assert rc == 0 and g.counters()["frame"] == 7
    q = first_wavefront(g, spp * W * H)
    pix, want = expected_aov(hip, q, sc, prims, spheres, spp, W, H, False)
    assert_aov_equal(got, pix, want, "frame 7")
    g.close()

    h = hip.Renderer(W, H, 4096, rank=1, nranks=2)
    h.load_scene(sc, nodes, prims)
    rc, got = aov_into(hip, h, spp)
    assert rc == 0
    o = orc.Oracle(W, H, spp * W * (H // 2), rank=1, nranks=2)
    o.load_scene(sc, nodes, prims)
    q = first_wavefront(o, spp * W * (H // 2))
    o.close()
    pix, want = expected_aov(hip, q, sc, prims, spheres, spp, W, H, False)
    assert np.all(pix // W % 2 == 1)
    assert_aov_equal(got, pix, want, "rank 1 of 2")
    rows = np.arange(H * W) // W
    assert np.all(got["depth"][rows % 2 == 0] == np.float32(SENTINEL)) and np.all(got["prim"][rows % 2 == 0] == int(SENTINEL))
    assert np.all(got["albedo"][rows % 2 == 0] == np.float32(SENTINEL))
    h.close()


@pytest.mark.gpu
def test_aov_on_c3_at_full_size(orc, hip):
    """C3's 1 M-triangle tree at 1920 x 1080, spp 1: the oracle's camera rays (stage primary) through tyr_query_closest with
    the spheres give the same ids and depth"""
    sc, nodes, prims = built_scene("mesh706")
    W, H = 1920, 1080
    o = orc.Oracle(W, H, W * H)
    o.load_scene(sc, nodes, prims)
    o.stage("begin")
    o.stage("primary")
    q = o.ray_queue(0, W * H)
    o.close()
    g = hip.Renderer(W, H, 1 << 16)
    g.load_scene(sc, nodes, prims)
    t, prim, geom, _ = (x.cpu().numpy() for x in g.query_closest(q["origin"], q["direction"], spheres=True))
    res = g.render_aov(1, albedo=False, normal=False)
    pix = q["index"]
    assert np.array_equal(res["prim"].cpu().numpy().reshape(-1)[pix], prim)
    assert np.array_equal(res["geom"].cpu().numpy().reshape(-1)[pix], geom)
    assert np.array_equal(bits(res["depth"].cpu().numpy().reshape(-1)[pix]), bits(t))
    assert (geom == 1).sum() > W * H // 20 and (geom == -1).sum() > W * H // 10 and (geom == 0).sum() > 0
    assert g.query_error() == 0
    g.close()


@pytest.mark.gpu
def test_aov_leaves_the_render_state_alone(orc, hip):
    """counters, frame, accumulation and both queue exports are the same before and after; a render after it equals the same
    render without it (the same counters and sample counts, radiance up to the order of the accumulation's atomics); a refit
    issued right after it waits for it"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    W, H, N = 96, 64, 8192

    def ctx(flags=0):
        g = hip.Renderer(W, H, N, flags=flags)
        g.load_scene(sc, nodes, prims)
        return g

    a, b = ctx(), ctx()
    for g in (a, b):
        g.render(1, 2)  # mid-render: survivors in the queue
    before = (a.counters(), a.blit_buffer(), a.ray_queue(0), a.ray_queue(1))
    a.render_aov(3)
    after = (a.counters(), a.blit_buffer(), a.ray_queue(0), a.ray_queue(1))
    assert before[0] == after[0]
    for x, y in zip(before[1:], after[1:]):
        assert x.tobytes() == y.tobytes()
    a.render(2)
    b.render(2)
    assert a.counters() == b.counters()
    ba, bb = a.blit_buffer(), b.blit_buffer()  # (the accumulation's float atomics land in any order: smoke()'s tolerance)
    assert np.array_equal(ba[:, 3], bb[:, 3]) and np.allclose(ba[:, :3], bb[:, :3], rtol=1e-5, atol=1e-6)
    a.close(), b.close()

    r = ctx(flags=64)  # TYR_FLAG_REFIT
    want = r.render_aov(8)
    dev = torch.device("cuda", 0)
    bufs = {k: torch.zeros_like(v) for k, v in want.items()}
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    out = hip.AovOut(*(bufs[k].data_ptr() for k in ("albedo", "normal", "depth", "prim", "geom")))
    assert r.L.tyr_render_aov(r.h, 8, C.byref(out), side.cuda_stream) == 0
    r.refit(prims)  # the same records: waits for the pass on `side` first
    torch.cuda.synchronize(dev)
    for k in want:
        assert torch.equal(bufs[k], want[k]), k
    r.close()


@pytest.mark.gpu
def test_aov_arguments_partial_outputs_and_streams(orc, hip):
    """NULL out, all-NULL outputs, spp 0, spp * P >= 2^32 and no scene return their status; an output left NULL is not
    written; a side stream gives the same answer"""
    import torch

    sc, nodes, prims = built_scene("cornell36")
    W, H = 64, 48
    g = hip.Renderer(W, H, 4096)
    dev = torch.device("cuda", 0)
    buf = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    one = hip.AovOut(buf.data_ptr(), None, None, None, None)
    assert g.L.tyr_render_aov(g.h, 1, C.byref(one), None) == hip.TYR_ERR_NO_SCENE
    g.load_scene(sc, nodes, prims)
    assert g.L.tyr_render_aov(g.h, 1, None, None) == hip.TYR_ERR_INVALID
    assert g.L.tyr_render_aov(g.h, 1, C.byref(hip.AovOut()), None) == hip.TYR_ERR_INVALID
    assert g.L.tyr_render_aov(g.h, 0, C.byref(one), None) == hip.TYR_ERR_INVALID
    big = (1 << 32) // (W * H) + 1
    assert g.L.tyr_render_aov(g.h, big, C.byref(one), None) == hip.TYR_ERR_INVALID
    assert g.L.tyr_render_aov(None, 1, C.byref(one), None) == hip.TYR_ERR_INVALID
    full = aov_into(hip, g, 3)[1]
    for which in (("albedo",), ("normal", "prim"), ("depth", "geom")):
        rc, part = aov_into(hip, g, 3, which=which)
        assert rc == 0
        for k in part:
            if k in which:
                assert part[k].tobytes() == full[k].tobytes(), (which, k)
            else:
                assert np.all(part[k] == (np.float32(SENTINEL) if part[k].dtype == np.float32 else int(SENTINEL))), (which, k)
    side = torch.cuda.Stream(dev)
    rc, on_side = aov_into(hip, g, 3, stream=side)
    assert rc == 0
    for k in full:
        assert on_side[k].tobytes() == full[k].tobytes(), k
    res = g.render_aov(3, stream=side)
    assert set(res) == {"albedo", "normal", "depth", "prim", "geom"} and tuple(res["normal"].shape) == (H, W, 3)
    assert np.array_equal(bits(res["depth"].cpu().numpy().reshape(-1)), bits(full["depth"]))
    assert set(g.render_aov(1, albedo=False, normal=False, depth=False)) == {"prim", "geom"}
    assert g.query_error() == 0
    g.close()


def read_pfm(path):
    with open(path, "rb") as f:
        data = f.read()
    parts, pos = [], 0
    for _ in range(3):
        end = data.index(b"\n", pos)
        parts.append(data[pos:end].decode().strip())
        pos = end + 1
    w, h = map(int, parts[1].split())
    scale = float(parts[2])
    px = np.frombuffer(data[pos:], dtype="<f4" if scale < 0 else ">f4").astype(np.float32)
    return parts[0], w, h, px


@pytest.mark.gpu
def test_example_writes_aov_guides(hip, tmp_path):
    """render_main with the AOV prefix writes <prefix>.albedo.pfm and <prefix>.normal.pfm of W x H equal to
    Renderer.render_aov(1) on the same scene, camera and frame; without it, only the image it always wrote"""
    from tyrant_amd import binding

    exe = os.path.join(ROOT, "tyrant_amd", "bin", "render_main")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, "example"], check=True)
    outdir = str(tmp_path)
    ply = os.path.join(outdir, "scene.ply")
    n = 16
    xs = np.linspace(-80.0, 80.0, n + 1)
    verts = [(x, y, -18.0 + 6.0 * np.sin(0.09 * x) * np.cos(0.08 * y)) for y in xs for x in xs]
    faces = [(j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i) for j in range(n) for i in range(n)]
    with open(ply, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\nelement face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
        f.write("".join(f"{x:.6f} {y:.6f} {z:.6f}\n" for x, y, z in verts))
        f.write("".join(f"4 {a} {b} {c} {d}\n" for a, b, c, d in faces))
    img = os.path.join(outdir, "img.ppm")
    p = subprocess.run([exe, "0", "2", img, ply], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert sorted(os.listdir(outdir)) == ["img.ppm", "scene.ply"]
    prefix = os.path.join(outdir, "guides")
    p = subprocess.run([exe, "0", "2", img, ply, prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    W, H = 640, 360
    tris = binding.load_ply(ply)
    nodes, prims = binding.bvh_build(tris)
    g = hip.Renderer(W, H, 262144)
    g.upload(nodes, prims)
    cam = type("Cam", (), {})()
    cam.position, cam.direction, cam.up = (0.0, -250.0, 95.0), binding.camera_update(0.0, -0.273), (0.0, 0.0, 1.0)
    cam.focalDistance, cam.lensRadius = 1.0, 0.0
    g.set_camera(cam)
    g.set_frame(2)  # the example rendered frames 1 and 2
    res = g.render_aov(1, depth=False, ids=False)
    for k in ("albedo", "normal"):
        kind, w, h, px = read_pfm(f"{prefix}.{k}.pfm")
        assert (w, h) == (W, H), (k, w, h)
        ch = 3 if kind == "PF" else 1
        got = px.reshape(h, w, ch)
        want = res[k].cpu().numpy()
        assert np.array_equal(bits(got[::-1]), bits(want)), k  # (PFM rows run bottom to top)
    g.close()
