"""Specular-chain guides (tyr_render_aov_chain, tyr_render_motion_chain): what they cost on C3, how much of C3 they change, and
whether the filters do better with them.

    python tools/specular_guides_bench.py [--calls 200] [--out profiles/specular_guides_bench.json]

Cost: C3 (1920 x 1080, the 1 M-triangle height field, 30 % of it mirrors) at 1 and 8 spp: tyr_render_aov next to
tyr_render_aov_chain at max_chain 0, 1, 4, 8, and tyr_render_motion next to tyr_render_motion_chain, each timed with a hipEvent
pair around the call on its stream after warm-up over `--calls` calls: median, p10, p90.  (k_render_aov's code is the parent
commit's instruction for instruction -- `make asm` before and after -- so its time here is the parent's.)

Coverage: the share of C3's pixels whose sample-0 chain has bounces, and the histogram of their number.

Quality: the mirror room (mirror_room below: Cornell walls, a mirror quad on the back and on the left wall, a glass sphere,
the two boxes) at 128 x 72 from the framed camera, panned as tests/test_temporal.py pans.  Ground truth per frame is a
1024-spp tyr_render.  Two recipes with their defaults, each with first-hit guides and with chain guides: a 4-spp still frame
through tyr_denoise, and a 16-frame 1-spp pan through motion + tyr_svgf (last frame).  Reported: the MSE with chain guides
over the MSE with first-hit guides, over the pixels with a chain and over the whole frame; the mean history length on the
chain pixels for both kinds of guides (tyr_temporal's, run with tyr_svgf's reprojection parameters: tyr_svgf applies the same
test and does not export the length); and, for the planar mirrors under a moved camera, the share of mirror pixels whose
prev_depth agrees with the previous frame's chain depth at the reprojected pixel within tyr_temporal's depth tolerance.
tests/test_specular_guides.py bounds the two chain-pixel ratios and that share by what is recorded here."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import frame_bench_common as fb  # noqa: E402  (torch before the library: one HIP runtime in the process)
import torch  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402

MAX_CHAIN = 8
VERY_FAR = np.float32(1e20)
MIN_CHAIN_SHARE = 0.2  # of the quality frame's pixels


def mirror_room():
    """Cornell walls and boxes; a mirror quad on the back wall and one on the left wall, half a unit in front of them; a glass
    sphere on the floor in front of the short box"""
    back = scenes._quad((-40, 49.5, 10), (40, 49.5, 10), (40, 49.5, 90), (-40, 49.5, 90), (0, -1, 0))
    left = scenes._quad((-49.5, -45, 10), (-49.5, 45, 10), (-49.5, 45, 90), (-49.5, -45, 90), (1, 0, 0))
    back["materialType"] = scenes.SPEC
    left["materialType"] = scenes.SPEC
    tris = np.concatenate([scenes.room_walls(), scenes._box(18.0, -12.0, 15.0, 15.0, 0.0, 30.0, -0.3), scenes._box(-16.0, 14.0, 15.0, 15.0, 0.0, 60.0, 0.3), back, left])
    spheres = scenes.cornell_spheres()
    spheres[0] = (11.0, (30.0, -38.0, 11.0), (0.02, 0.015, 0.004), (0.0, 0.0, 0.0), scenes.REFR)
    return scenes.SceneData("mirror_room", tris, spheres, scenes.FRAMED_CAMERA, triangle_materials=True)


def pan(cam, k):
    """tests/test_temporal.py's pan: 0.4 units along x and 0.002 rad about z per frame"""
    return fb.moved(cam, k)


def guides(g, spp, prev, chain):
    """the guides and motion of the ctx's camera against the camera `prev`: first-hit (chain False) or chain guides"""
    if not chain:
        aov = g.render_aov(spp)
        mot = g.render_motion(aov["prim"], aov["geom"], prev)
    else:
        aov = g.render_aov(spp, max_chain=MAX_CHAIN)
        mot = g.render_motion(aov["prim"], aov["geom"], prev, chain=aov["chain"], length0=aov["length0"])
    return aov, mot


def converged(sc, nodes, prims, cam, W, H, spp):
    return fb.converged(sc, nodes, prims, cam, W, H, spp, flags=binding.TYR_FLAG_TRIANGLE_MATERIALS)


def quality(W=128, H=72, frames=16, ref_spp=1024):
    sc = mirror_room()
    nodes, prims = binding.bvh_build(sc.triangles)
    cams = [pan(sc.camera, k) for k in range(frames)]
    g = binding.Renderer(W, H, 1 << 16, flags=binding.TYR_FLAG_TRIANGLE_MATERIALS)
    g.load_scene(sc, nodes, prims)
    res = {"workload": f"mirror_room at FRAMED_CAMERA, {W}x{H}; still: 4 spp -> denoise; pan: {frames} frames at 1 spp (0.4 units, 0.002 rad per frame) -> motion -> svgf, last frame; "
                       f"each against {ref_spp} spp; linear rgb MSE, chain guides over first-hit guides; max_chain {MAX_CHAIN}"}

    def ratios(outs, noisy, conv, on_chain):
        seen = (noisy[:, 3] > 0) & (conv[:, 3] > 0)
        want = conv[:, :3].astype(np.float64) / np.maximum(conv[:, 3:], 1)
        mse = lambda a, m: float(((a.reshape(-1, 4)[m, :3].astype(np.float64) - want[m]) ** 2).mean())  # noqa: E731
        cm = seen & on_chain
        return {"chain_pixels": int(cm.sum()), "mse_first_chain_pixels": mse(outs[False], cm), "mse_chain_chain_pixels": mse(outs[True], cm),
                "ratio_chain_pixels": mse(outs[True], cm) / mse(outs[False], cm), "ratio_frame": mse(outs[True], seen) / mse(outs[False], seen)}

    # still frame
    g.set_camera(cams[0])
    g.set_frame(1)
    g.reset_accum()
    g.render(4)
    acc = torch.from_numpy(g.blit_buffer()).to("cuda:0")
    outs = {}
    for chain in (False, True):
        g.set_frame(1)
        aov, _ = guides(g, 4, cams[0], chain)
        outs[chain] = g.denoise(aov["albedo"], aov["normal"], aov["depth"], accum=acc).cpu().numpy()
    g.set_frame(1)
    on_chain = g.render_aov(1, max_chain=MAX_CHAIN)["chain"].cpu().numpy().reshape(-1) > 0
    res["chain_share"] = float(on_chain.mean())
    assert res["chain_share"] >= MIN_CHAIN_SHARE, res["chain_share"]
    res["still"] = ratios(outs, acc.cpu().numpy().reshape(-1, 4), converged(sc, nodes, prims, cams[0], W, H, ref_spp), on_chain)

    # pan: the same rendered frames through svgf with either kind of guides
    g.set_frame(1)
    seq = []
    prev = cams[0]
    for cam in cams:
        g.set_camera(cam)
        g.reset_accum()
        both = {chain: guides(g, 1, prev, chain) for chain in (False, True)}
        g.render(1)
        seq.append((both, torch.from_numpy(g.blit_buffer()).to("cuda:0")))
        prev = cam
    outs, lens = {}, {}
    for chain in (False, True):
        for k, (both, accum) in enumerate(seq):
            aov, mot = both[chain]
            out = g.svgf(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], accum=accum, reset=(k == 0))
            # tyr_svgf does not export its history length: tyr_temporal with tyr_svgf's reprojection parameters applies the same test
            _, ln = g.temporal(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], accum=accum, max_history=binding.SVGF_MAX_HISTORY,
                               depth_tolerance=binding.SVGF_DEPTH_TOLERANCE, normal_cos=binding.SVGF_NORMAL_COS, reset=(k == 0), want_history_len=True)
        outs[chain], lens[chain] = out.cpu().numpy(), ln.cpu().numpy().reshape(-1)
    on_chain = seq[-1][0][True][0]["chain"].cpu().numpy().reshape(-1) > 0
    res["pan"] = ratios(outs, seq[-1][1].cpu().numpy().reshape(-1, 4), converged(sc, nodes, prims, cams[-1], W, H, ref_spp), on_chain)
    res["pan"]["history_len_chain_pixels"] = {"first_hit_guides": float(lens[False][on_chain].mean()), "chain_guides": float(lens[True][on_chain].mean())}
    g.close()
    res["mirror_reprojection"] = mirror_reprojection(W, H)
    return res


def mirror_reprojection(W=128, H=72, steps=8, depth_tolerance=binding.TEMPORAL_DEPTH_TOLERANCE):
    """the planar mirrors of mirror_room under a camera moved by `steps` pan steps: for the pixels whose chain is one bounce off
    a mirror triangle and whose previous position is in the frame, the share whose prev_depth agrees with the previous frame's
    chain depth at the nearest pixel there as tyr_temporal tests it: |z_prev - prev_depth| <= depth_tolerance * prev_depth"""
    sc = mirror_room()
    nodes, prims = binding.bvh_build(sc.triangles)
    g = binding.Renderer(W, H, 1 << 16, flags=binding.TYR_FLAG_TRIANGLE_MATERIALS)
    g.load_scene(sc, nodes, prims)
    prev, cur = sc.camera, pan(sc.camera, steps)
    z_prev = g.render_aov(1, max_chain=MAX_CHAIN)["depth"].cpu().numpy().reshape(-1)
    g.set_camera(cur)
    aov, mot = guides(g, 1, prev, True)
    g.close()
    first = aov["prim"].cpu().numpy().reshape(-1)
    mirror = (aov["geom"].cpu().numpy().reshape(-1) == 1) & (aov["chain"].cpu().numpy().reshape(-1) == 1)
    mirror[mirror] &= prims["materialType"][first[mirror]] == scenes.SPEC
    m, pd = mot["motion"].cpu().numpy().reshape(-1, 2), mot["prev_depth"].cpu().numpy().reshape(-1)
    pix = np.arange(W * H)
    px, py = np.round(pix % W + m[:, 0]).astype(np.int64), np.round(pix // W + m[:, 1]).astype(np.int64)
    ok = mirror & (pd < VERY_FAR) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    q = (py * W + px)[ok]
    agree = np.abs(z_prev[q] - pd[ok]) <= np.float32(depth_tolerance) * pd[ok]
    return {"steps": steps, "mirror_pixels": int(ok.sum()), "share_within_depth_tolerance": float(agree.mean())}


def timing(calls, warmup):
    g, sc, _, _ = fb.c3_renderer(steps=3, queue=1 << 16)
    g.set_frame(1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = fb.W * fb.H
    f32 = lambda k: torch.zeros(n * k, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    bufs = {"albedo": f32(3), "normal": f32(3), "depth": f32(1), "prim": i32(), "geom": i32(), "chain": i32(), "end_prim": i32(), "end_geom": i32(), "length0": f32(1), "depth_first": f32(1)}
    import ctypes as C

    out = binding.AovOut(*(bufs[k].data_ptr() for k in ("albedo", "normal", "depth", "prim", "geom")))
    ext = binding.AovChainOut(*(bufs[k].data_ptr() for k in ("chain", "end_prim", "end_geom", "length0", "depth_first")))
    res = {}
    for spp in (1, 8):
        r = {"render_aov": fb.timed(stream, calls, warmup, lambda: g.L.tyr_render_aov(g.h, spp, C.byref(out), stream.cuda_stream))}
        for mc in (0, 1, 4, 8):
            r[f"render_aov_chain_{mc}"] = fb.timed(stream, calls, warmup, lambda: g.L.tyr_render_aov_chain(g.h, spp, mc, C.byref(out), C.byref(ext), stream.cuda_stream))
            r[f"render_aov_chain_{mc}_over_render_aov"] = r[f"render_aov_chain_{mc}"]["median_ms"] / r["render_aov"]["median_ms"]
        res[f"spp{spp}"] = r
    torch.cuda.synchronize()
    aov = g.render_aov(1, max_chain=MAX_CHAIN)
    chain = aov["chain"].cpu().numpy().reshape(-1)
    res["coverage"] = {"share_chain_pixels": float((chain > 0).mean()), "histogram": np.bincount(chain, minlength=MAX_CHAIN + 1).tolist()}
    res["render_motion"] = fb.timed(stream, calls, warmup, lambda: g.render_motion(aov["prim"], aov["geom"], sc.camera, stream=stream))
    res["render_motion_chain"] = fb.timed(stream, calls, warmup, lambda: g.render_motion(aov["prim"], aov["geom"], sc.camera, chain=aov["chain"], length0=aov["length0"], stream=stream))
    res["render_motion_chain_over_render_motion"] = res["render_motion_chain"]["median_ms"] / res["render_motion"]["median_ms"]
    assert g.query_error() == 0
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specular_guides_bench.json"))
    args = ap.parse_args()
    t0 = time.perf_counter()
    res = {"workload": "C3: mesh_scene(706), 1920x1080, a camera moved by 3 pan steps; tyr_render_aov against tyr_render_aov_chain at max_chain 0, 1, 4, 8 (1 and 8 spp), tyr_render_motion against tyr_render_motion_chain"}
    if not args.no_timing:
        res["timing"] = timing(args.calls, args.warmup)
    if not args.no_quality:
        res["quality"] = quality()
    res["device"] = torch.cuda.get_device_name(0)
    res["wall_s"] = time.perf_counter() - t0
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
