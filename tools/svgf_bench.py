"""Variance-guided spatiotemporal filtering (tyr_svgf): its time on C3 at 1080p next to tyr_temporal + tyr_denoise, and its
quality on tools/temporal_bench.py's panning Cornell sequence against temporal -> denoise, with the grid the defaults come from.

    python tools/svgf_bench.py [--calls 200] [--out profiles/svgf_bench_c3.json]

Time: C3 (1920 x 1080, the 1 M-triangle height field) as tools/temporal_bench.py sets it up: 1-spp tyr_render_aov guides at a
camera moved by 3 pan steps, tyr_render_motion against the scene's camera, an 8-spp accumulation buffer.  tyr_svgf with its
defaults, and tyr_temporal followed by tyr_denoise with theirs, each timed with a hipEvent pair around the call on its stream,
after warm-up, over `--calls` calls: median and spread.

Quality: temporal_bench.py's sequence (the framed Cornell view at 128 x 72, 16 frames at 1 spp of a slow pan, set_camera ->
render_aov(1) -> render_motion -> render(1) per frame).  The last frame of svgf, and of temporal -> denoise, against a 1024-spp
render at the last camera (linear rgb MSE over the pixels both saw): svgf_over_temporal_denoised is the ratio
tests/test_svgf.py bounds.  The grid runs svgf over the same rendered frames for max_history x sigma_luminance x passes."""
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
from tyrant_amd import binding  # noqa: E402

MAX_HISTORY = (4, 8, 16)
SIGMA_LUMINANCE = (1.0, 2.0, 4.0, 8.0, 16.0)
PASSES = (2, 3, 4, 5)


def timing(calls, warmup):
    g, sc, _, _ = fb.c3_renderer(steps=3)
    _, gd, mv = fb.c3_guides(g, sc)
    g.reset_accum()
    g.set_frame(1)
    g.render(fb.SPP)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    res = {}
    g.svgf(**gd, **mv, reset=True)
    res["svgf"] = fb.timed(stream, calls, warmup, lambda: g.svgf(**gd, **mv, stream=stream))
    g.temporal(**gd, **mv, reset=True)
    res["temporal_denoise"] = fb.timed(stream, calls, warmup, lambda: g.denoise(**gd, accum=g.temporal(**gd, **mv, stream=stream), stream=stream))
    res["temporal"] = fb.timed(stream, calls, warmup, lambda: g.temporal(**gd, **mv, stream=stream))
    res["denoise"] = fb.timed(stream, calls, warmup, lambda: g.denoise(**gd, stream=stream))
    torch.cuda.synchronize()
    _, var = g.svgf(**gd, **mv, want_variance=True)
    res["svgf_over_temporal_denoise"] = res["svgf"]["median_ms"] / res["temporal_denoise"]["median_ms"]
    res["variance_mean"] = float(var.mean().item())
    g.close()
    return res


def quality(frames=16, ref_spp=1024, Wq=128, Hq=72):
    sc, nodes, prims, cams = fb.pan_scene(frames)
    g = binding.Renderer(Wq, Hq, 1 << 16)
    g.load_scene(sc, nodes, prims)
    seq = [(aov, mot, torch.from_numpy(acc).to("cuda:0")) for aov, mot, acc in fb.pan_frames(g, cams)]
    noisy = seq[-1][2].cpu().numpy()
    seen, mse = fb.reference(noisy, fb.converged(sc, nodes, prims, cams[-1], Wq, Hq, ref_spp))
    last = seq[-1][0]
    gd = {k: last[k] for k in ("albedo", "normal", "depth")}
    for k, (aov, mot, acc) in enumerate(seq):
        out = g.temporal(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], accum=acc, reset=(k == 0))
    td_mse = mse(g.denoise(**gd, accum=out).cpu().numpy())
    den_mse = mse(g.denoise(**gd, accum=seq[-1][2]).cpu().numpy())

    def run(**kw):
        for k, (aov, mot, acc) in enumerate(seq):
            out, var = g.svgf(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], accum=acc, reset=(k == 0), want_variance=True, **kw)
        s = mse(out.cpu().numpy())
        v = var.cpu().numpy().reshape(-1)
        return {"svgf_mse": s, "svgf_over_temporal_denoised": s / td_mse, "svgf_over_denoised": s / den_mse, "mean_variance": float(v[seen].mean())}

    grid = [dict(max_history=mh, sigma_luminance=sl, passes=p, **run(max_history=mh, sigma_luminance=sl, passes=p)) for mh in MAX_HISTORY for sl in SIGMA_LUMINANCE for p in PASSES]
    best = min(grid, key=lambda x: x["svgf_mse"])
    res = {"workload": f"cornell_box at FRAMED_CAMERA, {Wq}x{Hq}, {frames} frames at 1 spp of a pan (0.4 units, 0.002 rad per frame), recipe render_aov -> render_motion -> render -> svgf, and -> temporal -> denoise; last frame against {ref_spp} spp; linear rgb MSE",
           "noisy_mse": mse(noisy / np.maximum(noisy[:, 3:], 1)), "denoised_mse": den_mse, "temporal_denoised_mse": td_mse,
           "defaults": {"max_history": binding.SVGF_MAX_HISTORY, "depth_tolerance": binding.SVGF_DEPTH_TOLERANCE, "normal_cos": binding.SVGF_NORMAL_COS, "passes": binding.SVGF_PASSES,
                        "sigma_luminance": binding.SVGF_SIGMA_LUMINANCE, "sigma_depth": binding.SVGF_SIGMA_DEPTH, "normal_power_log2": binding.SVGF_NORMAL_POWER_LOG2}}
    res.update(run())
    res["grid_best"] = {k: best[k] for k in ("max_history", "sigma_luminance", "passes", "svgf_mse", "svgf_over_temporal_denoised")}
    res["grid"] = grid
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf_bench_c3.json"))
    args = ap.parse_args()
    t0 = time.perf_counter()
    res = {"workload": "C3: mesh_scene(706), 1920x1080; render_aov(1) at a camera moved by 3 pan steps, render_motion against the scene's camera, an 8-spp accumulation; tyr_svgf, tyr_temporal and tyr_denoise with their defaults"}
    res["timing"] = timing(args.calls, args.warmup)
    if not args.no_quality:
        res["quality"] = quality()
    res["device"] = torch.cuda.get_device_name(0)
    res["wall_s"] = time.perf_counter() - t0
    print(json.dumps({k: v for k, v in res.items() if k != "quality"}, indent=1))
    if "quality" in res:
        print(json.dumps({k: v for k, v in res["quality"].items() if k != "grid"}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
