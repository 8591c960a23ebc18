"""Motion vectors and temporal reprojection (tyr_render_motion, tyr_temporal): their time on C3 at 1080p next to the 8-spp
render and tyr_denoise, and the quality of the per-frame recipe on a panning Cornell sequence.

    python tools/temporal_bench.py [--calls 200] [--out profiles/temporal_bench_c3.json]

Time: C3 (1920 x 1080, the 1 M-triangle height field); 1-spp tyr_render_aov guides at a camera moved from the scene's, and
tyr_render_motion against the scene's camera; tyr_temporal with the defaults on an 8-spp render's accumulation buffer, and
tyr_denoise with its defaults on the same inputs.  Each call is timed with a hipEvent pair around it on its stream, after
warm-up, over `--calls` calls: median and spread.  The render's time is a host clock around render(8) (it returns once the
stream is idle).

Quality: the framed Cornell view (scenes.FRAMED_CAMERA) at 128 x 72, 16 frames at 1 spp of a slow pan (0.4 units along x
and 0.002 rad about z per frame), each frame through the recipe set_camera -> render_aov(1) -> render_motion -> render(1) ->
temporal -> denoise.  The last frame is compared with a 1024-spp render at the last camera (linear rgb MSE over the pixels
both saw): temporal over the last noisy frame, temporal + denoise over denoise alone -- the ratios tests/test_temporal.py
bounds -- for the defaults and a small grid of max_history and depth_tolerance over the same rendered frames."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import frame_bench_common as fb  # noqa: E402  (torch before the library: one HIP runtime in the process)
import torch  # noqa: E402
from tyrant_amd import binding  # noqa: E402

MAX_HISTORY = (4, 8, 16, 32)
DEPTH_TOLERANCE = (0.02, 0.05, 0.1)


def timing(calls, warmup):
    g, sc, _, _ = fb.c3_renderer(steps=3)
    render = fb.timed_renders(g)
    aov, gd, mv = fb.c3_guides(g, sc)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    res = {}
    res["render_motion"] = fb.timed(stream, calls, warmup, lambda: g.render_motion(aov["prim"], aov["geom"], sc.camera, stream=stream))
    g.temporal(**gd, **mv, reset=True)
    res["temporal"] = fb.timed(stream, calls, warmup, lambda: g.temporal(**gd, **mv, stream=stream))
    res["denoise"] = fb.timed(stream, calls, warmup, lambda: g.denoise(**gd, stream=stream))
    torch.cuda.synchronize()
    _, ln = g.temporal(**gd, **mv, want_history_len=True)
    res["history_len_gt1_fraction"] = float((ln.cpu().numpy() > 1).mean())
    res["render_8spp"] = render
    g.close()
    return res


def quality(frames=16, ref_spp=1024, Wq=128, Hq=72):
    sc, nodes, prims, cams = fb.pan_scene(frames)
    g = binding.Renderer(Wq, Hq, 1 << 16)
    g.load_scene(sc, nodes, prims)
    seq = [(aov, mot, torch.from_numpy(acc).to("cuda:0")) for aov, mot, acc in fb.pan_frames(g, cams)]
    noisy = seq[-1][2].cpu().numpy()
    _, mse = fb.reference(noisy, fb.converged(sc, nodes, prims, cams[-1], Wq, Hq, ref_spp))
    last = seq[-1][0]
    gd = {k: last[k] for k in ("albedo", "normal", "depth")}
    noisy_mse = mse(noisy[:, :3] / np.maximum(noisy[:, 3:], 1))
    den_mse = mse(g.denoise(**gd, accum=seq[-1][2]).cpu().numpy().reshape(-1, 4))

    def run(**kw):
        for k, (aov, mot, acc) in enumerate(seq):
            out, ln = g.temporal(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], accum=acc, reset=(k == 0), want_history_len=True, **kw)
        den = g.denoise(**gd, accum=out)
        t, d = mse(out.cpu().numpy().reshape(-1, 4)), mse(den.cpu().numpy().reshape(-1, 4))
        return {"temporal_mse": t, "temporal_denoised_mse": d, "temporal_over_noisy": t / noisy_mse, "temporal_denoised_over_denoised": d / den_mse,
                "mean_history_len": float(ln.cpu().numpy()[ln.cpu().numpy() > 0].mean())}

    grid = [dict(max_history=mh, depth_tolerance=dt, **run(max_history=mh, depth_tolerance=dt)) for mh in MAX_HISTORY for dt in DEPTH_TOLERANCE]
    res = {"workload": f"cornell_box at FRAMED_CAMERA, {Wq}x{Hq}, {frames} frames at 1 spp of a pan (0.4 units, 0.002 rad per frame), recipe render_aov -> render_motion -> render -> temporal -> denoise; last frame against {ref_spp} spp; linear rgb MSE",
           "noisy_mse": noisy_mse, "denoised_mse": den_mse,
           "defaults": {"max_history": binding.TEMPORAL_MAX_HISTORY, "depth_tolerance": binding.TEMPORAL_DEPTH_TOLERANCE, "normal_cos": binding.TEMPORAL_NORMAL_COS}}
    res.update(run())
    res["grid"] = grid
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench_c3.json"))
    args = ap.parse_args()
    res = {"workload": "C3: mesh_scene(706), 1920x1080; render_aov(1) at a camera moved by 3 pan steps, render_motion against the scene's camera; tyr_temporal and tyr_denoise with the defaults"}
    res["timing"] = timing(args.calls, args.warmup)
    if not args.no_quality:
        res["quality"] = quality()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
