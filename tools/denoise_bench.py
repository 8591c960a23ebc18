"""The a-trous denoiser (tyr_denoise): its time on C3 at 1080p next to the 8-spp render it filters, and its quality on the
Cornell box, from which its default sigmas were chosen.

    python tools/denoise_bench.py [--calls 200] [--out profiles/denoise_bench_c3.json] [--kernel-stats STATS_CSV]

Time: C3 (1920 x 1080, the 1 M-triangle height field), an 8-spp render's accumulation buffer and 8-spp tyr_render_aov guides
at the render's starting frame; tyr_denoise with the defaults (5 passes), linear and TYR_DENOISE_RESOLVE, each timed with a
hipEvent pair around the call on its stream, after warm-up, over `--calls` calls: median and spread.  The render's time is a
host clock around render(8) (it returns once the stream is idle).  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats`; --kernel-stats merges its kernel_stats.csv rows of the denoise kernels into the output.

Quality: Cornell at 256 x 256, 4 spp, guides from tyr_render_aov(4) at the render's starting frame; the MSE of the linear rgb
against a 2048-spp render of the same view, denoised over noisy, for a grid of (sigma_color, sigma_depth) at 5 passes and
normal power 2^7.  The ratio falls as sigma_color grows (the colour term matters less and less on the box's smooth walls);
the defaults are the smallest sigma_color whose best ratio is within 5 % of the grid's best, with its best sigma_depth, so
that the colour term still stops the filter at strong contrasts."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import frame_bench_common as fb  # noqa: E402  (torch before the library: one HIP runtime in the process)
import torch  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402

SIGMA_COLOR = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
SIGMA_DEPTH = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)


def guides(aov):
    return {k: aov[k] for k in ("albedo", "normal", "depth")}


def timing(calls, warmup):
    g, _, _, _ = fb.c3_renderer()
    aov = g.render_aov(fb.SPP, ids=False)
    render = fb.timed_renders(g)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    res = {}
    for resolve in (False, True):
        res["resolve" if resolve else "linear"] = fb.timed(stream, calls, warmup, lambda: g.denoise(**guides(aov), resolve=resolve, stream=stream))
    acc = g.blit_buffer()
    z = aov["depth"].cpu().numpy().reshape(-1)
    res["valid_pixel_fraction"] = float(((acc[:, 3] > 0) & (z < 1e20)).mean())
    res["render_8spp"] = render
    g.close()
    return res


def quality():
    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)
    Wq = Hq = 256
    g = binding.Renderer(Wq, Hq, 1 << 18)
    g.load_scene(sc, nodes, prims)
    aov = g.render_aov(4, ids=False)
    g.render(4)
    noisy = g.blit_buffer()
    _, mse = fb.reference(noisy, fb.converged(sc, nodes, prims, None, Wq, Hq, 2048, queue=1 << 20))
    noisy_mse = mse(noisy[:, :3] / np.maximum(noisy[:, 3:], 1))
    grid = []
    for sc_ in SIGMA_COLOR:
        for sd in SIGMA_DEPTH:
            out = g.denoise(**guides(aov), sigma_color=sc_, sigma_depth=sd).cpu().numpy()
            grid.append({"sigma_color": sc_, "sigma_depth": sd, "mse": mse(out), "ratio": mse(out) / noisy_mse})
    out = g.denoise(**guides(aov)).cpu().numpy()
    g.close()
    best = min(grid, key=lambda e: e["ratio"])
    return {"workload": "cornell_box, 256x256, 4 spp (guides: render_aov(4) at frame 1) against 2048 spp; linear rgb MSE", "noisy_mse": noisy_mse,
            "grid": grid, "best": best,
            "defaults": {"passes": binding.DENOISE_PASSES, "sigma_color": binding.DENOISE_SIGMA_COLOR, "sigma_depth": binding.DENOISE_SIGMA_DEPTH,
                         "normal_power_log2": binding.DENOISE_NORMAL_POWER_LOG2},
            "ratio_at_defaults": mse(out) / noisy_mse}


def kernel_stats(path):
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            if "k_denoise" in row.get("Name", ""):
                rows.append({k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in row})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-quality", action="store_true", help="timing only (the profiler run)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool to merge")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench_c3.json"))
    args = ap.parse_args()
    res = {"workload": "C3: mesh_scene(706), 1920x1080, an 8-spp render's accumulation buffer and 8-spp render_aov guides at frame 1; tyr_denoise with the defaults"}
    res["denoise"] = timing(args.calls, args.warmup)
    res["denoise_linear_over_render_8spp"] = res["denoise"]["linear"]["median_ms"] / res["denoise"]["render_8spp"]["median_ms"]
    if not args.no_quality:
        res["quality"] = quality()
    if args.kernel_stats:
        res["kernel_stats"] = kernel_stats(args.kernel_stats)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
