"""Adaptive sampling (tyr_set_sample_map, tyr_render_adaptive, tyr_allocate_samples): what mapped mode costs, what building a
map and its ticket list costs, and what an adaptive render buys at an equal number of samples.

    python tools/adaptive_bench.py [--reps 20] [--out profiles/adaptive_bench_c3.json]

Overhead: C3 (mesh_scene(706), 1920 x 1080, queue = 8 spp of pixels) render(8) against render_adaptive(full(8)), alternated,
after warm-up, `--reps` each (wall time of the synchronous call): median and spread; and on a TYR_FLAG_PROFILE ctx the primary
stage alone inside the same two renders (k_primary against k_primary_mapped, hipEvent pairs).  Build times: set_sample_map and
allocate_samples of an 8-spp-average map at 1080p (a hipEvent pair on its stream; set_sample_map, which returns once the list is
built: wall time).
Quality (tests/test_adaptive.py's recipe): uniform render(8) against 2 + 2 uniform spp, a two-buffer error, allocate_samples(4 P)
and render_adaptive, linear-rgb MSE against a 1024-spp uniform reference, for the raw error and a 3 x 3 box-filtered one and a few
max_spp; the time ratio is that of the adaptive renders' wall time to render(8)'s."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime in the process)

import adaptive_ref as ar  # noqa: E402
import temporal_bench as tb  # noqa: E402
from tyrant_amd import binding, scenes  # noqa: E402


def spread(xs):
    q = np.percentile(xs, [10, 90])
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "p10_ms": float(q[0]), "p90_ms": float(q[1]), "max_ms": max(xs), "n": len(xs)}


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def c3(flags=0):
    W, H = 1920, 1080
    sc = scenes.mesh_scene(706)
    g = binding.Renderer(W, H, 8 * W * H, flags=binding.TYR_FLAG_TRIANGLE_MATERIALS | flags)
    g.set_spheres(sc.spheres)
    g.set_sun_position(*sc.sun_position)
    g.build_upload(sc.triangles)
    g.set_camera(sc.camera)
    return g, W, H


def overhead(reps, warmup):
    g, W, H = c3()
    full = torch.full((H, W), 8, dtype=torch.int32, device="cuda:0")
    uni, ada = [], []
    for i in range(warmup + reps):
        g.set_frame(1)
        g.reset_accum()
        a = wall(lambda: g.render(8))
        g.set_frame(1)
        g.reset_accum()
        b = wall(lambda: g.render_adaptive(full))
        if i >= warmup:
            uni.append(a)
            ada.append(b)
    assert g.counters()["device_error"] == 0
    res = {"render_8": spread(uni), "render_adaptive_full_8": spread(ada)}
    res["median_ratio"] = res["render_adaptive_full_8"]["median_ms"] / res["render_8"]["median_ms"]
    g.close()
    # the camera-ray kernel itself inside the same renders: TYR_FLAG_PROFILE's hipEvent pair around the primary stage only
    # (k_primary against k_primary_mapped, summed over a render's launches), on a ctx of its own
    g, W, H = c3(binding.TYR_FLAG_PROFILE)
    g.set_tuning(profile_mask=1)
    pu, pa = [], []
    for i in range(warmup + reps):
        g.set_frame(1)
        g.reset_accum()
        g.timings(reset=True)
        g.render(8)
        a = g.timings(reset=True)["primary"]["ms"]
        g.set_frame(1)
        g.reset_accum()
        g.render_adaptive(full)
        b = g.timings(reset=True)["primary"]["ms"]
        if i >= warmup:
            pu.append(a)
            pa.append(b)
    res["primary_stage_in_render_8"] = spread(pu)
    res["primary_stage_in_render_adaptive_full_8"] = spread(pa)
    # the map and its list at 1080p: an 8-spp-average allocation from one sample's error stand-in
    g.set_frame(1)
    g.reset_accum()
    g.render(2)
    err = torch.from_numpy(ar.two_buffer_error(g.blit_buffer(), np.zeros((W * H, 4), np.float32)).reshape(H, W)).to("cuda:0")
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    res["allocate_samples_8spp_1080p"] = tb.timed(stream, reps, warmup, lambda: g.allocate_samples(err, 8 * W * H, stream=stream))
    m, total = g.allocate_samples(err, 8 * W * H)
    res["allocated_map"] = {"total": total, "max": int(m.max().item()), "min": int(m.min().item())}
    # (set_sample_map returns once the list is built: wall time of the call)
    res["set_sample_map_8spp_1080p"] = spread([wall(lambda: g.set_sample_map(m)) for _ in range(warmup + reps)][warmup:])
    res["set_sample_map_uniform_8_1080p"] = spread([wall(lambda: g.set_sample_map(full)) for _ in range(warmup + reps)][warmup:])
    g.set_budget(0)
    g.close()
    return res


def quality(name, W, H, ref_spp=1024):
    from conftest import built_scene

    sc, nodes, prims = built_scene(name)
    flags = (1 if sc.triangle_materials else 0) | (8 if sc.light_list else 0) | (16 if sc.triangle_colors else 0)
    P = W * H
    g = binding.Renderer(W, H, 1 << 16, flags=flags)
    g.load_scene(sc, nodes, prims)
    g.render(ref_spp)
    ref = g.blit_buffer()
    ref = ref[:, :3] / ref[:, 3:4]

    def mse(buf):
        return float(np.mean((buf[:, :3] / buf[:, 3:4] - ref) ** 2))

    g.set_frame(5000)
    g.reset_accum()
    t_uni = wall(lambda: g.render(8))
    uni = g.blit_buffer()
    g.set_frame(9000)
    g.reset_accum()
    g.render(2)
    a = g.blit_buffer()
    g.reset_accum()
    g.render(2)
    b = g.blit_buffer()
    raw = ar.two_buffer_error(a, b).reshape(H, W)
    out = {"uniform_8_mse": mse(uni)}
    # tests/test_adaptive.py's recipe exactly: the adaptive render follows the two 2-spp renders' frames
    m, _ = g.allocate_samples(ar.box3(raw), 4 * P, min_spp=1, max_spp=65535)
    g.reset_accum()
    g.render_adaptive(m)
    out["test_recipe_box3_mse_ratio"] = mse(a + b + g.blit_buffer()) / mse(uni)
    for filt in ("raw", "box3"):
        err = raw if filt == "raw" else ar.box3(raw)
        for max_spp in (16, 64, 256, 65535):
            g.reset_accum()
            g.set_frame(9000 + 7)
            m, total = g.allocate_samples(err, 4 * P, min_spp=1, max_spp=max_spp)
            g.reset_accum()
            t_ada = wall(lambda: g.render_adaptive(m))
            c = g.blit_buffer()
            ada = a + b + c
            out[f"{filt}_max{max_spp}"] = {"spent": int(ada[:, 3].sum()), "mse_ratio": mse(ada) / mse(uni), "adaptive_render_ms_over_render8_ms": t_ada / t_uni,
                                           "clamped_pixels": int((m.cpu().numpy() >= max_spp).sum())}
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_bench_c3.json"))
    args = ap.parse_args()
    res = {"workload": "C3: mesh_scene(706), 1920x1080, queue 8 spp of pixels; quality: 96x64 / 96x54 small scenes, 8 spp both ways",
           "device": torch.cuda.get_device_name(0), "overhead": overhead(args.reps, args.warmup), "quality": {}}
    for name, W, H in (("tyrant_default", 96, 64), ("glass_dof48", 96, 54), ("cornell36", 96, 64)):
        res["quality"][name] = quality(name, W, H)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
