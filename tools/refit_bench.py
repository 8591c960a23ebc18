"""Cost of tyr_scene_refit (moving geometry in the uploaded tree) next to rebuilding the scene, on C3.

C3's scene (scenes.mesh_scene(706), 996,882 triangles) built and uploaded with tyr_scene_build_upload on a TYR_FLAG_REFIT ctx,
then:
  refit_device   a torch wave deformation of the height field's vertices on the device, then Renderer.refit(tensor): wall
                 time of the refit call alone (the deformation has finished before the clock starts), median of REPS calls
  refit_host     the same with numpy records (host input: the copy to the device is part of the call)
  build_upload   tyr_scene_build_upload of the same mesh: wall time, median of BUILDS calls, on a ctx without TYR_FLAG_REFIT
                 (and, as build_upload_with_refit_plan, on the refit ctx, nodes returned: the plan's extra cost)
  render         the C3 job (1920x1080, 8 spp) after a moderate deformation on the refitted tree and on a tree rebuilt from
                 the moved triangles (informational: what a refit loses in tree quality)

    python tools/refit_bench.py [--reps 20] [--out profiles/refit_bench_c3.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime in the process, see tests/conftest.py)

import numpy as np  # noqa: E402

from tyrant_amd import binding, scenes  # noqa: E402

W, H, SPP = 1920, 1080, 8


def summary(samples_ms):
    return {"median_ms": statistics.median(samples_ms), "min_ms": min(samples_ms), "max_ms": max(samples_ms), "samples": len(samples_ms)}


def wave(base_z, x, y, t, amp):
    """the height field's z moved by a travelling wave (the room's walls move with it: every vertex does)"""
    return base_z + amp * torch.sin(0.2 * x + t) * torch.cos(0.15 * y + 0.5 * t)


def renderer(sc, N, flags=0):
    g = binding.Renderer(W, H, N, flags=flags | binding.TYR_FLAG_TRIANGLE_MATERIALS)
    g.set_spheres(sc.spheres)
    g.set_camera(sc.camera)
    g.set_sun_position(*sc.sun_position)
    return g


def time_render(g, reps):
    out = []
    for _ in range(reps):
        g.reset_accum()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.render(SPP)
        out.append((time.perf_counter() - t0) * 1e3)
    return summary(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=706)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--render-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_bench_c3.json"))
    args = ap.parse_args()
    sc = scenes.mesh_scene(args.cells)
    N = min(SPP * W * H, 32 << 20)
    g = renderer(sc, N, binding.TYR_FLAG_REFIT)
    builds = []
    for _ in range(args.builds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nodes, prims, _ = g.build_upload(sc.triangles)
        builds.append((time.perf_counter() - t0) * 1e3)
    info = g.scene_info()
    g0 = renderer(sc, 1 << 16)  # the same call on a ctx without TYR_FLAG_REFIT (no plan kept)
    builds_plain = []
    for _ in range(args.builds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g0.build_upload(sc.triangles, want_nodes=False)
        builds_plain.append((time.perf_counter() - t0) * 1e3)
    g0.close()
    n = prims.shape[0]
    dev = torch.device("cuda", 0)
    rec = torch.from_numpy(prims.view(np.float32).reshape(n, 10).copy()).to(dev)  # vert = columns 0..2
    x, y, z0 = rec[:, 0].clone(), rec[:, 1].clone(), rec[:, 2].clone()

    # device input: a new wave every call
    dev_ms = []
    for k in range(args.reps + 3):
        rec[:, 2] = wave(z0, x, y, 0.1 * k, 1.5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.refit(rec)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 3:
            dev_ms.append(dt)
    # host input
    host_ms = []
    for k in range(args.reps + 3):
        m = prims.copy()
        m["vert"][:, 2] = wave(z0, x, y, 0.1 * k, 1.5).cpu().numpy()
        t0 = time.perf_counter()
        g.refit(m)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 3:
            host_ms.append(dt)

    # render after a moderate deformation: the refitted tree against one rebuilt from the moved triangles
    moved = prims.copy()
    moved["vert"][:, 2] = wave(z0, x, y, 1.0, 3.0).cpu().numpy()
    g.refit(moved)
    r_refit = time_render(g, args.render_reps)
    k_refit = g.counters()
    g.close()
    g2 = renderer(sc, N)
    g2.build_upload(moved)
    r_rebuilt = time_render(g2, args.render_reps)
    k_rebuilt = g2.counters()
    g2.close()

    result = {
        "scene": f"mesh_scene({args.cells})", "n_prims": int(n), "n_nodes": int(nodes.shape[0]), "n_quad_nodes": info["n_quad_nodes"],
        "device_bytes_with_refit_plan": info["device_bytes"],
        "refit_device_input": summary(dev_ms),
        "refit_host_input": summary(host_ms),
        "build_upload_with_refit_plan": summary(builds),
        "build_upload": summary(builds_plain),
        "render_8spp_after_deformation": {"refit_tree": r_refit, "rebuilt_tree": r_rebuilt,
                                          "extend_rays": [int(k_refit["total_extend_rays"]), int(k_rebuilt["total_extend_rays"])]},
        "gate_refit_device_below_ms": 1.1,
    }
    result["gate_met"] = result["refit_device_input"]["median_ms"] < 1.1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in result.items()}))


if __name__ == "__main__":
    main()
