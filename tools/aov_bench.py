"""First-hit AOV pass (tyr_render_aov) on C3 (1920 x 1080, the 1 M-triangle height field) against the camera rays' share of
the render: k_primary plus the first traversal launch of the same 8-spp job (queue 8 W H), from TYR_FLAG_PROFILE timings.
Those two launches make and trace the same camera rays without shading them.

    python tools/aov_bench.py [--reps 20] [--out profiles/aov_bench_c3.json]

AOV time: hipEvent pairs around the call on its stream, after warm-up calls.  The render's: the "primary" and "extend"
stage timings of render(8, max_iterations=1) -- one iteration: the top-up and its traversal launch (the stage timings'
events bracket the launches)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import frame_bench_common as fb  # noqa: E402  (torch before the library: one HIP runtime in the process)
import torch  # noqa: E402
from frame_bench_common import SPP, H, W  # noqa: E402
from tyrant_amd import binding  # noqa: E402


def summary(ms):
    return fb.summary(ms, percentiles=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=706)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_bench_c3.json"))
    args = ap.parse_args()
    g, sc, nodes, prims = fb.c3_renderer(flags=binding.TYR_FLAG_PROFILE, cells=args.cells)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    aov = {f"spp{spp}": fb.timed(stream, args.reps, 3, lambda: g.render_aov(spp, stream=stream), percentiles=False) for spp in (1, SPP)}

    # the render's camera-ray launches: the first iteration of the same job, each on a fresh ctx (an empty queue at frame 1)
    prim_ms, ext_ms = [], []
    for _ in range(3):
        r = binding.Renderer(W, H, SPP * W * H, flags=binding.TYR_FLAG_PROFILE | binding.TYR_FLAG_TRIANGLE_MATERIALS)
        r.set_spheres(sc.spheres)
        r.set_camera(sc.camera)
        r.set_sun_position(*sc.sun_position)
        r.upload(nodes, prims)
        r.timings(reset=True)
        r.render(SPP, 1)
        t = r.timings(reset=True)
        prim_ms.append(t["primary"]["ms"])
        ext_ms.append(t["extend"]["ms"])
        r.close()
    render = {"primary": summary(prim_ms), "first_traversal": summary(ext_ms),
              "primary_plus_first_traversal_median_ms": statistics.median([p + e for p, e in zip(prim_ms, ext_ms)])}
    res = {
        "workload": "C3: mesh_scene(706), 1920x1080, camera rays of an 8-spp job (queue 8 W H) at frame 1",
        "render_aov": aov,
        "render_camera_rays": render,
        "aov8_over_primary_plus_first_traversal": aov[f"spp{SPP}"]["median_ms"] / render["primary_plus_first_traversal_median_ms"],
        "query_error": g.query_error(),
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    g.close()


if __name__ == "__main__":
    main()
