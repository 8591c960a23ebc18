"""What the frame benchmarks (tools/{aov,denoise,temporal,svgf,taa,specular_guides}_bench.py) share: the summary of a call's
samples and the loop that takes them, the C3 renderer their timings run on, and the panning Cornell sequence with its converged
reference that the quality figures of tyr_temporal, tyr_svgf and tyr_taa come from."""
from __future__ import annotations

import dataclasses
import math
import statistics
import time

import numpy as np
import torch  # (before the library: one HIP runtime in the process)

from tyrant_amd import binding, scenes

W, H, SPP = 1920, 1080, 8  # C3 at 1080p, and the samples of the render the filters are timed next to


def summary(ms, percentiles=True):
    res = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}
    if percentiles:
        res["p10_ms"], res["p90_ms"] = (float(q) for q in np.percentile(ms, [10, 90]))
    return res


def timed(stream, calls, warmup, fn, percentiles=True):
    """fn() `calls` times behind `warmup` calls, each timed with an event pair around it on `stream` and waited for"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return summary(ms, percentiles)


def moved(cam, k):
    """the pan: 0.4 k units along x and 0.002 k rad about z"""
    a = 0.002 * k
    dx, dy, dz = cam.direction
    c, s = math.cos(a), math.sin(a)
    return dataclasses.replace(cam, position=(cam.position[0] + 0.4 * k, cam.position[1], cam.position[2]), direction=(c * dx - s * dy, s * dx + c * dy, dz))


def c3_renderer(steps=0, flags=0, queue=SPP * W * H, cells=706):
    """C3 -- mesh_scene(706) at 1920 x 1080 -- built and uploaded, the camera moved from the scene's by `steps` pan steps:
    (renderer, scene, nodes, prims)"""
    sc = scenes.mesh_scene(cells)
    g = binding.Renderer(W, H, queue, flags=flags | binding.TYR_FLAG_TRIANGLE_MATERIALS)
    g.set_spheres(sc.spheres)
    g.set_sun_position(*sc.sun_position)
    nodes, prims, _ = g.build_upload(sc.triangles)
    g.set_camera(moved(sc.camera, steps) if steps else sc.camera)
    return g, sc, nodes, prims


def c3_guides(g, sc):
    """the filters' inputs at frame 1 of a moved camera: render_aov(1), and render_motion against the scene's camera --
    (aov, {albedo, normal, depth}, {motion, prev_depth})"""
    g.set_frame(1)
    aov = g.render_aov(1)
    mot = g.render_motion(aov["prim"], aov["geom"], sc.camera)
    return aov, {k: aov[k] for k in ("albedo", "normal", "depth")}, {"motion": mot["motion"], "prev_depth": mot["prev_depth"]}


def timed_renders(g, reps=3):
    """host clock around render(SPP) from frame 1 (it returns once the stream is idle): the report's "render_8spp" """
    ms = []
    for _ in range(reps):
        g.reset_accum()
        g.set_frame(1)
        t0 = time.perf_counter()
        g.render(SPP)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": ms, "median_ms": statistics.median(ms)}


def pan_scene(frames=16):
    """the Cornell box at scenes.FRAMED_CAMERA, built, and the cameras of a pan of `frames` frames: (scene, nodes, prims, cameras)"""
    sc = dataclasses.replace(scenes.cornell_box(), camera=scenes.FRAMED_CAMERA)
    nodes, prims = binding.bvh_build(sc.triangles)
    return sc, nodes, prims, [moved(sc.camera, k) for k in range(frames)]


def pan_frames(g, cams, reset_accum=False):
    """per camera set_camera (-> reset_accum) -> render_aov(1) -> render_motion against the camera before -> render(1): yields
    (aov, motion, the accumulation buffer on the host) as each frame is done"""
    prev = cams[0]
    for cam in cams:
        g.set_camera(cam)
        if reset_accum:
            g.reset_accum()
        aov = g.render_aov(1)
        mot = g.render_motion(aov["prim"], aov["geom"], prev)
        g.render(1)
        yield aov, mot, g.blit_buffer()
        prev = cam


def converged(sc, nodes, prims, cam, Wq, Hq, spp, queue=1 << 18, flags=0):
    """the accumulation buffer of `spp` samples per pixel on a ctx of its own, at `cam` (None: the scene's camera)"""
    r = binding.Renderer(Wq, Hq, queue, flags=flags)
    r.load_scene(sc, nodes, prims)
    if cam is not None:
        r.set_camera(cam)
    r.render(spp)
    conv = r.blit_buffer()
    r.close()
    return conv


def reference(noisy, conv):
    """(seen, mse) of a noisy and a converged accumulation buffer: the pixels both saw, and the linear rgb MSE of a frame of
    (.., 3) or (.., 4) floats against the converged one over those pixels"""
    seen = (noisy[:, 3] > 0) & (conv[:, 3] > 0)
    want = conv[seen, :3].astype(np.float64) / conv[seen, 3:]
    return seen, lambda a: float(((a.reshape(-1, a.shape[-1])[seen, :3].astype(np.float64) - want) ** 2).mean())
