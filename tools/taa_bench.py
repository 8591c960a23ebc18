"""Temporal anti-aliasing (tyr_taa): its time on C3 at 1080p next to tyr_temporal and tyr_svgf, and what it does to the error and
the frame-to-frame flicker of tools/temporal_bench.py's panning Cornell sequence and of a still camera, with the grid the
defaults come from.

    python tools/taa_bench.py [--calls 200] [--out profiles/taa_bench_c3.json]

Time: C3 (1920 x 1080, the 1 M-triangle height field) as tools/svgf_bench.py sets it up: 1-spp tyr_render_aov guides at a camera
moved by 3 pan steps, tyr_render_motion against the scene's camera, an 8-spp accumulation buffer; the colour input is
tyr_svgf's resolved frame.  tyr_taa with its defaults, tyr_taa with bilinear=True, tyr_temporal and tyr_svgf with theirs take
turns -- one call each per round, `--calls` rounds after warm-up -- each call timed with a hipEvent pair around it on its
stream: median and spread.

Quality: temporal_bench.py's sequence (the framed Cornell view at 128 x 72, 16 frames at 1 spp of a slow pan), every frame
through set_camera -> reset_accum -> render_aov(1) -> render_motion -> render(1) -> svgf(resolve=True) -> taa, against a 1024-spp
render PER FRAME resolved with tyr_resolve (display space, over the pixels both saw).  Over the last 8 frames, for svgf alone
and for svgf -> taa: the mean MSE, and the flicker -- the mean over pixels and consecutive frame pairs of
((out_k - ref_k) - (out_{k-1} - ref_{k-1}))^2.  The same for 16 frames of a still camera (one reference).  The grid runs taa
over the same svgf frames for alpha x gamma x sampler; "selected" is the grid point with the lowest panning flicker among those
whose panning MSE is within 5 % of the grid's best -- the rule the shipped defaults (binding.TAA_ALPHA, TAA_GAMMA) follow."""
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

ALPHA = (0.05, 0.1, 0.2, 0.4)
GAMMA = (0.75, 1.0, 1.25, 1.5)
TAIL = 8  # the frames the figures are taken over: the last 8 of 16
MSE_SLACK = 1.05


def alternated(stream, calls, warmup, fns):
    """fns: name -> callable; one call of each per round, each timed with its own event pair"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: fb.summary(v) for k, v in ms.items()}


def timing(calls, warmup):
    g, sc, _, _ = fb.c3_renderer(steps=3)
    aov, gd, mv = fb.c3_guides(g, sc)
    g.reset_accum()
    g.set_frame(1)
    g.render(fb.SPP)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    color = g.svgf(**gd, **mv, reset=True, resolve=True)
    g.temporal(**gd, **mv, reset=True)
    out = torch.empty_like(color)
    g.taa(color, aov["depth"], **mv, reset=True, out=out)
    torch.cuda.synchronize()
    res = alternated(stream, calls, warmup, {
        "taa": lambda: g.taa(color, aov["depth"], **mv, out=out, stream=stream),
        "taa_bilinear": lambda: g.taa(color, aov["depth"], **mv, bilinear=True, out=out, stream=stream),
        "temporal": lambda: g.temporal(**gd, **mv, stream=stream),
        "svgf": lambda: g.svgf(**gd, **mv, stream=stream),
    })
    torch.cuda.synchronize()
    res["taa_over_svgf"] = res["taa"]["median_ms"] / res["svgf"]["median_ms"]
    res["taa_over_temporal"] = res["taa"]["median_ms"] / res["temporal"]["median_ms"]
    res["pixels_seen_fraction"] = float((color.reshape(-1, 4)[:, 3] != 0).float().mean().item())
    g.close()
    return res


def resolved_reference(sc, nodes, prims, cam, Wq, Hq, spp):
    """(display-space frame (n, 4), the accumulation's count channel)"""
    r = binding.Renderer(Wq, Hq, 1 << 18)
    r.load_scene(sc, nodes, prims)
    r.set_camera(cam)
    r.reset_accum()
    r.render(spp)
    dst = torch.zeros((Hq, Wq, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.resolve_into(dst.data_ptr())
    torch.cuda.synchronize()
    cnt = r.blit_buffer()[:, 3]
    r.close()
    return dst.cpu().numpy().reshape(-1, 4).astype(np.float64), cnt


def figures(outs, refs):
    """(mean MSE, flicker) of the last TAIL frames; outs: (n, 4) float arrays, refs: (frame, seen mask) per frame"""
    err, ok = [], []
    for o, (r, seen) in zip(outs[-TAIL:], refs[-TAIL:]):
        o = o.astype(np.float64)
        ok.append(seen & (o[:, 3] != 0))
        err.append(o[:, :3] - r[:, :3])
    mse = float(np.mean([(e[m] ** 2).mean() for e, m in zip(err, ok)]))
    num = cnt = 0.0
    for k in range(1, TAIL):
        m = ok[k] & ok[k - 1]
        d = (err[k] - err[k - 1])[m]
        num += float((d ** 2).sum())
        cnt += d.size
    return mse, num / cnt


def sequence(g, sc, nodes, prims, cams, Wq, Hq, ref_spp):
    """the recipe up to svgf(resolve=True) for every camera, and the resolved references of the last TAIL frames"""
    seq = []
    for k, (aov, mot, acc) in enumerate(fb.pan_frames(g, cams, reset_accum=True)):
        # (a copy of the accumulation, as tools/svgf_bench.py passes it: the filter runs on torch's stream, and the next frame's
        # reset_accum on the ctx's would otherwise clear the buffer under it)
        sv = g.svgf(aov["albedo"], aov["normal"], aov["depth"], mot["motion"], mot["prev_depth"], accum=torch.from_numpy(acc).to("cuda:0"), reset=(k == 0), resolve=True)
        seq.append((sv, aov["depth"], mot["motion"], mot["prev_depth"], acc[:, 3] > 0))
    torch.cuda.synchronize()
    refs, cache = [], {}
    for k, cam in enumerate(cams):
        if k < len(cams) - TAIL:
            refs.append(None)
            continue
        key = (tuple(cam.position), tuple(cam.direction))
        if key not in cache:
            cache[key] = resolved_reference(sc, nodes, prims, cam, Wq, Hq, ref_spp)
        r, cnt = cache[key]
        refs.append((r, (cnt > 0) & seq[k][4]))
    return seq, refs


def run_taa(g, seq, **kw):
    outs = []
    for k, (sv, z, m, pd, _) in enumerate(seq):
        outs.append(g.taa(sv, z, m, pd, reset=(k == 0), **kw).cpu().numpy().reshape(-1, 4))
    return outs


def quality(frames=16, ref_spp=1024, Wq=128, Hq=72):
    sc, nodes, prims, cams = fb.pan_scene(frames)
    g = binding.Renderer(Wq, Hq, 1 << 16)
    g.load_scene(sc, nodes, prims)
    runs = {"panning": cams, "still": [sc.camera] * frames}
    data = {}
    for name, cams in runs.items():
        seq, refs = sequence(g, sc, nodes, prims, cams, Wq, Hq, ref_spp)
        mse, flicker = figures([s[0].cpu().numpy().reshape(-1, 4) for s in seq], refs)
        data[name] = (seq, refs, mse, flicker)

    def point(**kw):
        res = {}
        for name, (seq, refs, mse, flicker) in data.items():
            m, f = figures(run_taa(g, seq, **kw), refs)
            res[name] = {"taa_mse": m, "taa_flicker": f, "mse_ratio": m / mse, "flicker_ratio": f / flicker}
        return res

    grid = [dict(alpha=a, gamma=gm, bilinear=b, **point(alpha=a, gamma=gm, bilinear=b)) for b in (False, True) for a in ALPHA for gm in GAMMA]
    best_mse = min(p["panning"]["taa_mse"] for p in grid)
    sel = min((p for p in grid if p["panning"]["taa_mse"] <= MSE_SLACK * best_mse), key=lambda p: p["panning"]["taa_flicker"])
    cr = [p for p in grid if not p["bilinear"]]
    best_cr = min(p["panning"]["taa_mse"] for p in cr)
    sel_cr = min((p for p in cr if p["panning"]["taa_mse"] <= MSE_SLACK * best_cr), key=lambda p: p["panning"]["taa_flicker"])
    res = {"workload": f"cornell_box at FRAMED_CAMERA, {Wq}x{Hq}, {frames} frames at 1 spp: a pan (0.4 units, 0.002 rad per frame) and a still camera; recipe render_aov -> render_motion -> render -> "
                       f"svgf(resolve) -> taa; the last {TAIL} frames against {ref_spp} spp per frame resolved by tyr_resolve; display-space rgb",
           "svgf": {name: {"mse": d[2], "flicker": d[3]} for name, d in data.items()},
           "defaults": {"alpha": binding.TAA_ALPHA, "gamma": binding.TAA_GAMMA, "bilinear": False}}
    res.update(point())
    res["grid_best_mse"] = best_mse
    res["selected"] = {k: sel[k] for k in ("alpha", "gamma", "bilinear")}
    res["selected_catmull_rom"] = {k: sel_cr[k] for k in ("alpha", "gamma", "bilinear")}
    res["grid"] = grid
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taa_bench_c3.json"))
    args = ap.parse_args()
    t0 = time.perf_counter()
    res = {"workload": "C3: mesh_scene(706), 1920x1080; render_aov(1) at a camera moved by 3 pan steps, render_motion against the scene's camera, an 8-spp accumulation; tyr_taa on tyr_svgf's resolved frame, "
                       "default and bilinear, taking turns with tyr_temporal and tyr_svgf (their defaults)"}
    if not args.no_timing:
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
