"""The camera window (host/primary_window.cpp, tyr_primary_window_probe): the pixel rectangle outside which no camera ray passes
the root box of the scene's tree.  tyr_render makes the window's camera rays first and the others beside the traversal launch
(DESIGN.md 4.8 (6)), so the window must hold every ray that enters the tree -- checked here on the ORACLE's own camera rays,
with the traversal's own root-box test in binary32 -- and must be a small part of the frame where the scene is, or the split
would idle.  No GPU: the probe is host code."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from conftest import built_scene

SPP = 2  # two sweeps over the frame: two sets of jitters


def _cam(base, **kw):
    return dataclasses.replace(base, **kw)


def cameras():
    from tyrant_amd import scenes

    c = scenes.CORNELL_CAMERA  # (0, -190, 50) looking along +y at the room [-50, 50] x [-50, 50] x [0, 100]
    return {
        "cornell": c,
        "edge": _cam(c, position=(110.0, -190.0, 50.0)),         # translated: the box runs off the frame's left edge
        "inside": _cam(c, position=(0.0, 0.0, 50.0)),            # inside the room
        "away": _cam(c, direction=(0.0, -1.0, 0.0)),             # every corner behind the camera
        "corner_behind": _cam(c, position=(0.0, -60.0, 50.0), direction=(1.0, 1.0, 0.0)),  # the box in view, two of its edges behind the camera plane
        "thin_lens": _cam(c, focalDistance=60.0, lensRadius=0.5),
        "off_axis": _cam(c, position=(30.0, -150.0, 20.0), direction=(-0.2, 1.0, 0.25)),   # not normalised, not axis-aligned
    }


WHOLE = ("inside", "away", "corner_behind", "thin_lens")  # section 1's three cases (two cameras for "a corner on or behind the plane")


def oracle_camera_rays(orc, scene, cam, W, H, rank, nranks):
    sc, nodes, prims = scene
    o = orc.Oracle(W, H, (W * H // nranks) * SPP, rank=rank, nranks=nranks, flags=1 if sc.triangle_materials else 0)
    o.load_scene(sc, nodes, prims)
    o.set_camera(cam)
    o.stage("begin")
    o.stage("primary")
    n = o.counters()["n_live"]
    assert n == (W * H // nranks) * SPP
    return o.ray_queue(0, n)


def passes_root_box(rays, lo, hi):
    """root_ref (hip/device_common.hpp) = slab_test (hip/traverse.hpp, Bbox.h:61) in binary32, with no bound on the distance (a
    sphere in front only removes rays)"""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        o, d = rays["origin"].astype(f), rays["direction"].astype(f)
        inv = f(1.0) / d
        neg = inv < 0
        near, far = np.where(neg, hi, lo).astype(f), np.where(neg, lo, hi).astype(f)
        t0, t1 = (near - o) * inv, (far - o) * inv
        tmin, tmax = t0[:, 0].copy(), t1[:, 0].copy()
        ok = ~((tmin > t1[:, 1]) | (t0[:, 1] > tmax))
        tmin, tmax = np.where(t0[:, 1] > tmin, t0[:, 1], tmin), np.where(t1[:, 1] < tmax, t1[:, 1], tmax)
        ok &= ~((tmin > t1[:, 2]) | (t0[:, 2] > tmax))
        tmax = np.where(t1[:, 2] < tmax, t1[:, 2], tmax)
        return ok & (tmax > 0)


CASES = [(scene, cam, 96, 64, 0, 1) for scene in ("cornell_soup2k", "mesh32") for cam in ("cornell", "edge", "off_axis")]
CASES += [("cornell_soup2k", cam, 96, 64, 0, 1) for cam in WHOLE]
CASES += [("cornell_soup2k", cam, 96, 66, rank, 3) for cam in ("cornell", "off_axis") for rank in (0, 1, 2)]
CASES += [("mesh32", "cornell", 97, 61, 0, 1)]


@pytest.mark.parametrize("scene,cam,W,H,rank,nranks", CASES)
def test_no_ray_outside_the_window_passes_the_root_box(orc, scene, cam, W, H, rank, nranks):
    from tyrant_amd import binding

    built = built_scene(scene)
    lo, hi = built[1][0]["bounds"]
    camera = cameras()[cam]
    w = binding.primary_window_probe(camera, W, H, lo, hi, rank, nranks)
    rays = oracle_camera_rays(orc, built, camera, W, H, rank, nranks)
    x, y = rays["index"] % W, rays["index"] // W
    assert np.all(y % nranks == rank)
    enters = passes_root_box(rays, lo, hi)
    outside = ~((x >= w["x0"]) & (x < w["x1"]) & (y >= w["y0"]) & (y < w["y1"]))
    print(cam, w, "rays", len(rays), "enter the tree", int(enters.sum()), "outside the window", int(outside.sum()))
    assert int(np.count_nonzero(outside & enters)) == 0
    # the rows of the window among the rank's own
    yl = y // nranks
    assert np.array_equal((y >= w["y0"]) & (y < w["y1"]), (yl >= w["local_y0"]) & (yl < w["local_y1"]))
    if cam in WHOLE:
        assert w["whole_frame"] == 1 and (w["x0"], w["x1"], w["y0"], w["y1"]) == (0, W, 0, H), w
    else:
        assert w["whole_frame"] == 0 and enters.any(), w
        # ... and not a loose one: the rays that enter the tree reach within the jitter's pixel and the margin's two of every side that is not the frame's
        ex, ey = x[enters], y[enters]
        # (a rank sees every nranks-th row only)
        for side, reach, at_frame, slack in ((w["x0"], ex.min(), 0, 3), (w["y0"], ey.min(), 0, 2 + nranks)):
            assert side == at_frame or reach - side <= slack, (w, reach)
        for side, reach, at_frame, slack in ((w["x1"], ex.max() + 1, W, 3), (w["y1"], ey.max() + 1, H, 2 + nranks)):
            assert side == at_frame or side - reach <= slack, (w, reach)


def test_the_cornell_window_is_a_small_part_of_the_frame():
    """otherwise every test of the split would pass with the feature idle"""
    from tyrant_amd import binding, scenes

    for scene in ("cornell_soup2k", "mesh32"):
        lo, hi = built_scene(scene)[1][0]["bounds"]
        for W, H in ((96, 64), (1920, 1080)):
            w = binding.primary_window_probe(scenes.CORNELL_CAMERA, W, H, lo, hi)
            area = (w["x1"] - w["x0"]) * (w["y1"] - w["y0"])
            assert w["whole_frame"] == 0 and 0 < area < W * H / 4, (scene, W, H, w)
    w = binding.primary_window_probe(cameras()["edge"], 96, 64, lo, hi)
    assert w["whole_frame"] == 0 and w["x0"] == 0 and w["x1"] < 96, w  # the translated camera: the box touches the frame's edge


def test_the_inset_shrinks_the_window_and_bad_arguments_are_refused():
    from tyrant_amd import binding, scenes

    lo, hi = built_scene("cornell_soup2k")[1][0]["bounds"]
    w0 = binding.primary_window_probe(scenes.CORNELL_CAMERA, 96, 64, lo, hi)
    w6 = binding.primary_window_probe(scenes.CORNELL_CAMERA, 96, 64, lo, hi, inset=6)
    assert (w6["x0"], w6["x1"], w6["y0"], w6["y1"]) == (w0["x0"] + 6, w0["x1"] - 6, w0["y0"] + 6, w0["y1"] - 6)
    assert binding.primary_window_probe(scenes.CORNELL_CAMERA, 96, 64, lo, hi, inset=40)["whole_frame"] == 1  # nothing left of it
    with pytest.raises(binding.TyrError):
        binding.primary_window_probe(scenes.CORNELL_CAMERA, 96, 64, lo, hi, rank=0, nranks=3)  # 64 rows do not deal out to three ranks
