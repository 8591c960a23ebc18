"""A top-up of camera rays made in two parts (TYR_TUNE_PRIMARY_OVERLAP): k_primary_window in front of the
iteration's traversal launch, k_primary_rest beside it on the ctx's second stream.  Which kernel makes a ray, and when, must not
show: renders agree with the oracle after every call -- iterations, every counter, the accumulation, the work queue bit for bit
-- with the split on and off, at three, four and five traversal blocks per CU, and with the window shrunk by six pixels
(TYR_TUNE_WINDOW_INSET), which puts rays that do enter the tree outside it: k_primary_rest then traces them itself.

The shapes, one failure mode each:
  whole    96 x 64, 2 spp, queue W * H * 2            whole sweeps over the frame in one top-up
  partial  96 x 64, 3 spp, queue W * H + 37           partial sweeps, the start position wrapping mid-row and mid-window, a top-up in every iteration
  ragged   97 x 61, 2 spp, queue W * H * 2            window edges that are not wave boundaries
  shard    96 x 66, rank 1 of 3, 2 spp                row sharding (the issue names 96 x 64, whose rows do not deal out to three ranks: tyr_create refuses it)
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from conftest import bits, built_scene
from test_gpu_parity import assert_accum_close, assert_state_equal
from test_render_sequences import FIELDS, PROFILES, Sides

gpu = pytest.mark.gpu

# (W, H, N, rank, nranks, spp)
SHAPES = {
    "whole": (96, 64, 96 * 64 * 2, 0, 1, 2),
    "partial": (96, 64, 96 * 64 + 37, 0, 1, 3),
    "ragged": (97, 61, 97 * 61 * 2, 0, 1, 2),
    "shard": (96, 66, 96 * 22 * 2, 1, 3, 2),
}
assert SHAPES["partial"][2] % 64 != 0
# the split's knobs: off; on at 3 / 4 / 5 traversal blocks per CU, the window as computed and shrunk by 6 pixels
KNOBS = {"off": dict(primary_overlap=0)}
KNOBS.update({f"on{b}_inset{i}": dict(primary_overlap=1, overlap_trace_blocks=b, window_inset=i, overlap_min_new=0) for b in (3, 4, 5) for i in (0, 6)})
LOOPS = ("default", "run_ahead0", "fold_prologue0")  # the merged render loops (launch_kernels' order, merge_trace 0, makes no split)


def sides(orc, hip, shape, knobs, profile="default", scene="cornell_soup2k", camera=None):
    W, H, N, rank, nranks, _ = SHAPES[shape]
    built = built_scene(scene)
    if camera is not None:
        built = (dataclasses.replace(built[0], camera=camera),) + tuple(built[1:])
    s = Sides(orc, hip, built, W, H, N, rank, nranks, profile)
    s.g.set_tuning(**KNOBS[knobs])
    return s


def expect_strays(s, knobs):
    w = s.g.primary_window()
    assert w["whole_frame"] == 0, w
    assert (w["splits"] > 0) == bool(KNOBS[knobs]["primary_overlap"]), (knobs, w)  # top-ups were launched in two parts, or none was
    if KNOBS[knobs].get("window_inset"):
        assert w["strays"] > 0, (knobs, w)  # the path that traces a ray outside the window ran
    else:
        assert w["strays"] == 0, (knobs, w)  # the window as computed holds every ray that enters the tree
    return w


@gpu
@pytest.mark.parametrize("profile", LOOPS)
@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_renders_match_the_oracle(orc, hip, shape, knobs, profile):
    """two full renders with an empty render and a render cut short between them, compared after every call"""
    s = sides(orc, hip, shape, knobs, profile)
    spp = SHAPES[shape][5]
    s.render(spp)
    s.render(0)
    s.render(2, 1)
    s.render(spp)
    expect_strays(s, knobs)


@gpu
@pytest.mark.parametrize("knobs", ["off", "on3_inset6", "on4_inset0"])
def test_on_the_mesh_scene_with_triangle_materials(orc, hip, knobs):
    s = sides(orc, hip, "partial", knobs, scene="mesh32")
    s.render(3), s.render(2, 2), s.render(1)
    expect_strays(s, knobs)


@gpu
def test_the_ctx_window_is_the_probes_and_follows_the_camera(hip):
    from tyrant_amd import binding, scenes

    sc, nodes, prims = built_scene("cornell_soup2k")
    lo, hi = nodes[0]["bounds"]
    g = hip.Renderer(96, 66, 4096, rank=1, nranks=3)
    assert g.primary_window()["whole_frame"] == 1  # no scene yet
    g.load_scene(sc, nodes, prims)
    assert g.primary_window() == binding.primary_window_probe(sc.camera, 96, 66, lo, hi, 1, 3)
    moved = dataclasses.replace(sc.camera, position=(30.0, -150.0, 20.0), direction=(-0.2, 1.0, 0.25))
    g.set_camera(moved)
    g.set_tuning(window_inset=3)
    assert g.primary_window() == binding.primary_window_probe(moved, 96, 66, lo, hi, 1, 3, inset=3)
    g.set_camera(dataclasses.replace(sc.camera, position=(0.0, 0.0, 50.0)))
    assert g.primary_window()["whole_frame"] == 1  # inside the room


@gpu
def test_a_thin_lens_takes_the_single_kernel(orc, hip):
    """no window is derived for a lens: the split's knobs must change nothing -- against the oracle, and the two HIP ctxs against each
    other: counters and queues bit for bit, path counts exact (the pixel sums are float atomics: their order is not fixed between
    two runs of ONE path either, so they are compared as everywhere, to 1e-5)"""
    from tyrant_amd import scenes

    lens = dataclasses.replace(scenes.CORNELL_CAMERA, focalDistance=60.0, lensRadius=0.5)
    a, b = sides(orc, hip, "whole", "on3_inset6", camera=lens), sides(orc, hip, "whole", "off", camera=lens)
    for s in (a, b):
        s.render(2), s.render(2, 2)
        w = s.g.primary_window()
        assert w["whole_frame"] == 1 and w["strays"] == 0 and w["splits"] == 0, w
    ka, kb = a.g.counters(), b.g.counters()
    assert {f: ka[f] for f in FIELDS} == {f: kb[f] for f in FIELDS}
    n = ka["primary_ray_cnt"]
    assert n > 0
    assert_state_equal(a.g.ray_queue(0, n), b.g.ray_queue(0, n), "thin lens: split on against off")
    assert_accum_close(a.g.blit_buffer(), b.g.blit_buffer(), "thin lens: split on against off")


@gpu
def test_a_sample_map_takes_the_mapped_kernel(orc, hip):
    """tyr_render_adaptive's camera rays come from the map's ticket list (launch_primary_mapped): with the split's knobs set, and the
    window shrunk so that the split would show as strays, a uniform map is still the oracle's render"""
    W, H, N, rank, nranks, spp = SHAPES["partial"]
    s = sides(orc, hip, "partial", "on3_inset6")
    it = s.g.render_adaptive(np.full((H, W), spp, dtype=np.int32))
    assert it == s.o.render(spp)
    s.shadow_exact = False  # (the default tuning answers some shadow rays in place: Sides.render says the same for this profile)
    s.check("render_adaptive(uniform map)")
    w = s.g.primary_window()
    assert w["whole_frame"] == 0 and w["strays"] == 0 and w["splits"] == 0, w
    s.render(spp)  # ... and an un-mapped render behind it splits again
    w = s.g.primary_window()
    assert w["strays"] > 0 and w["splits"] > 0, w


@gpu
@pytest.mark.parametrize("knobs", ["on3_inset6", "on4_inset0"])
def test_ten_steps_repeat_the_first(hip, knobs):
    """set_frame(1), reset_accum, render(spp) ten times: every step is the same job"""
    from test_render_boundaries import STATE, TOTALS, small_ctx

    spp = 2
    g = small_ctx(hip, **KNOBS[knobs])
    first, before = None, g.counters()
    for step in range(10):
        g.set_frame(1)
        g.reset_accum()
        it = g.render(spp)
        k = g.counters()
        seen = dict({f: k[f] for f in STATE}, iterations=it, **{f: k[f] - before[f] for f in TOTALS})
        before = k
        if first is None:
            first = seen
            assert first["device_error"] == 0 and first["total_primary_rays"] == spp * 96 * 64, first
        assert seen == first, (knobs, step, {f: (first[f], seen[f]) for f in first if first[f] != seen[f]})
    fresh = small_ctx(hip, primary_overlap=0)
    fresh.render(spp)
    assert_accum_close(fresh.blit_buffer(), g.blit_buffer(), f"[{knobs}] step 10 against a fresh ctx's single-kernel render")
    w = g.primary_window()
    assert (w["strays"] > 0) == (KNOBS[knobs]["window_inset"] > 0) and w["splits"] >= 10, w


@gpu
def test_fuzz_slice_with_the_splits_knobs(hip):
    """30 seeded cases of tests/fuzz_primary_overlap.py: tests/fuzz_parity.py's random scenes, frames, shards (up to eight ranks), queue
    sizes and cameras against the oracle, with primary_overlap, overlap_trace_blocks, window_inset and overlap_min_new = 0 drawn on top"""
    import fuzz_primary_overlap as fz

    rng, own = np.random.default_rng(20261019), np.random.default_rng([20261019, 28])
    failed, split, strayed, sharded = [], 0, 0, 0
    for i in range(30):
        c = fz.draw_case(rng, own, i)
        ok, why, line, splits, strays = fz.run_case(c)
        print(line)
        split += splits > 0
        strayed += strays > 0
        sharded += splits > 0 and c["nranks"] > 1
        if not ok:
            failed.append(line)
    assert not failed, "\n".join(failed)
    assert split >= 8 and strayed >= 2 and sharded >= 2, (split, strayed, sharded)  # (the slice reaches the two kernels, the fallback and the row sharding)
