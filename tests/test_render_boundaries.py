"""The boundaries of a render: what happens between the last kernel of one tyr_render and the first of the next, and how a
TYR_FLAG_PROFILE ctx times its stages.

tyr_reset_accum, tyr_set_budget and the undo of an iteration queued ahead for nothing write the host's mirror of the counters
themselves and send the few words they change in stream order: no copy of the whole struct, no wait.  What a caller can see must
not have changed: the counters after every call, the accumulation, the queues.  Stage times taken from events attached to the
stage's own launches (TYR_TUNE_STAGE_TIMING 1) must tell the same story as the event pairs (0), minus the idle the pairs
themselves put between the kernels -- profiles/boundary_idle_accounting.txt has that figure."""
from __future__ import annotations

import os
import re
import statistics

import numpy as np
import pytest

from conftest import built_scene
from test_gpu_parity import assert_accum_close
from test_render_sequences import FIELDS, PROFILES, SHADOW_EXACT, SHAPES, Sides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# profiles/boundary_idle_accounting.txt, section 1, last line ("Without a profiler the same seven pairs cost ... 4.5 us a pair"):
# what ONE stage's event pair adds to a step of an un-profiled run, which is what this test is.  One pair per timed stage launch.
ACCOUNTING = "profiles/boundary_idle_accounting.txt"
EVENT_IDLE_US_PER_LAUNCH = 4.5
STATE = ("primary_ray_cnt", "start_position", "shadow_ray_cnt", "n_live", "frame", "budget_remaining", "device_error")
TOTALS = ("total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible")


def small_ctx(hip, flags=0, **tuning):
    sc, nodes, prims = built_scene("cornell_soup2k")
    W, H = 96, 64
    g = hip.Renderer(W, H, W * H * 2, flags=(1 if sc.triangle_materials else 0) | flags)
    g.load_scene(sc, nodes, prims)
    g.set_tuning(**tuning)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("profile", list(PROFILES))
def test_twenty_steps_repeat_the_first(hip, profile):
    """set_frame(1), reset_accum, render(spp) twenty times: every step is the same job"""
    spp = 2
    g = small_ctx(hip, **PROFILES[profile])
    first, before = None, g.counters()
    for step in range(20):
        g.set_frame(1)
        g.reset_accum()
        it = g.render(spp)
        k = g.counters()
        seen = dict({f: k[f] for f in STATE}, iterations=it, **{f: k[f] - before[f] for f in TOTALS})
        before = k
        if first is None:
            first = seen
            assert first["device_error"] == 0 and first["total_primary_rays"] == spp * 96 * 64, first
        assert seen == first, (profile, step, {f: (first[f], seen[f]) for f in first if first[f] != seen[f]})
    fresh = small_ctx(hip, **PROFILES[profile])
    fresh.render(spp)
    assert_accum_close(fresh.blit_buffer(), g.blit_buffer(), f"[{profile}] step 20 against a fresh ctx's render")


def _sides(orc, hip, profile):
    W, H, N, rank, nranks = SHAPES["tight"]
    return Sides(orc, hip, built_scene("cornell_soup2k"), W, H, N, rank, nranks, profile)


def _both(s, name, *args):
    """one call on the oracle and on the HIP ctx, nothing read in between"""
    ro = getattr(s.o, name)(*args)
    rg = getattr(s.g, name)(*args)
    if name == "render":
        assert ro == rg, (s.tag(name), ro, rg)
        s.shadow_exact = s.profile in SHADOW_EXACT
    return rg


def seq_no_reset(s, peek):
    for _ in range(6):
        _both(s, "set_frame", 1), peek()
        _both(s, "render", 2), peek()


def seq_budget_twice(s, peek):
    odd = s.N - 37 if (s.N - 37) % 64 else s.N - 38
    for _ in range(3):
        _both(s, "set_frame", 1), peek()
        _both(s, "reset_accum"), peek()
        _both(s, "set_budget", 7), peek()
        _both(s, "set_budget", odd), peek()
        _both(s, "launch_kernels"), peek()
        s.shadow_exact = True
        _both(s, "launch_kernels"), peek()
        _both(s, "render", 1), peek()


def seq_after_cut_short(s, peek):
    _both(s, "render", 2, 2), peek()
    for _ in range(3):
        _both(s, "set_frame", 1), peek()
        _both(s, "reset_accum"), peek()
        _both(s, "render", 2), peek()
    _both(s, "render", 3, 1), peek()
    _both(s, "reset_accum"), peek()
    _both(s, "render", 0), peek()


def seq_steps(s, peek):
    for _ in range(4):
        _both(s, "set_frame", 1), peek()
        _both(s, "reset_accum"), peek()
        _both(s, "render", 2), peek()


SEQUENCES = {"no_reset": seq_no_reset, "budget_twice": seq_budget_twice, "after_cut_short": seq_after_cut_short, "steps": seq_steps}


@pytest.mark.gpu
@pytest.mark.parametrize("profile", list(PROFILES))
@pytest.mark.parametrize("counters_between", [False, True])
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_boundary_sequences_against_the_oracle(orc, hip, name, counters_between, profile):
    """bench-style steps with reset_accum omitted, the budget set twice, after a render cut short by max_iterations -- with nothing
    read between the calls, and with a counters() call between every two of them -- end where the oracle ends"""
    s = _sides(orc, hip, profile)
    s.g.set_tuning(stage_timing=1 if counters_between else 0)  # (the profiles that time their stages: both forms of the timing)

    def peek():
        if counters_between:
            ko, kg = s.o.counters(), s.g.counters()
            diff = {f: (ko[f], kg[f]) for f in FIELDS if ko[f] != kg[f]}
            assert kg["device_error"] == 0 and not diff, f"{s.tag(name)}: counters differ (oracle, HIP): {diff}"
        s.step += 1

    SEQUENCES[name](s, peek)
    s.check(name)


@pytest.mark.gpu
def test_stage_timing_attached_against_event_pairs(hip):
    """stage_timing 1 (events attached to the launches) against 0 (event pairs) on one ctx: the same launches per stage; per stage
    the new time is not above the pairs' and not below it by more than the idle the pairs add (EVENT_IDLE_US_PER_LAUNCH per
    launch, from ACCOUNTING) plus the pairs' own spread over five renders"""
    assert os.path.exists(os.path.join(ROOT, ACCOUNTING))
    sc, nodes, prims = built_scene("cornell_soup2k")
    W, H = 256, 256
    g = hip.Renderer(W, H, W * H * 2, flags=(1 if sc.triangle_materials else 0) | hip.TYR_FLAG_PROFILE)
    g.load_scene(sc, nodes, prims)

    def five(mode):
        g.set_tuning(stage_timing=mode)
        out = []
        for _ in range(6):
            g.set_frame(1)
            g.reset_accum()
            g.timings(reset=True)
            g.render(2)
            out.append(g.timings())
        return out[1:]  # (the first render after a change of mode warms the path up)

    five(0)
    ev, new = five(0), five(1)
    assert g.counters()["device_error"] == 0
    for stage in ev[0]:
        launches = [t[stage]["launches"] for t in ev]
        assert launches == [t[stage]["launches"] for t in new], (stage, launches, [t[stage]["launches"] for t in new])
        if launches[0] == 0:
            assert all(t[stage]["ms"] == 0.0 for t in new), stage
            continue
        e, n = [t[stage]["ms"] for t in ev], [t[stage]["ms"] for t in new]
        e_med, n_med, spread = statistics.median(e), statistics.median(n), max(e) - min(e)
        print(f"{stage}: {launches[0]} launches; event pairs {e_med:.4f} ms (spread {spread:.4f}), attached {n_med:.4f} ms (spread {max(n) - min(n):.4f})")
        assert n_med > 0.0, stage
        assert n_med <= e_med, (stage, n_med, e_med)
        assert n_med >= e_med - (launches[0] * EVENT_IDLE_US_PER_LAUNCH * 1e-3 + spread), (stage, n_med, e_med, spread)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_timings_are_zero_without_the_profile_flag(hip, mode):
    g = small_ctx(hip, stage_timing=mode)
    g.render(2)
    assert all(v["ms"] == 0.0 and v["launches"] == 0 for v in g.timings().values()), g.timings()


def _body(src, signature):
    at = src.index(signature)
    depth, i = 0, src.index("{", at)
    for j in range(i, len(src)):
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[i : j + 1]
    raise AssertionError(signature)


def test_reset_and_budget_do_not_wait_for_the_stream():
    """the round trips between two renders must not come back: tyr_reset_accum and tyr_set_budget neither synchronise the stream
    nor copy the whole counter struct, and the render loop's undo does not push it"""
    drv = open(os.path.join(ROOT, "tyrant_amd", "csrc", "host", "driver.cpp")).read()
    loop = open(os.path.join(ROOT, "tyrant_amd", "csrc", "host", "render_loop.cpp")).read()
    for sig in ("int tyr_reset_accum(tyr_ctx* c)", "int tyr_set_budget(tyr_ctx* c, uint64_t primary_rays)"):
        body = re.sub(r"//[^\n]*", "", _body(drv, sig))
        for banned in ("hipStreamSynchronize", "push_counters", "sync_counters", "hipDeviceSynchronize", "hipMemcpy("):
            assert banned not in body, (sig, banned)
    assert "push_counters" not in re.sub(r"//[^\n]*", "", loop)
    body = re.sub(r"//[^\n]*", "", _body(loop, "static int render_budget("))
    assert body.count("sync_counters(") == 1 and "hipStreamSynchronize" not in body
