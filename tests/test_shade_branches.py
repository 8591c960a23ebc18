"""The shade kernel on crafted rays that reach every branch (tests/shade_cases.py builds the scene and the batches).

Every other test of k_shade renders a stock scene from its camera; which of shade's branches those renders reach is recorded
nowhere.  Here the oracle's shade stage writes a per-record BRANCH TRACE (oracle/orc.h ORC_TR_*, test infrastructure only), the
CPU tests assert from the oracle alone that the batches reach what they are for, and the GPU tests hold k_shade to the oracle on
them: stage by stage and bit for bit (test_shade_stage_bit_for_bit), and through tyr_render / tyr_launch_kernels under the
sixteen settings of fold_spheres, resolve_shadows, retire_sky and fold_prologue (test_render_loop_folded_paths), whose
sphere pre-pass, resolved shadow rays and retired ghosts exist in the HIP kernel only.

Conditions asserted on the batch of 16,411 records of every flag set (0, 1, 1|16, 1|8, 1|8|16) and both pixel layouts, over two
iterations (the second shades the first one's survivors):
    every trace bit and conjunction of shade_cases.possible(flags) in >= 32 records of the shuffled batch;
    every one of them that the ray's geometry decides in a run of >= 64 consecutive slots of the sorted batch;
    ghost candidates, shadow rays blocked by a sphere, visible ones clear of the root box, ones blocked by a triangle: >= 32 each
    (after the first shade; "clear" = by 1e-2 units in float64).
Not reachable, and why:
    a triangle seen from behind (INSIDE with TRIANGLE; absorption in a REFR triangle): loader.h:28 culls back faces, extend
        never reports such a hit;
    the bits shade_cases.possible() leaves out per flag set (no palette without TYR_FLAG_TRIANGLE_COLORS, ...);
    a run of 64 for the bits a record's random numbers decide (which NEE branch, each rejection, Phong rounds, the roulette's
        draw, the emitter pick, the Fresnel pick): the seed changes with the slot, so sorting cannot line them up; they are
        held to >= 32 records in the sorted batch as well;
    frame 0: tyr_set_frame refuses it and the reference never has it (kernel.cu:736-739).  Every seed IS 0 in the batch at
        frame 2^31 on even pixels (frame * pixel = 0 modulo 2^32), and for pixel 0 and slot 0 of every batch.

The GPU comparisons.  Stage API: every batch (nine sizes, shuffled and sorted, at frame 1 and at frame 4,000,000,007; one of 255
records whose every seed is 0) through begin / import / primary / extend / shade / connect / end and a second iteration on the
survivors, on a ctx of its own per setting of merge_trace and kernel_snapshot.  The staged calls build their launch parameters
without the tuning record (host/driver.cpp make_params): none of TUNING_KEYS changes what enqueue_shade launches there, the two
knobs are run because a staged call must not depend on them.  A survivor's record on the device carries origin, direction,
throughput, pixel, bounces and lastSpecular (its hit fields are extend's to write): those are "all fields" of the survivor
queue; the shadow queue is compared byte for byte.  With one record per pixel the accumulation buffer is compared bit for bit
after shade and after connect (a pixel receives its terms in the same order on both sides); piled, by assert_accum_close.
Render loop: the folded paths add a record's terms to each other before they reach the pixel (a resolved shadow ray's colour, a
ghost's next miss), so there radiance is bit-exact only where the oracle shows a pixel to receive at most two terms over the run
(0 + a + b = 0 + (a + b) in floating point), and within the project's 1e-5 elsewhere.

Seed 0 and the Phong loop (decided: kept as the reference has it).  xorshift32 maps 0 to 0, so a record with seed 0 draws 0.0 for
ever; its Phong sample is the mirror direction itself, and `do ... while (dot(d, normal) <= epsilon)` (kernel.cu:523-536) does
not end when that direction lies within epsilon of the surface.  The reference, the oracle and k_shade agree on this, and the
project's contract is the reference's arithmetic bit for bit, so the loop is left alone; the batches keep records aimed at a
PHONG surface below cosine 0.05 away from zero seeds (shade_cases.batch), and every GPU test takes its expected values from the
oracle first, so nothing that does not end on the CPU reaches a GPU.
"""
import itertools

import numpy as np
import pytest

import shade_cases as sc
from conftest import bits

DRAWN = tuple(n for n in list(sc.TRACE_BITS) + [c[0] for c in sc.COMBOS] if n not in sc.GEOMETRIC + sc.GEOMETRIC_COMBOS)


# ---- CPU: the batches reach what they are for -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["one", "piled"])
@pytest.mark.parametrize("flags", sc.FLAG_SETS)
def test_batches_reach_every_branch(orc, flags, layout):
    reach, never = sc.possible(flags)
    assert set(reach) | set(never) == set(sc.TRACE_BITS) | {c[0] for c in sc.COMBOS}
    shuffled, srt = sc.batch(flags, sc.BIG, layout, "shuffled"), sc.batch(flags, sc.BIG, layout, "sorted")
    m = np.concatenate([it["trace"] for it in shuffled["iterations"]])
    ms = [it["trace"] for it in srt["iterations"]]
    counts = {name: int(sc.has(m, name).sum()) for name in reach}
    print(f"flags {flags} {layout}: " + " ".join(f"{k}={v}" for k, v in counts.items()))
    for name in reach:
        assert counts[name] >= 32, (flags, layout, name, counts[name])
        if name in DRAWN:
            assert sum(int(sc.has(x, name).sum()) for x in ms) >= 32, (flags, layout, "sorted", name)
        else:
            assert max(sc.longest_run(sc.has(x, name)) for x in ms) >= 64, (flags, layout, "sorted: no run of 64", name)
    for name in never:
        assert not sc.has(m, name).any(), (flags, name)
    assert not (sc.has(m, "TRIANGLE") & sc.has(m, "INSIDE")).any()  # back faces are culled
    folded = sc.folded_path_counts(flags, shuffled["iterations"][0])
    print(f"flags {flags} {layout}: {folded}")
    assert folded["visible"] == shuffled["iterations"][0]["visible"]  # the same verdicts as the oracle's connect
    for k in ("ghost_candidates", "blocked_by_sphere", "visible_clear_of_root", "blocked_by_triangle"):
        assert folded[k] >= 32, (flags, layout, k, folded[k])
    for it in shuffled["iterations"] + srt["iterations"]:
        assert np.isfinite(it["accum"]).all()


def test_batches_hold_the_asked_inputs():
    """every size: finite records, pixel 0 and the last pixel, slot 0, bounces in {0, 4, 5}; the throughput forms of the issue in the
    large batch; negative throughput only with one record per pixel; a zero seed for every record of the frame-2^31 batch"""
    for n in sc.SIZES:
        for layout in ("one", "piled"):
            b = sc.batch(0, n, layout, "shuffled")
            r = b["rays"]
            assert len(r) == n and np.isfinite(r["origin"]).all() and np.isfinite(r["direction"]).all() and np.isfinite(r["direct"]).all()
            assert set(np.unique(r["bounces"])) <= {0, 4, 5}
            if n > 1:
                assert 0 in r["index"] and b["W"] * b["H"] - 1 in r["index"] and r["index"].max() < b["W"] * b["H"]
            if layout == "one":
                assert len(np.unique(r["index"])) == n
            else:
                assert (r["direct"] >= 0).all() and len(np.unique(r["index"])) <= 5
    d = sc.batch(0, sc.BIG, "one", "shuffled")["rays"]["direct"]
    top = d.max(axis=1)
    eps = np.float32(1e-3)
    for what, sel in (("zero", (d == 0).all(axis=1)), ("epsilon", top == eps), ("below epsilon", top == np.nextafter(eps, np.float32(0))), ("above epsilon", top == np.nextafter(eps, np.float32(1))),
                      ("one", top == 1), ("above one", (top > 1) & (top < 10)), ("1e30", top == np.float32(1e30)), ("denormal", (top > 0) & (top < 1e-38)), ("negative", (d < 0).sum(axis=1) == 1)):
        assert sel.sum() >= 32, what
    z = sc.batch(0, 255, "one", "shuffled", sc.ZERO_SEED_FRAME)
    assert (sc.seeds(z["rays"], sc.ZERO_SEED_FRAME) == 0).all()
    assert (sc.seeds(sc.batch(0, sc.BIG, "one", "shuffled")["rays"], 1) == 0).sum() in (1, 2)  # pixel 0 and slot 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
ORDERS = ("shuffled", "sorted")
FRAMES = (1, sc.LARGE_FRAME)
STAGED_KNOBS = tuple(dict(merge_trace=m, kernel_snapshot=k) for m in (1, 0) for k in (1, 0))
FOLD_KNOBS = tuple(dict(fold_spheres=a, resolve_shadows=b, retire_sky=c, fold_prologue=d) for a, b, c, d in itertools.product((1, 0), repeat=4))
SHADOW_FIELDS = ("origin", "direction", "color", "closestDistance")


def new_renderer(hip, flags, b, **knobs):
    g = hip.Renderer(b["W"], b["H"], len(b["rays"]), flags=flags)
    sc.load(g, flags)
    g.set_tuning(**knobs)
    return g


def assert_accum(layout, want, got, what):
    from test_gpu_parity import assert_accum_close

    if layout == "one":  # a pixel receives 0 + colour, then + shadow colour, in the same order on both sides
        assert np.array_equal(bits(want), bits(got)), f"{what}: {np.count_nonzero(np.any(bits(want) != bits(got), axis=1))} pixels differ"
    else:
        assert_accum_close(want, got, what)


def check_staged(hip, flags, layout, b, frame, what):
    """two staged iterations of batch `b` on a ctx of its own per launch-shape setting, each held to the oracle's"""
    from test_gpu_parity import assert_state_equal

    for knobs in STAGED_KNOBS:
        g = new_renderer(hip, flags, b, **knobs)
        for i, want in enumerate(b["iterations"]):
            tag = f"{what} {knobs} iteration {i}"
            got = sc.staged_iteration(g, i == 0, b["rays"], frame)
            assert got["n_live"] == want["n_live"], tag
            qo, qg = want["extended"], got["extended"]
            assert np.array_equal(bits(qo["distance"]), bits(qg["distance"])), tag + ": extend distance"
            hit = qo["distance"] < sc.VERY_FAR
            assert np.array_equal(qo["identifier"][hit], qg["identifier"][hit]) and np.array_equal(qo["geometry_type"][hit], qg["geometry_type"][hit]), tag + ": extend identifier"
            for f in ("ns", "nh", "n_survive", "total_shadow_rays"):
                assert got[f] == want[f], (tag, f, want[f], got[f])
            assert got["device_error"] == 0, tag
            assert got["rank_check"] == (want["ns"], 0), (tag, "rank tables of the scan", got["rank_check"])
            assert_state_equal(want["survivors"], got["survivors"], tag + ": survivors")
            so, sg = want["shadows"], got["shadows"]
            for f in SHADOW_FIELDS:
                assert np.array_equal(bits(so[f]), bits(sg[f])), f"{tag}: shadow {f} differs in {np.count_nonzero(np.any(bits(so[f]) != bits(sg[f]), axis=-1))} records"
            assert np.array_equal(so["buffer_index"], sg["buffer_index"]), tag + ": shadow buffer_index"
            assert_accum(layout, want["accum_shade"], got["accum_shade"], tag + ": accumulation after shade")
            assert got["visible"] == want["visible"], (tag, "n_shadow_visible", want["visible"], got["visible"])
            assert_accum(layout, want["accum"], got["accum"], tag + ": accumulation after connect")
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("layout", ["one", "piled"])
@pytest.mark.parametrize("flags", sc.FLAG_SETS)
def test_shade_stage_bit_for_bit(orc, hip, flags, layout, frame):
    """k_shade alone against the oracle's shade on every size and order of the crafted batches: queues, counters, rank tables,
    accumulation (module docstring, "The GPU comparisons")"""
    for n in sc.SIZES:
        for order in ORDERS:
            check_staged(hip, flags, layout, sc.batch(flags, n, layout, order, frame), frame, f"flags {flags} {layout} {order} {n} frame {frame}")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", sc.FLAG_SETS)
def test_shade_stage_with_every_seed_zero(orc, hip, flags):
    """255 records, one per even pixel, at frame 2^31: every record draws 0.0 for every random number"""
    for order in ORDERS:
        b = sc.batch(flags, 255, "one", order, sc.ZERO_SEED_FRAME)
        assert (sc.seeds(b["rays"], sc.ZERO_SEED_FRAME) == 0).all()
        check_staged(hip, flags, "one", b, sc.ZERO_SEED_FRAME, f"flags {flags} zero seeds {order}")


def check_driven(hip, flags, layout, b, want, frame, what):
    """batch `b` through render(0) and through LAUNCHES launch_kernels under each of the sixteen settings of the folded paths:
    each against the oracle driven the same way, and all against the first"""
    from test_gpu_parity import assert_accum_close, assert_state_equal

    g = new_renderer(hip, flags, b)
    sc.prime(g)
    few = np.nonzero(want["addends"] <= 2)[0] if layout == "one" else np.zeros(0, dtype=np.int64)
    first = {}
    for knobs in FOLD_KNOBS:
        g.set_tuning(**knobs)
        for how in ("render", "launches"):
            tag = f"{what} {how} {knobs}"
            w, got = want[how], sc.drive(g, b["rays"], frame, how)
            assert got["device_error"] == 0, tag
            for f in ("iterations", "left", "frame") + sc.RENDER_FIELDS:
                assert got[f] == w[f], (tag, f, w[f], got[f])
            assert_accum_close(w["accum"], got["accum"], tag)
            assert np.array_equal(bits(w["accum"][few]), bits(got["accum"][few])), f"{tag}: {np.count_nonzero(np.any(bits(w['accum'][few]) != bits(got['accum'][few]), axis=1))} pixels of at most two terms differ"
            if how == "launches":
                assert_state_equal(w["queue"], got["queue"], tag + ": work queue")
            ref = first.setdefault(how, got)
            assert np.array_equal(ref["accum"][:, 3], got["accum"][:, 3]) and np.array_equal(bits(ref["accum"][few]), bits(got["accum"][few])), tag + ": against the first setting"
            assert np.allclose(got["accum"][:, :3], ref["accum"][:, :3], rtol=1e-5, atol=1e-6), tag + ": against the first setting"
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("layout", ["one", "piled"])
@pytest.mark.parametrize("flags", sc.FLAG_SETS)
def test_render_loop_folded_paths(orc, hip, flags, layout, frame):
    """the paths only the render loop runs -- shade's sphere pre-pass for the rays it emits, shadow rays answered in place, ghosts
    retired one iteration early -- on every size and order of the crafted batches (module docstring, "The GPU comparisons")"""
    for n in sc.SIZES:
        for order in ORDERS:
            want = sc.driven(flags, n, layout, order, frame)
            check_driven(hip, flags, layout, sc.batch(flags, n, layout, order, frame), want, frame, f"flags {flags} {layout} {order} {n} frame {frame}")
    big = sc.driven(flags, sc.BIG, layout, "shuffled", frame)
    assert big["launches"]["left"] >= 32 and big["render"]["iterations"] > sc.LAUNCHES, "the bounded drive leaves survivors to export"
