"""Call sequences that mix renders with refit, AOVs, motion vectors, the filters, sample maps and the allocator.

test_render_sequences.py holds the render loop to the oracle after every operation of `render, launch, staged, budget, reset,
camera, sun, import, query`.  The entry points added since then read or write the same hidden state, or keep state of their
own on the ctx: tyr_scene_refit swaps the geometry under work queued ahead, tyr_set_sample_map / tyr_render_adaptive are a MODE
with enter and leave rules and a ctx-owned ticket list that is regrown, tyr_render_aov / tyr_render_motion regenerate the
camera rays of the ctx's frame, tyr_denoise / tyr_temporal / tyr_svgf read the ctx's blit buffer when accum is NULL (the last
two keep a history), tyr_allocate_samples has ctx-owned scratch.  Here they join the alphabet: WideSides is Sides with

    refit            HIP Renderer.refit (host arrays and device arrays in turn); oracle: upload(refit_nodes(...), moved).
                     Own check: scene_hash == the hash of a fresh upload of the refitted tree.
    sample_map,      oracle side: tests/mapped_model.py, the oracle-only model of mapped mode (pinned by test_mapped_model.py).
    render_adaptive  While the model is in mapped mode launch and staged take its iteration; render and set_budget leave it.
    aov, motion      test_aov.expected_aov / test_temporal.expected_motion for the ctx's CURRENT frame, camera and (refitted)
                     geometry, from the restated camera rays traced by a scratch oracle ctx -- whatever mode the ctx is in:
                     the header defines both by the frame counter and the scan-line cursor at 0, not by the mode.
    denoise,         accum = None, launched right behind a render / render_adaptive with no read-back in between (`then=`) or
    temporal, svgf   on their own: bit for bit the numpy restatement on g.blit_buffer() and the guides the sequence made last;
                     the restatements' histories are carried from call to call.
    allocate         the map equals adaptive_ref.allocate on the ctx's rows; the caller may feed it to sample_map.
    frame            tyr_set_frame, the oracle's orc_set_frame: the seeds of what follows, 2^32 - 1 (the wrap past 0) included.

and after EVERY operation Sides.check(): FIELDS, the accumulation, the work queue, the shadow queue where shadow_exact.

The named sequences each reach one state a caller can produce, the random ones mix the old and the new alphabet with fixed
seeds (their own generator: test_render_sequences.random_ops keeps its cases); both run on every tuning profile.
test_wide_sequences_reach_their_states replays them on the oracle / model alone and asserts the states and the coverage.

Wall time on one MI355X, `pytest -m gpu`, measured in one session on the same machine (each module prints its own):
test_render_sequences.py, 168 cases, 2.0 s -- unchanged from the commit before this module; this module, 168 cases (12 named
and 12 random sequences on 7 profiles), 4.6 s.  The frames are SHAPES' (at most 37 x 23 pixels): the numpy restatements of the
filters and the model's per-ray Python loop are what the time goes to."""
from __future__ import annotations

import time

import numpy as np
import pytest

import adaptive_ref as ar
import denoise_ref
import svgf_ref
import temporal_ref
from conftest import bits, built_scene
from mapped_model import MappedOracle, maps
from test_render_sequences import FIELDS, MAX_BOUNCES, PROFILES, SCENES, SHADOW_EXACT, SHAPES, UNBOUNDED, COUNTED, Sides, dark_ground_scene

TYR_FLAG_REFIT = 64
OLD_OPS = ("render", "launch", "staged", "budget", "reset", "camera", "sun", "import", "query")
NEW_OPS = ("refit", "sample_map", "render_adaptive", "aov", "motion", "denoise", "temporal", "svgf", "allocate", "frame")
FILTERS = ("denoise", "temporal", "svgf")
MAP_KINDS = ("uniform1", "uniform2", "random", "sparse", "one_large", "zero")


def assert_bits(got, want, what):
    bad = bits(np.asarray(got)) != bits(np.asarray(want))
    if bad.ndim > 1:
        bad = bad.any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first {np.flatnonzero(bad)[:5]}"


class WideSides(Sides):
    """Sides over the wide alphabet.  `trace` keeps, per operation, its kind and the state it met: survivors held, mapped mode,
    the operation before it."""

    def __init__(self, orc, hip, scene, W, H, N, rank=0, nranks=1, profile="default"):
        super().__init__(orc, hip, scene, W, H, N, rank, nranks, profile, hip_flags=TYR_FLAG_REFIT)
        sc, nodes, prims = scene
        self.orc, self.hip = orc, hip
        self.flags = (1 if sc.triangle_materials else 0) | (8 if sc.light_list else 0) | (16 if sc.triangle_colors else 0)
        self.o = MappedOracle(self.o, sc.camera, rank, nranks)
        self.nodes0, self.prims0 = nodes, prims  # as uploaded: every refit deforms these (no drift), the tree keeps its shape
        self.nodes, self.prims = nodes, prims  # what both sides hold now
        self.geometry = 0  # counts the refits
        self.old_prims = None  # the records held before the refits since the last motion pass (its prev_prims)
        self.prev_cam = sc.camera  # the camera of the last motion pass (its prev_camera)
        self.guides = None  # the last aov pass: tensors, numpy copies, sample-0 rays and what they were made for
        self.mot = None  # the last motion pass
        self.hist = {"temporal": None, "svgf": None}  # the restatements' histories
        self.filtered = {k: 0 for k in FILTERS}  # calls compared
        self.kept = {"temporal": 0, "svgf": 0}  # pixels whose history a call took over
        self.device_refit = False
        self.k = 0
        self.trace = []

    # ---- bookkeeping ----
    def note(self, kind, **kw):
        self.k += 1  # (counts the caller's operations alike with and without a HIP ctx: the maps and deformations are seeded by it)
        k = self.o.counters()
        self.trace.append(dict(op=kind, surv=k["primary_ray_cnt"], mapped=self.o.mapped, tickets=self.o.T, budget=k["budget_remaining"], start=k["start_position"],
                               prev=self.trace[-1]["op"] if self.trace else None, refits=self.geometry, **kw))

    def map_of(self, kind):
        """a map of one of MAP_KINDS (or an array, taken as it is), seeded by the step"""
        if not isinstance(kind, str):
            return np.asarray(kind, np.int32), "given"
        return maps(self.H, self.W, np.random.default_rng(1000 + self.k))[kind], kind

    # ---- the old alphabet, traced (the filters can ride behind a render: `then`) ----
    def _render_like(self, name, kind, spp, fo, fg_call, max_iterations, then):
        """a render on both sides.  `spp` goes into `renders` for check_loop: a mapped render is entered as 0, so that it is held to
        its profile's launch counts but does not arm check_loop's "some render folded a prologue" proof -- a map whose tickets
        last to the render's end (one pixel with thousands) tops up in every iteration and has no prologue to fold"""
        t0 = self.g.timings() if self.g is not None and self.profile in COUNTED else None
        launched = {}

        def fg():
            it = fg_call()
            if then is not None:
                launched["out"] = self.launch_filter(*then)  # right behind the render: no counter or buffer is read in between
            if t0 is not None:
                t1 = self.g.timings()
                self.renders.append((spp, max_iterations, it, {k: t1[k]["launches"] - t0[k]["launches"] for k in ("primary", "extend", "connect")}))
            return it

        if max_iterations:
            self.shadow_exact = self.profile in SHADOW_EXACT
        if then is not None and self.g is not None:
            self.need_guides()
        it = self._do(name, fo, fg, returns=True)
        if it:
            self.own_scan = self.o.counters()["primary_ray_cnt"] > 0
        if then is not None:
            self.note(then[0], behind=kind)
            if self.g is not None:
                self.compare_filter(then[0], launched["out"], *then[1:])
                self.check(f"{then[0]} behind {kind}")
            self.step += 1
        return it

    def render(self, spp, max_iterations=UNBOUNDED, then=None):
        self.note("render", spp=spp, max_iterations=max_iterations)
        mi = "unbounded" if max_iterations == UNBOUNDED else max_iterations
        return self._render_like(f"render({spp}, {mi})", "render", spp, lambda: self.o.render(spp, 1 << 30 if max_iterations == UNBOUNDED else max_iterations),
                                 lambda: self.g.render(spp, max_iterations), max_iterations, then)

    def launch(self):
        self.note("launch")
        super().launch()

    def staged(self):
        self.note("staged")
        super().staged()

    def set_budget(self, n):
        self.note("budget")
        super().set_budget(n)

    def reset_accum(self):
        self.note("reset")
        super().reset_accum()

    def set_camera(self):
        self.note("camera")
        super().set_camera()

    def set_sun(self):
        self.note("sun")
        super().set_sun()

    def import_queue(self):
        self.note("import")
        super().import_queue()

    def query(self):
        self.note("query")
        super().query()

    # ---- the new alphabet ----
    def refit(self):
        from test_scene_refit import deform, expected_hash, held_hash, refit_nodes, tri_bboxes

        self.note("refit")
        moved = deform(self.prims0, amp=0.5 + 0.5 * (self.k % 3), seed=self.k)
        want = refit_nodes(self.nodes0, tri_bboxes(moved))

        def fg():
            self.device_refit = not self.device_refit
            if self.device_refit:
                import torch

                got = self.g.refit(torch.from_numpy(np.ascontiguousarray(moved).view(np.uint8).reshape(-1).copy()).to(f"cuda:{self.g.device}"), want_nodes=True)
            else:
                got = self.g.refit(moved, want_nodes=True)
            assert got.tobytes() == want.tobytes(), self.tag("refit: nodes_out")

        if self.old_prims is None:
            self.old_prims = self.prims
        self.nodes, self.prims = want, moved
        self.geometry += 1
        self._do("refit", lambda: self.o.upload(want, moved), fg)
        if self.g is not None:
            assert held_hash(self.g) == expected_hash(self.hip, want, moved, False), self.tag("refit: the held scene is not the upload of the refitted tree")

    def set_frame(self, frame):
        """tyr_set_frame / orc_set_frame: the next iteration, and the AOV and motion passes from here on, run at `frame`"""
        self.note("frame", frame=frame)
        self._do(f"set_frame({frame})", lambda: self.o.set_frame(frame), lambda: self.g.set_frame(frame))

    def sample_map(self, kind):
        m, what = self.map_of(kind)
        self.note("sample_map", map=what)
        return self._do(f"set_sample_map({what})", lambda: self.o.set_sample_map(m), lambda: self.g.set_sample_map(m), returns=True)

    def render_adaptive(self, kind, max_iterations=UNBOUNDED, then=None):
        m, what = self.map_of(kind)
        self.note("render_adaptive", map=what, max_iterations=max_iterations)
        mi = "unbounded" if max_iterations == UNBOUNDED else max_iterations
        return self._render_like(f"render_adaptive({what}, {mi})", "render_adaptive", 0, lambda: self.o.render_adaptive(m, 1 << 30 if max_iterations == UNBOUNDED else max_iterations),
                                 lambda: self.g.render_adaptive(m, max_iterations), max_iterations, then)

    def camera_records(self, spp):
        """the records of tyr_render_aov's samples in ticket order (sample i // P of local pixel i % P at launch index i, the
        scan-line cursor at 0) at the ctx's frame and camera, traced by a scratch oracle ctx holding the ctx's geometry"""
        from tyrant_amd.scenes import RAY_DTYPE

        P = self.W * (self.H // self.nranks)
        n = spp * P
        i = np.arange(n)
        origin, direction, index = ar.camera_rays(self.orc.lib(), self.o.cam, self.W, self.H, i % P, i, self.o.counters()["frame"], self.rank, self.nranks)
        q = np.zeros(n, RAY_DTYPE)
        q["origin"], q["direction"], q["index"] = origin, direction, index
        q["direct"], q["geometry_type"], q["lastSpecular"] = 1.0, 1, 1
        so = self.orc.Oracle(self.W, self.H, n, rank=self.rank, nranks=self.nranks, flags=self.flags)
        so.load_scene(self.sc, self.nodes, self.prims)
        so.set_budget(0)
        so.stage("begin")
        so.import_work_queue(q, n)
        so.stage("primary")
        so.stage("extend")
        q = so.ray_queue(0, n)
        so.close()
        return q

    def guides_key(self):
        return (self.o.counters()["frame"], self.o.cam, self.geometry)

    def aov(self, spp=1, nested=False):
        from test_aov import assert_aov_equal, expected_aov

        if not nested:
            self.note("aov", spp=spp)
        if self.g is None:
            self.log.append(dict(op="aov", before=None, after=self.o.counters(), ret=None))
            return
        tag = self.tag(f"render_aov({spp})")
        res = self.g.render_aov(spp)
        q = self.camera_records(spp)
        pix, want = expected_aov(self.hip, q, self.sc, self.prims, np.ascontiguousarray(self.sc.spheres), spp, self.W, self.H, self.sc.triangle_colors)
        n = self.W * self.H
        got = {k: v.cpu().numpy().reshape((n, 3) if k in ("albedo", "normal") else (n,)) for k, v in res.items()}
        assert_aov_equal(got, pix, want, tag)
        other = np.ones(n, bool)
        other[pix] = False
        assert not np.any(got["depth"][other]) and not np.any(got["albedo"][other]), tag + ": rows of other ranks written"
        self.guides = dict(res=res, np=got, q0=q[: q.shape[0] // spp], key=self.guides_key())
        self.mot = None
        self.log.append(dict(op="aov", before=None, after=self.o.counters(), ret=None))
        self.check(f"render_aov({spp})")
        self.step += 1

    def motion(self, nested=False):
        from test_temporal import check_motion, expected_motion

        if not nested:
            self.note("motion")
        if self.g is None:
            self.log.append(dict(op="motion", before=None, after=self.o.counters(), ret=None))
            return
        if self.guides is None or self.guides["key"] != self.guides_key():
            self.aov(1, nested=True)  # prim and geom "as tyr_render_aov wrote them at this camera and frame"
        tag = self.tag("render_motion")
        cam, prev, old = self.o.cam, self.prev_cam, self.old_prims
        res = self.g.render_motion(self.guides["res"]["prim"], self.guides["res"]["geom"], prev, prev_prims=old)
        want = expected_motion(self.hip, self.g, self.guides["q0"], self.prims, np.ascontiguousarray(self.sc.spheres), cam, prev, self.W, self.H, old=old)
        check_motion(res, want, self.W, self.H, tag)
        if prev == cam and old is None:
            assert not np.any(res["motion"].cpu().numpy()), tag + ": an unchanged view moves"
        self.mot = dict(res=res, np={k: v.cpu().numpy() for k, v in res.items()})
        self.prev_cam, self.old_prims = cam, None
        self.log.append(dict(op="motion", before=None, after=self.o.counters(), ret=None))
        self.check("render_motion")
        self.step += 1

    def need_guides(self):
        if self.guides is None:
            self.aov(1, nested=True)
        if self.mot is None:
            self.motion(nested=True)

    def launch_filter(self, kind, reset=False):
        a, m = self.guides["res"], self.mot["res"]
        if kind == "denoise":
            return self.g.denoise(a["albedo"], a["normal"], a["depth"])
        if kind == "temporal":
            return self.g.temporal(a["albedo"], a["normal"], a["depth"], m["motion"], m["prev_depth"], reset=reset, want_history_len=True)
        return self.g.svgf(a["albedo"], a["normal"], a["depth"], m["motion"], m["prev_depth"], reset=reset, want_variance=True)

    def compare_filter(self, kind, out, reset=False):
        tag = self.tag(kind + (" (reset)" if reset else ""))
        W, H = self.W, self.H
        accum = self.g.blit_buffer()
        a, n, z = (self.guides["np"][k] for k in ("albedo", "normal", "depth"))
        if kind == "denoise":
            assert_bits(out.cpu().numpy().reshape(-1, 4), denoise_ref.denoise(accum, a, n, z, W, H), tag)
        else:
            m, pd = self.mot["np"]["motion"], self.mot["np"]["prev_depth"]
            ref = temporal_ref.temporal if kind == "temporal" else svgf_ref.svgf
            want, second, hist = ref(accum, a, n, z, m, pd, None if reset else self.hist[kind], W, H)
            assert_bits(out[0].cpu().numpy().reshape(-1, 4), want, tag)
            assert_bits(out[1].cpu().numpy().reshape(-1), second, tag + (": history length" if kind == "temporal" else ": variance"))
            if self.hist[kind] is not None and not reset:
                self.kept[kind] += int((hist.hu[:, 3] > 1).sum())
            self.hist[kind] = hist
        self.filtered[kind] += 1

    def filter(self, kind, reset=False):
        self.note(kind, reset=reset)
        self.log.append(dict(op=kind, before=None, after=self.o.counters(), ret=None))
        if self.g is None:
            return
        self.need_guides()
        self.compare_filter(kind, self.launch_filter(kind, reset), reset)
        self.check(kind)
        self.step += 1

    def allocate(self, total, min_spp=0, max_spp=6):
        """a map from the oracle's own frame (a sample's brightness as the error: both sides and the CPU replay see the same
        field); returns the full-frame map, the ctx's rows filled"""
        self.note("allocate")
        err = ar.two_buffer_error(self.o.blit_buffer(), np.zeros((self.W * self.H, 4), np.float32)).reshape(self.H, self.W)
        want, _ = ar.allocate(ar.local_rows(err, self.rank, self.nranks), total, min_spp, max_spp)
        full = np.zeros((self.H, self.W), np.int32)
        full[self.rank::self.nranks] = want.reshape(-1, self.W)
        self.log.append(dict(op="allocate", before=None, after=self.o.counters(), ret=int(want.sum())))
        if self.g is not None:
            m, got = self.g.allocate_samples(err, total, min_spp=min_spp, max_spp=max_spp)
            assert np.array_equal(m.cpu().numpy(), full), self.tag("allocate_samples: the map")
            assert got == int(want.sum()), self.tag("allocate_samples: the total")
            self.check("allocate_samples")
            self.step += 1
        return full


# ---- the named sequences ----
def seq_mapped_with_survivors(s):
    """1. render(2, 2), sample_map(random), launch x 3, render_adaptive(random): mapped mode entered with survivors held"""
    s.render(2, 2), s.sample_map("random"), s.launch(), s.launch(), s.launch(), s.render_adaptive("random")


def seq_list_shrinks_and_regrows(s):
    """2. render_adaptive(m, 2), render_adaptive(m', unbounded) with T' < T, then T'' > the list's capacity: the list is
    replaced mid-map by a shorter one, then regrown"""
    s.render_adaptive("uniform2", 2), s.render_adaptive("sparse"), s.render_adaptive(s.map_of("random")[0] + 2), s.render_adaptive("sparse", 1), s.staged()


def seq_render_leaves_the_mode(s):
    """3. sample_map(m), launch, render(1): tyr_render leaves the mode from the middle of a map; then render_adaptive(uniform 1)
    twice -- the first from wherever the cursor stands, the second from start_position == 0 or not, as the model says"""
    s.sample_map("random"), s.launch(), s.render(1), s.render_adaptive("uniform1"), s.render_adaptive("uniform1"), s.render(1)


def seq_budget_leaves_the_mode(s):
    """4. sample_map(m), launch, set_budget(odd), launch x 3: tyr_set_budget leaves the mode"""
    s.sample_map("random"), s.launch()
    s.set_budget(s.N - 37 if (s.N - 37) % 64 else s.N - 38)
    s.launch(), s.launch(), s.launch()


def seq_empty_maps(s):
    """5. render_adaptive(all zero) on a fresh ctx, after a finished render and with survivors held: render(0)'s three states"""
    s.render_adaptive("zero"), s.render(2), s.render_adaptive("zero"), s.render(2, 2), s.render_adaptive("zero"), s.render(1), s.staged()


def seq_refit_under_survivors(s):
    """6. render(2, 2), refit, aov, render(2), refit, render_adaptive(m): refit under survivors, twice, into mapped mode"""
    s.render(2, 2), s.refit(), s.aov(2), s.render(2, 2), s.refit(), s.render_adaptive("random")


def seq_denoising_pipeline(s):
    """7. four frames of INTEGRATION.md 4g: (camera move | refit), aov, motion, render(1) with svgf right behind it, temporal,
    denoise; histories checked every frame, across the camera move, the refit and a reset flag"""
    for k in range(4):
        if k in (1, 3):
            s.set_camera()
        if k == 2:
            s.refit()
        s.reset_accum()
        s.aov(1), s.motion()
        s.render(1, then=("svgf", False))
        s.filter("temporal", reset=(k == 3))
        s.filter("denoise")


def seq_filters_on_a_cut_render(s):
    """8. render(2, 2) with denoise right behind it, temporal, svgf (each reads the blit buffer of a cut render), render(0)"""
    s.aov(1), s.motion()
    s.render(2, 2, then=("denoise",)), s.filter("temporal"), s.filter("svgf"), s.render(0, then=("svgf", False)), s.filter("temporal")


def seq_adaptive_loop_on_a_shard(s):
    """9. INTEGRATION.md 4h on rank 1 of 3: render(1), allocate, render_adaptive(that map), allocate from the new buffer,
    render_adaptive"""
    P = s.W * (s.H // s.nranks)
    s.render(1)
    s.render_adaptive(s.allocate(2 * P, min_spp=1, max_spp=9))
    s.render_adaptive(s.allocate(3 * P + 17, min_spp=0, max_spp=5), then=("denoise",))


def seq_passes_back_to_back(s):
    """10. query, refit, aov, query, refit, motion back to back with no render between: the shared ticket words, the refit's wait"""
    s.render(1, 1), s.query(), s.refit(), s.aov(3), s.query(), s.refit(), s.motion(), s.query(), s.render(1)


def seq_early_ending_mapped(s):
    """11. on the scene whose renders end before kMaxBounces iterations: render_adaptive(uniform 1) and (all zero) alternating"""
    for _ in range(6):
        s.render_adaptive("uniform1"), s.render_adaptive("zero")


def seq_frame_counter(s):
    """12. render(1, 2), set_frame(2^32 - 1), aov, launch (the counter wraps past 0), motion, render_adaptive(random) with svgf
    behind it, set_frame(7), render(1): the passes and the mapped rays are seeded by the counter the caller set"""
    s.render(1, 2), s.set_frame(0xFFFFFFFF), s.aov(2), s.launch(), s.motion(), s.render_adaptive("random", then=("svgf", False)), s.set_frame(7), s.aov(1), s.render(1)


NAMED = {
    "mapped_with_survivors": (seq_mapped_with_survivors, "tight"),
    "list_shrinks_and_regrows": (seq_list_shrinks_and_regrows, "tight"),
    "render_leaves_the_mode": (seq_render_leaves_the_mode, "tight"),
    "budget_leaves_the_mode": (seq_budget_leaves_the_mode, "tight"),
    "empty_maps": (seq_empty_maps, "tight"),
    "refit_under_survivors": (seq_refit_under_survivors, "tight"),
    "denoising_pipeline": (seq_denoising_pipeline, "fits"),
    "filters_on_a_cut_render": (seq_filters_on_a_cut_render, "tight"),
    "adaptive_loop_on_a_shard": (seq_adaptive_loop_on_a_shard, "shard"),
    "passes_back_to_back": (seq_passes_back_to_back, "tight"),
    "early_ending_mapped": (seq_early_ending_mapped, "dark16"),
    "frame_counter": (seq_frame_counter, "tight"),
}


def named_sides(orc, hip, name, profile):
    fn, where = NAMED[name]
    if where == "dark16":
        return fn, WideSides(orc, hip, dark_ground_scene(), 16, 16, 256, profile=profile)
    W, H, N, rank, nranks = SHAPES[where]
    return fn, WideSides(orc, hip, built_scene("cornell_soup2k"), W, H, N, rank, nranks, profile)


# ---- the random sequences ----
N_RANDOM = 12  # per profile: every scene with every shape
_WEIGHTS = {"render": 4, "launch": 2, "staged": 1, "budget": 1, "reset": 1, "camera": 1, "sun": 1, "import": 1, "query": 1,
            "refit": 3, "sample_map": 3, "render_adaptive": 3, "aov": 1, "motion": 1, "denoise": 1, "temporal": 1, "svgf": 1, "allocate": 1, "frame": 1}


def wide_ops(seed, N):
    """9 to 13 operations over the old and the new alphabet"""
    rng = np.random.default_rng(seed)
    odd_budget = N - 37 if (N - 37) % 64 else N - 38
    names = [k for k, w in _WEIGHTS.items() for _ in range(w)]
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]  # noqa: E731
    ops = []
    for _ in range(int(rng.integers(9, 14))):
        k = str(rng.choice(names))
        then = None
        if k in ("render", "render_adaptive") and rng.random() < 0.25:
            f = pick(FILTERS)
            then = (f,) if f == "denoise" else (f, bool(rng.random() < 0.2))
        if k == "render":
            ops.append(("render", int(rng.integers(0, 4)), pick([0, 1, 2, 3, UNBOUNDED]), then))
        elif k == "render_adaptive":
            ops.append(("render_adaptive", pick(MAP_KINDS), pick([1, 2, 3, UNBOUNDED, UNBOUNDED]), then))
        elif k == "sample_map":
            ops.append(("sample_map", pick(MAP_KINDS)))
        elif k == "budget":
            ops.append(("budget", pick([0, odd_budget, N + 37])))
        elif k == "aov":
            ops.append(("aov", int(rng.integers(1, 4))))
        elif k in ("temporal", "svgf"):
            ops.append((k, bool(rng.random() < 0.2)))
        elif k == "allocate":
            ops.append(("allocate", int(rng.integers(1, 4)), bool(rng.random() < 0.6)))
        elif k == "frame":
            ops.append(("frame", pick([1, 7, 123456789, 0xFFFFFFFF])))
        else:
            ops.append((k,))
    return ops


def run_wide(s, ops):
    for op in ops:
        k = op[0]
        if k == "render":
            s.render(op[1], op[2], then=op[3])
        elif k == "render_adaptive":
            s.render_adaptive(op[1], op[2], then=op[3])
        elif k == "sample_map":
            s.sample_map(op[1])
        elif k == "budget":
            s.set_budget(op[1])
        elif k == "aov":
            s.aov(op[1])
        elif k == "frame":
            s.set_frame(op[1])
        elif k == "denoise":
            s.filter("denoise")
        elif k in ("temporal", "svgf"):
            s.filter(k, reset=op[1])
        elif k == "allocate":
            m = s.allocate(op[1] * s.W * (s.H // s.nranks) + 5)
            if op[2]:
                s.sample_map(m)
        else:
            {"launch": s.launch, "staged": s.staged, "reset": s.reset_accum, "camera": s.set_camera, "sun": s.set_sun, "import": s.import_queue,
             "query": s.query, "refit": s.refit, "motion": s.motion}[k]()


def wide_case(orc, hip, profile, i):
    p = list(PROFILES).index(profile)
    scene = SCENES[i % len(SCENES)]  # (i in range(12): every pair of a scene and a shape)
    shape = list(SHAPES)[i % len(SHAPES)]
    W, H, N, rank, nranks = SHAPES[shape]
    seed = 104729 * (p + 1) + i
    return WideSides(orc, hip, built_scene(scene), W, H, N, rank, nranks, profile), wide_ops(seed, N), f"{scene} {shape} seed {seed}"


# ---- the tests ----
@pytest.fixture(scope="module")
def wall_time(request):
    t0 = time.perf_counter()
    yield
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    capman = request.config.pluginmanager.get_plugin("capturemanager")
    if tr is not None and capman is not None:
        with capman.global_and_fixture_disabled():
            tr.write_line(f"test_call_sequences: {time.perf_counter() - t0:.1f} s wall time")


@pytest.mark.gpu
@pytest.mark.parametrize("profile", list(PROFILES))
@pytest.mark.parametrize("name", list(NAMED))
def test_named_wide_sequence(orc, hip, wall_time, name, profile):
    fn, s = named_sides(orc, hip, name, profile)
    fn(s)
    s.check_loop()
    if name == "denoising_pipeline":
        assert s.filtered == {"denoise": 4, "temporal": 4, "svgf": 4}, s.filtered
        assert s.kept["svgf"] > 0 and s.kept["temporal"] > 0, s.kept  # (a history was really taken over across the frames)
    if name == "filters_on_a_cut_render":
        assert s.filtered == {"denoise": 1, "temporal": 2, "svgf": 2}, s.filtered


@pytest.mark.gpu
@pytest.mark.parametrize("profile", list(PROFILES))
@pytest.mark.parametrize("i", range(N_RANDOM))
def test_random_wide_sequence(orc, hip, wall_time, profile, i):
    s, ops, what = wide_case(orc, hip, profile, i)
    print(what, ops)
    run_wide(s, ops)
    s.check_loop()


def test_wide_sequences_reach_their_states(orc):
    """the named sequences on the oracle / model alone: each still reaches the state it is named for; and the random set
    covers what it is there for"""

    def run(name):
        fn, s = named_sides(orc, None, name, "default")
        fn(s)
        return s, s.trace

    P = SHAPES["tight"][0] * SHAPES["tight"][1]
    # 1: the map arrives with survivors held, the launches are mapped, and the second map replaces the first in mid-list
    s, t = run("mapped_with_survivors")
    assert t[1]["op"] == "sample_map" and t[1]["surv"] > 0 and not t[1]["mapped"]
    assert all(e["op"] == "launch" and e["mapped"] and e["surv"] > 0 for e in t[2:5])
    assert t[5]["op"] == "render_adaptive" and t[5]["mapped"] and 0 < t[5]["budget"] < t[5]["tickets"] and t[5]["surv"] > 0
    k = s.o.counters()
    assert k["budget_remaining"] == 0 and k["primary_ray_cnt"] == 0
    # 2: cut after two iterations with tickets left; a shorter list; then one longer than any before; then a shorter one again
    s, t = run("list_shrinks_and_regrows")
    T = [e["tickets"] for e in t]
    assert t[1]["mapped"] and t[1]["budget"] > 0 and t[1]["surv"] > 0, "the first map is not cut in its middle"
    assert T[1] == 2 * P and T[2] < T[1] and T[3] > T[1] and s.o.T < T[3], T
    assert t[4]["op"] == "staged" and t[4]["mapped"] and t[4]["surv"] > 0
    # 3: render leaves the mode in mid-map; the uniform maps after it start at start_position != 0 and == 0
    s, t = run("render_leaves_the_mode")
    assert t[2]["op"] == "render" and t[2]["mapped"] and 0 < t[2]["budget"] < t[2]["tickets"] and t[2]["surv"] > 0
    assert not t[3]["mapped"] and t[3]["op"] == "render_adaptive" and t[3]["start"] != 0, t[3]
    assert t[4]["start"] == t[3]["start"], "a whole sample per pixel moves the cursor"
    assert t[5]["op"] == "render" and t[5]["mapped"] and t[5]["budget"] == 0
    # 4: set_budget leaves the mode in mid-map, with an odd budget, and the launches after it are raster launches
    s, t = run("budget_leaves_the_mode")
    assert t[2]["op"] == "budget" and t[2]["mapped"] and 0 < t[2]["budget"] < t[2]["tickets"] and t[2]["surv"] > 0
    assert all(e["op"] == "launch" and not e["mapped"] for e in t[3:]) and t[3]["budget"] % 64 != 0 and 0 < t[3]["budget"] < s.N
    # 5: the empty map meets a fresh ctx, a finished render and survivors
    s, t = run("empty_maps")
    z = [e for e in t if e["op"] == "render_adaptive"]
    assert [e["map"] for e in z] == ["zero"] * 3
    assert z[0]["surv"] == 0 and z[0]["start"] == 0 and z[1]["surv"] == 0 and z[1]["budget"] == 0 and z[2]["surv"] > 0 and z[2]["budget"] > 0
    r = [e for e in s.log if e["op"].startswith("render_adaptive")]
    assert r[0]["ret"] == 1 and r[1]["ret"] == 1 and r[2]["ret"] >= 2
    # 6: both refits meet survivors; the second render carries them into the mapped render
    s, t = run("refit_under_survivors")
    rf = [e for e in t if e["op"] == "refit"]
    assert len(rf) == 2 and all(e["surv"] > 0 for e in rf)
    assert t[-1]["op"] == "render_adaptive" and t[-1]["surv"] > 0 and t[-1]["refits"] == 2 and t[2]["op"] == "aov" and t[2]["surv"] > 0
    # 7: four frames, every filter on each, a camera move, a refit and a reset among them
    s, t = run("denoising_pipeline")
    ops = [e["op"] for e in t]
    assert ops.count("svgf") == ops.count("temporal") == ops.count("denoise") == ops.count("aov") == ops.count("motion") == 4
    assert ops.count("camera") == 2 and ops.count("refit") == 1 and sum(bool(e.get("reset")) for e in t) == 1
    assert all(e.get("behind") == "render" for e in t if e["op"] == "svgf")
    # 8: the filters read a cut render's buffer (survivors held, budget left), then an empty render's
    s, t = run("filters_on_a_cut_render")
    f = [e for e in t if e["op"] in FILTERS]
    assert [e["op"] for e in f] == ["denoise", "temporal", "svgf", "svgf", "temporal"]
    assert all(e["surv"] > 0 and e["budget"] > 0 for e in f[:3]) and f[0].get("behind") == "render" and f[3].get("behind") == "render"
    # 9: a shard; both maps come from the allocator, the second from the buffer the first render left; neither is uniform
    s, t = run("adaptive_loop_on_a_shard")
    assert (s.rank, s.nranks) == (1, 3)
    ra = [e for e in t if e["op"] == "render_adaptive"]
    al = [e for e in s.log if e["op"] == "allocate"]
    Pl = s.W * (s.H // 3)
    assert len(ra) == 2 and ra[0]["map"] == "given" and Pl < al[0]["ret"] <= 2 * Pl and al[1]["ret"] <= 3 * Pl + 17 and al[1]["ret"] > Pl
    assert ra[1]["mapped"] and ra[1]["budget"] == 0
    count = s.o.blit_buffer()[:, 3].reshape(s.H, s.W)
    assert not np.any(count[0::3]) and not np.any(count[2::3]) and len(np.unique(count[1::3])) > 2
    # 10: the passes and the refits follow each other with survivors held and no render between
    s, t = run("passes_back_to_back")
    ops = [e["op"] for e in t]
    assert ops[1:8] == ["query", "refit", "aov", "query", "refit", "motion", "query"] and all(e["surv"] > 0 for e in t[1:8])
    # 11: mapped renders that end before kMaxBounces iterations
    s, t = run("early_ending_mapped")
    r = [e for e in s.log if e["op"].startswith("render_adaptive(uniform1")]
    assert len(r) == 6 and sum(e["ret"] < MAX_BOUNCES + 1 for e in r) >= 2
    assert any(e["ret"] < MAX_BOUNCES + 1 and e["after"]["shadow_ray_cnt"] > 0 for e in r)
    # 12: the counter is set with survivors held, wraps in the launch behind the AOV pass, and is set again behind a mapped render
    s, t = run("frame_counter")
    fr = [e for e in s.log if e["op"].startswith("set_frame")]
    assert t[1]["op"] == "frame" and t[1]["surv"] > 0 and fr[0]["after"]["frame"] == 0xFFFFFFFF
    ln = [e for e in s.log if e["op"] == "launch_kernels()"][0]
    assert ln["before"]["frame"] == 0xFFFFFFFF and ln["after"]["frame"] == 1
    assert fr[1]["before"]["frame"] > 2 and fr[1]["after"]["frame"] == 7 and t[6]["mapped"]

    # the random sequences
    seen, with_surv, after_refit, enter, left = set(), set(), set(), 0, {"render": 0, "budget": 0, "sample_map": 0, "render_adaptive": 0}
    for profile in PROFILES:
        for i in range(N_RANDOM):
            s, ops, what = wide_case(orc, None, profile, i)
            run_wide(s, ops)
            seen.add(what.split()[0]), seen.add(what.split()[1])
            refit_seen = False
            for e in s.trace:
                seen.add(e["op"])
                if e["surv"] > 0:
                    with_surv.add(e["op"])
                if refit_seen:
                    after_refit.add(e["op"])
                refit_seen = refit_seen or e["op"] == "refit"
                if e["op"] in ("sample_map", "render_adaptive") and e["surv"] > 0 and not e["mapped"]:
                    enter += 1
                if e["mapped"] and e["op"] in left and (e["op"] in ("render", "budget") or e["budget"] > 0):
                    left[e["op"]] += 1
    assert seen >= set(SCENES) | set(SHAPES) | set(OLD_OPS) | set(NEW_OPS), (set(OLD_OPS) | set(NEW_OPS)) - seen
    assert with_surv >= set(NEW_OPS), set(NEW_OPS) - with_surv
    assert after_refit >= set(NEW_OPS) - {"refit"}, set(NEW_OPS) - after_refit
    assert enter > 0 and left["render"] > 0 and left["budget"] > 0 and left["sample_map"] + left["render_adaptive"] > 0, (enter, left)
