"""Call sequences of the render loop against the oracle.

tyr_render (host/render_loop.cpp) queues iteration i + 1 before iteration i's counts reach the host and steers by state
that lives across iterations and across calls: the folded prologue, the carried slot scan, the deferred shadow rays, the
undo of an empty look-ahead iteration.  The oracle's orc_render is a plain loop of orc_launch_kernels with none of that
state, so it is the specification: every operation below is applied to an oracle ctx and to a HIP ctx on the same scene,
and after EVERY operation the two must agree -- the iteration count a render returns, the counters, the accumulation
buffer (path counts exact, radiance within 1e-5 relative), the work queue bit for bit and, where the HIP ctx queues every
shadow ray, the shadow queue bit for bit.

Each named sequence reaches one state a caller can produce (a render on an empty ctx, survivors carried into a render,
a budget that is not a multiple of 64, ...); the fixed-seed random sequences mix the same operations over three scenes
and four frame / queue shapes.  Both run on every tuning profile, since each one drives a different host path.
test_named_sequences_reach_their_states runs the named sequences on the oracle alone (no GPU) and checks that each one
still reaches the state it is named for."""
from __future__ import annotations

import dataclasses
import time

import numpy as np
import pytest

from conftest import bits, built_scene
from test_gpu_parity import assert_accum_close, assert_state_equal

UNBOUNDED = 0xFFFFFFFF
MAX_BOUNCES = 5  # kMaxBounces, kernel.cu:16
FIELDS = ("primary_ray_cnt", "start_position", "shadow_ray_cnt", "n_live", "frame", "budget_remaining", "total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible")
SHADOW_FIELDS = ("origin", "direction", "color", "closestDistance")
FLAG_PROFILE = 2  # TYR_FLAG_PROFILE: per-stage launch counts in timings()

# tuning profile -> knobs; each one takes a different path through tyr_render
PROFILES = {
    "default": dict(),  # one iteration ahead of the counts, folded prologue, slot scan in the traversal launch, kernel-written snapshot
    "run_ahead0": dict(run_ahead=0),  # merged launches, the host waits for every iteration's counts
    "merge_trace0": dict(merge_trace=0),  # launch_iteration's loop: launch_kernels' order, a connect launch per iteration
    "fold_prologue0": dict(fold_prologue=0),  # run-ahead with every iteration opened by its own k_primary / hole-padding launches
    "scan_snapshot0": dict(scan_in_trace=0, kernel_snapshot=0),  # run-ahead with a k_scan_words launch and the counts copied behind shade
    "resolve_shadows0": dict(resolve_shadows=0),  # every shadow ray queued: the export after a render is the reference's queue
    "wide_blocks": dict(wide_block_min_items=0),  # every traversal launch as 768-thread blocks
}
# the profiles whose renders queue every shadow ray (the others answer some in place: TYR_TUNE_RESOLVE_SHADOWS)
SHADOW_EXACT = ("resolve_shadows0", "merge_trace0")
# the profiles whose loop is proved from the launch counts
COUNTED = ("default", "merge_trace0")

# frame / queue shapes: (W, H, N, rank, nranks)
SHAPES = {
    "fits": (24, 16, 512, 0, 1),  # N >= W * H: a whole sample per pixel in one top-up
    "tight": (32, 24, 320, 0, 1),  # N < W * H, and not a multiple of 64
    "odd": (37, 23, 500, 0, 1),
    "shard": (30, 24, 200, 1, 3),  # rank 1 of 3: every third row
}
SCENES = ("tyrant_default", "cornell_soup2k", "mesh32")


def dark_ground_scene():
    """test_gpu_parity.test_shadow_queue_after_a_render_that_ends_early's scene: a nearly black ground ends most paths by
    Russian roulette at once, so renders end before kMaxBounces iterations"""
    from oracle import pyorc
    from tyrant_amd import scenes

    sc0 = scenes.tyrant_default()
    sp = sc0.spheres.copy()
    sp["color"][4] = (0.06, 0.05, 0.04)
    sp["color"][0] = (0.1, 0.1, 0.1)
    sc = dataclasses.replace(sc0, spheres=sp)
    nodes, prims = pyorc.bvh_build(sc.triangles, scenes.triangle_bboxes(sc.triangles))
    return sc, nodes, prims


class Sides:
    """an oracle ctx and (with `hip`) a HIP ctx on the same scene; every operation goes to both and is followed by a comparison.
    `log` keeps, per operation, the oracle's counters before and after it and what it returned."""

    def __init__(self, orc, hip, scene, W, H, N, rank=0, nranks=1, profile="default", hip_flags=0):
        sc, nodes, prims = scene
        flags = (1 if sc.triangle_materials else 0) | (8 if sc.light_list else 0) | (16 if sc.triangle_colors else 0)
        self.sc, self.W, self.H, self.N, self.rank, self.nranks = sc, W, H, N, rank, nranks
        self.profile = profile
        self.o = orc.Oracle(W, H, N, rank=rank, nranks=nranks, flags=flags)
        self.o.load_scene(sc, nodes, prims)
        self.g = None
        if hip is not None:
            self.g = hip.Renderer(W, H, N, rank=rank, nranks=nranks, flags=flags | hip_flags | (FLAG_PROFILE if profile in COUNTED else 0))
            self.g.load_scene(sc, nodes, prims)
            self.g.set_tuning(**PROFILES[profile])
        self.donor = orc.Oracle(W, H, N, rank=rank, nranks=nranks, flags=flags)  # a second ctx whose survivors import_work_queue hands over
        self.donor.load_scene(sc, nodes, prims)
        self.donor.render(2, 2)
        self.moved = False
        self.sun_moved = False
        self.shadow_exact = True  # does the HIP ctx's shadow queue hold every shadow ray of the last iteration?
        self.own_scan = False  # are the survivors in the work queue placed by this ctx's own shade + slot scan (rank tables valid)?
        self.renders = []  # (spp, max_iterations, iterations, launch-count deltas) of the HIP ctx's renders
        self.log = []
        self.step = 0

    # ---- the operations ----
    def _do(self, name, fo, fg=None, returns=False):
        before = self.o.counters()
        ret = fo() if returns else (fo(), None)[1]
        if self.g is not None and fg is not None:
            rg = fg()
            assert not returns or rg == ret, f"{self.tag(name)}: returned {rg}, the oracle {ret}"
        self.log.append(dict(op=name, before=before, after=self.o.counters(), ret=ret))
        self.check(name)
        self.step += 1
        return ret

    def render(self, spp, max_iterations=UNBOUNDED):
        t0 = self.g.timings() if self.g is not None and self.profile in COUNTED else None

        def fg():
            it = self.g.render(spp, max_iterations)
            if t0 is not None:
                t1 = self.g.timings()
                self.renders.append((spp, max_iterations, it, {k: t1[k]["launches"] - t0[k]["launches"] for k in ("primary", "extend", "connect")}))
            return it

        if max_iterations:
            self.shadow_exact = self.profile in SHADOW_EXACT
        it = self._do(f"render({spp}, {'unbounded' if max_iterations == UNBOUNDED else max_iterations})", lambda: self.o.render(spp, 1 << 30 if max_iterations == UNBOUNDED else max_iterations), fg, returns=True)
        if it:
            self.own_scan = self.o.counters()["primary_ray_cnt"] > 0
        return it

    def launch(self):
        self.shadow_exact = True  # (launch_kernels queues every shadow ray)
        self._do("launch_kernels()", self.o.launch_kernels, self.g and self.g.launch_kernels)
        self.own_scan = True

    def staged(self):
        tag = self.tag("staged iteration")
        for st in ("begin", "primary", "extend", "shade", "connect", "end"):
            if st == "primary":
                survivors = self.o.counters()["primary_ray_cnt"]
            self.o.stage(st)
            if self.g is not None:
                self.g.stage(st)
            if st == "primary" and self.g is not None:
                ko, kg = self.o.counters(), self.g.counters()
                assert kg["device_error"] == 0, tag
                assert ko["n_live"] == kg["n_live"], (tag, "n_live after primary", ko["n_live"], kg["n_live"])
                n = ko["n_live"]
                assert_state_equal(self.o.ray_queue(0, n), self.g.ray_queue(0, n), tag + " after primary")
                if self.own_scan and survivors > 0:
                    assert self.g.queue_rank_check(0) == (n, 0), tag + ": rank tables -- survivors in front, fresh primary rays behind"
        self.log.append(dict(op="staged iteration", before=None, after=self.o.counters(), ret=None))
        self.own_scan, self.shadow_exact = True, True
        self.check("staged iteration")
        self.step += 1

    def set_budget(self, n):
        self._do(f"set_budget({n})", lambda: self.o.set_budget(n), lambda: self.g.set_budget(n))

    def reset_accum(self):
        self._do("reset_accum()", self.o.reset_accum, self.g and self.g.reset_accum)
        self.own_scan = False

    def set_camera(self):
        from tyrant_amd import scenes

        c = self.sc.camera
        self.moved = not self.moved
        cam = scenes.Camera(position=tuple(np.array(c.position) + np.array([3.0, 2.0, -1.0])), direction=c.direction, up=c.up, focalDistance=c.focalDistance, lensRadius=c.lensRadius) if self.moved else c
        self._do(f"set_camera({'moved' if self.moved else 'back'})", lambda: self.o.set_camera(cam), self.g and (lambda: self.g.set_camera(cam)))

    def set_sun(self):
        self.sun_moved = not self.sun_moved
        sun = (0.2, 0.25) if self.sun_moved else tuple(self.sc.sun_position)
        self._do(f"set_sun_position{sun}", lambda: self.o.set_sun_position(*sun), self.g and (lambda: self.g.set_sun_position(*sun)))

    def import_queue(self):
        n = self.donor.counters()["primary_ray_cnt"]
        rays = self.donor.ray_queue(0, n)
        self._do(f"import_work_queue({n} rays)", lambda: self.o.import_work_queue(rays, n), self.g and (lambda: self.g.import_work_queue(rays, n)))
        self.own_scan = False

    def query(self):
        """a batch of closest-hit and any-hit queries on the HIP ctx's scene (the oracle has none): they must leave the render state alone"""
        if self.g is None:
            self.log.append(dict(op="query", before=None, after=self.o.counters(), ret=None))
            return
        rng = np.random.default_rng(self.step)
        n = 777
        org = np.tile(np.float32(self.sc.camera.position), (n, 1)) + rng.normal(0, 1, (n, 3)).astype(np.float32)
        d = rng.normal(0, 1, (n, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        t, prim, geom, _ = self.g.query_closest(org, d, spheres=True)
        occ = self.g.query_any(org, d, spheres=True)
        assert bool(((prim >= 0) == occ).all()), self.tag("query: closest hit and any hit disagree on which rays hit")
        self.log.append(dict(op="query", before=None, after=self.o.counters(), ret=None))
        self.check("query batch")
        self.step += 1

    # ---- the comparison after every operation ----
    def tag(self, what):
        return f"[{self.profile}] step {self.step}: {what}"

    def check(self, what):
        if self.g is None:
            return
        tag = self.tag(what)
        ko, kg = self.o.counters(), self.g.counters()
        assert kg["device_error"] == 0, (tag, kg["device_error"])
        diff = {f: (ko[f], kg[f]) for f in FIELDS if ko[f] != kg[f]}
        assert not diff, f"{tag}: counters differ (oracle, HIP): {diff}"
        assert_accum_close(self.o.blit_buffer(), self.g.blit_buffer(), tag)
        n = ko["primary_ray_cnt"]
        assert_state_equal(self.o.ray_queue(0, n), self.g.ray_queue(0, n), tag + ": work queue")
        if self.shadow_exact:
            nh = ko["shadow_ray_cnt"]
            so, sg = self.o.shadow_queue(nh), self.g.shadow_queue(nh)
            for f in SHADOW_FIELDS:
                assert np.array_equal(bits(so[f]), bits(sg[f])), f"{tag}: shadow queue, {f}"
            assert np.array_equal(so["buffer_index"], sg["buffer_index"]), f"{tag}: shadow queue, buffer_index"

    def check_loop(self):
        """the launch counts show that the renders took the profile's loop (a sequence that silently takes the other path tests nothing)"""
        if self.g is None or self.profile not in COUNTED:
            return
        for spp, mx, it, d in self.renders:
            if self.profile == "merge_trace0":  # launch_kernels' order: primary, extend, shade, connect, iteration by iteration
                assert d["primary"] == d["extend"] == d["connect"] == it, (self.profile, spp, mx, it, d)
            else:  # merged: connect rides in the next traversal launch; at most one launch of its own for the render's last shadow rays
                assert d["connect"] <= 1 and d["extend"] >= it, (self.profile, spp, mx, it, d)
        if self.profile == "default" and any(spp > 0 and mx == UNBOUNDED and it >= 3 for spp, mx, it, _ in self.renders):
            # one iteration ahead with the prologue folded into the previous iteration's last kernel: fewer k_primary launches than iterations
            assert any(d["primary"] < it for _, _, it, d in self.renders), (self.profile, self.renders)


# ---- the named sequences ----
def _tight(orc, hip, profile):
    W, H, N, rank, nranks = SHAPES["tight"]
    return Sides(orc, hip, built_scene("cornell_soup2k"), W, H, N, rank, nranks, profile)


def seq_fresh_render0(s):
    """1. a fresh ctx: render(0), render(2), one staged iteration"""
    s.render(0), s.render(2), s.staged()


def seq_render0_after_finished(s):
    """2. render(0) on a ctx that holds no survivors and no budget (right after a finished render), then render(2), a staged iteration"""
    s.render(2), s.render(0), s.render(2), s.staged()


def seq_one_iteration_renders(s):
    """3. render(3, 1) again and again (each call re-arms the budget), then render(0, 1) until the survivors are gone, then render(0)"""
    for _ in range(5):
        s.render(3, 1)
    for _ in range(2 * MAX_BOUNCES):
        if s.o.counters()["primary_ray_cnt"] == 0:
            break
        s.render(0, 1)
    s.render(0)


def seq_cut_then_render(s):
    """4. render(2, 2), then render(2): survivors carried into a run-ahead render's iteration 0"""
    s.render(2, 2), s.render(2)


def seq_budget_launches(s):
    """5. set_budget(k) with k < N and k % 64 != 0, launch_kernels() three times, then render(1)"""
    s.set_budget(s.N - 120 if (s.N - 120) % 64 else s.N - 121)
    s.launch(), s.launch(), s.launch()
    s.render(1)


def seq_sun_with_survivors(s):
    """6. render(2, 2), set_sun_position (the accumulation reset with survivors held), render(1)"""
    s.render(2, 2), s.set_sun(), s.render(1)


def seq_camera_with_survivors(s):
    """7. render(2, 2), set_camera(moved), render(2)"""
    s.render(2, 2), s.set_camera(), s.render(2)


def seq_reset_with_survivors(s):
    """8. render(2, 2), reset_accum(), render(2)"""
    s.render(2, 2), s.reset_accum(), s.render(2)


def seq_render_zero_iterations(s):
    """9. render(1, 0) (sets the budget, runs nothing), launch_kernels(), render(1)"""
    s.render(1, 0), s.launch(), s.render(1)


def seq_import_drain(s):
    """10. import_work_queue, set_budget(0), render(0): only the imported rays drain (behind a render(1, 1): the first iteration of a
    fresh ctx resets the accumulation, and with it the survivors, as the camera counts as moved)"""
    s.render(1, 1), s.import_queue(), s.set_budget(0), s.render(0)


def seq_queries_between(s):
    """11. render(2, 2), a batch of ray queries, render(2)"""
    s.render(2, 2), s.query(), s.render(2)


def seq_early_ending(s):
    """12. on a scene whose renders end before kMaxBounces iterations: render(1) and render(0) alternating"""
    for _ in range(6):
        s.render(1), s.render(0)


NAMED = {
    "fresh_render0": (seq_fresh_render0, "tight"),
    "render0_after_finished": (seq_render0_after_finished, "tight"),
    "one_iteration_renders": (seq_one_iteration_renders, "tight"),
    "cut_then_render": (seq_cut_then_render, "tight"),
    "budget_launches": (seq_budget_launches, "tight"),
    "sun_with_survivors": (seq_sun_with_survivors, "tight"),
    "camera_with_survivors": (seq_camera_with_survivors, "tight"),
    "reset_with_survivors": (seq_reset_with_survivors, "tight"),
    "render_zero_iterations": (seq_render_zero_iterations, "tight"),
    "import_drain": (seq_import_drain, "tight"),
    "queries_between": (seq_queries_between, "tight"),
    "early_ending": (seq_early_ending, "dark16"),
}


def named_sides(orc, hip, name, profile):
    fn, where = NAMED[name]
    if where == "dark16":
        s = Sides(orc, hip, dark_ground_scene(), 16, 16, 256, profile=profile)
    else:
        s = _tight(orc, hip, profile)
    return fn, s


# ---- the random sequences ----
N_RANDOM = 12  # per profile: every scene with every shape


def random_ops(seed, N):
    """8 to 12 operations over the same alphabet as the named sequences"""
    rng = np.random.default_rng(seed)
    odd_budget = N - 37 if (N - 37) % 64 else N - 38
    ops = []
    for _ in range(int(rng.integers(8, 13))):
        k = rng.choice(["render"] * 5 + ["launch", "staged", "budget", "reset", "camera", "sun", "import", "query"])
        if k == "render":
            ops.append(("render", int(rng.integers(0, 4)), [0, 1, 2, 3, UNBOUNDED][int(rng.integers(0, 5))]))
        elif k == "budget":
            ops.append(("budget", [0, odd_budget, N + 37][int(rng.integers(0, 3))]))
        else:
            ops.append((str(k),))
    return ops


def run_random(s, ops):
    for op in ops:
        {"render": lambda: s.render(op[1], op[2]), "launch": s.launch, "staged": s.staged, "budget": lambda: s.set_budget(op[1]), "reset": s.reset_accum,
         "camera": s.set_camera, "sun": s.set_sun, "import": s.import_queue, "query": s.query}[op[0]]()


def random_case(orc, hip, profile, i):
    p = list(PROFILES).index(profile)
    scene = SCENES[i % len(SCENES)]  # (i in range(12): every pair of a scene and a shape)
    shape = list(SHAPES)[i % len(SHAPES)]
    W, H, N, rank, nranks = SHAPES[shape]
    seed = 7919 * (p + 1) + i
    return Sides(orc, hip, built_scene(scene), W, H, N, rank, nranks, profile), random_ops(seed, N), f"{scene} {shape} seed {seed}"


# ---- the tests ----
@pytest.fixture(scope="module")
def wall_time(request):
    t0 = time.perf_counter()
    yield
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    capman = request.config.pluginmanager.get_plugin("capturemanager")
    if tr is not None and capman is not None:
        with capman.global_and_fixture_disabled():
            tr.write_line(f"test_render_sequences: {time.perf_counter() - t0:.1f} s wall time")


@pytest.mark.gpu
@pytest.mark.parametrize("profile", list(PROFILES))
@pytest.mark.parametrize("name", list(NAMED))
def test_named_sequence(orc, hip, wall_time, name, profile):
    fn, s = named_sides(orc, hip, name, profile)
    fn(s)
    s.check_loop()


@pytest.mark.gpu
@pytest.mark.parametrize("profile", list(PROFILES))
@pytest.mark.parametrize("i", range(N_RANDOM))
def test_random_sequence(orc, hip, wall_time, profile, i):
    s, ops, what = random_case(orc, hip, profile, i)
    print(what, ops)
    run_random(s, ops)
    s.check_loop()


def test_named_sequences_reach_their_states(orc):
    """the named sequences on the oracle alone: each still reaches the state it is named for (a change to a scene generator or
    a shape must not quietly empty a sequence)"""

    def run(name):
        fn, s = named_sides(orc, None, name, "default")
        fn(s)
        return s, [e for e in s.log if e["op"].startswith("render")]

    # 2: render(0) meets a ctx with no survivors and no budget, and the render after it starts from there
    s, r = run("render0_after_finished")
    assert r[0]["ret"] > MAX_BOUNCES and r[1]["op"] == "render(0, unbounded)"
    assert r[1]["before"]["primary_ray_cnt"] == 0 and r[1]["before"]["budget_remaining"] == 0
    assert r[1]["ret"] == 1
    # 1: the fresh ctx's render(0) is one empty iteration
    s, r = run("fresh_render0")
    assert r[0]["before"]["primary_ray_cnt"] == 0 and r[0]["ret"] == 1 and r[0]["after"]["total_primary_rays"] == 0
    # 4, 6, 7, 8: the second render begins with survivors held
    for name in ("cut_then_render", "sun_with_survivors", "camera_with_survivors", "reset_with_survivors"):
        s, r = run(name)
        assert r[0]["ret"] == 2 and r[0]["after"]["primary_ray_cnt"] > 0 and r[0]["after"]["budget_remaining"] > 0, name
        assert s.log[1]["before"]["primary_ray_cnt"] > 0, name  # (the operation between the renders meets them too)
    # 3: one-iteration renders with survivors carried from call to call, then drained one iteration per call
    s, r = run("one_iteration_renders")
    assert all(e["ret"] == 1 for e in r[:-1]) and r[1]["before"]["primary_ray_cnt"] > 0
    assert any(e["op"] == "render(0, 1)" for e in r) and r[-1]["before"]["primary_ray_cnt"] == 0
    # 5: the budget is smaller than the queue and not a multiple of 64, and the launches spend it
    s, _ = run("budget_launches")
    k = s.log[0]["after"]["budget_remaining"]
    assert 0 < k < s.N and k % 64 != 0
    assert s.log[1]["after"]["budget_remaining"] == 0 and s.log[1]["after"]["total_primary_rays"] == k
    # 9: render(1, 0) sets the budget and runs nothing; launch_kernels() then spends it
    s, r = run("render_zero_iterations")
    assert r[0]["ret"] == 0 and r[0]["after"]["budget_remaining"] == s.W * s.H and r[0]["after"]["frame"] == r[0]["before"]["frame"]
    # 10: rays imported into a fresh ctx, drained without a top-up
    s, r = run("import_drain")
    n = s.log[1]["after"]["primary_ray_cnt"]
    assert n > 0 and n != s.log[0]["after"]["primary_ray_cnt"] and r[1]["before"]["primary_ray_cnt"] == n and r[1]["before"]["budget_remaining"] == 0
    assert r[1]["ret"] >= 2 and r[1]["after"]["total_primary_rays"] == r[1]["before"]["total_primary_rays"] and r[1]["after"]["n_survive"] > r[1]["before"]["n_survive"]
    # 11: survivors held across the queries
    s, r = run("queries_between")
    assert r[0]["after"]["primary_ray_cnt"] > 0
    # 12: renders that end before kMaxBounces iterations, at least one of them with shadow rays in its last iteration
    s, r = run("early_ending")
    ones = [e for e in r if e["op"] == "render(1, unbounded)"]
    assert sum(e["ret"] < MAX_BOUNCES + 1 for e in ones) >= 2
    assert any(e["ret"] < MAX_BOUNCES + 1 and e["after"]["shadow_ray_cnt"] > 0 for e in ones)
    # the random sequences: every scene and every shape, renders that carry survivors, and every operation
    seen = set()
    for profile in PROFILES:
        for i in range(N_RANDOM):
            s, ops, what = random_case(orc, None, profile, i)
            run_random(s, ops)
            seen.add(what.split()[0]), seen.add(what.split()[1])
            seen.update(op[0] for op in ops)
    assert seen >= set(SCENES) | set(SHAPES) | {"render", "launch", "staged", "budget", "reset", "camera", "sun", "import", "query"}, seen
