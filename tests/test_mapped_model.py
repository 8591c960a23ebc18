"""The oracle-only model of mapped mode (tests/mapped_model.py) pinned on the CPU: these tests are the guard that the model,
not the GPU, is the specification the sequence tests (test_call_sequences.py) hold the HIP ctx to."""
import numpy as np
import pytest

import adaptive_ref as ar
from conftest import bits, built_scene
from mapped_model import MappedOracle, maps
from test_render_sequences import FIELDS


def flags_of(sc):
    return (1 if sc.triangle_materials else 0) | (8 if sc.light_list else 0) | (16 if sc.triangle_colors else 0)


def oracle(orc, name, W, H, N, rank=0, nranks=1):
    sc, nodes, prims = built_scene(name)
    o = orc.Oracle(W, H, N, rank=rank, nranks=nranks, flags=flags_of(sc))
    o.load_scene(sc, nodes, prims)
    return o


def model(orc, name, W, H, N, rank=0, nranks=1):
    return MappedOracle(oracle(orc, name, W, H, N, rank, nranks), built_scene(name)[0].camera, rank, nranks)


def assert_same_state(a, b, what):
    """two oracle-side ctxs: FIELDS, the accumulation buffer, both ray queues (all N slots) and the shadow queue, bit for bit"""
    ka, kb = a.counters(), b.counters()
    diff = {f: (ka[f], kb[f]) for f in FIELDS if ka[f] != kb[f]}
    assert not diff, (what, diff)
    assert a.blit_buffer().tobytes() == b.blit_buffer().tobytes(), what + ": accumulation"
    for which in (0, 1):
        assert a.ray_queue(which).tobytes() == b.ray_queue(which).tobytes(), f"{what}: ray queue {which}"
    n = ka["shadow_ray_cnt"]
    assert a.shadow_queue(n).tobytes() == b.shadow_queue(n).tobytes(), what + ": shadow queue"


# (scene, W, H, N, rank, nranks, k): glass_dof48 has a lens; N < W * H with N % 64 != 0; a shard
UNIFORM = [("cornell36", 40, 24, 700, 0, 1, 2), ("glass_dof48", 48, 27, 700, 0, 1, 3), ("tyrant_default", 24, 16, 512, 0, 1, 2), ("tyrant_default", 30, 24, 200, 1, 3, 2)]


@pytest.mark.parametrize("name,W,H,N,rank,nranks,k", UNIFORM)
def test_uniform_map_on_a_fresh_ctx_is_render(orc, name, W, H, N, rank, nranks, k):
    """start_position == 0: render_adaptive(full(k)) IS render(k) -- the iteration count, and after the render all of FIELDS,
    the accumulation buffer and the queues bit for bit; the same holds iteration by iteration through launch_kernels"""
    m, o = model(orc, name, W, H, N, rank, nranks), oracle(orc, name, W, H, N, rank, nranks)
    assert m.counters()["start_position"] == 0
    full = np.full((H, W), k, np.int32)
    it = m.render_adaptive(full)
    assert it == o.render(k) and it > 1
    assert m.counters()["total_primary_rays"] == k * W * (H // nranks)
    assert_same_state(m, o, f"{name} uniform {k}")
    # ... and step by step, from the state the renders left (start_position back at 0: whole samples were spent)
    assert m.counters()["start_position"] == 0
    assert m.set_sample_map(full) == k * W * (H // nranks)
    o.set_budget(k * W * (H // nranks))
    for i in range(it):
        m.launch_kernels(), o.launch_kernels()
        assert_same_state(m, o, f"{name} uniform {k}, iteration {i}")
    assert m.counters()["budget_remaining"] == 0 and m.counters()["primary_ray_cnt"] == 0


def test_uniform_map_off_the_first_pixel_is_not_render(orc):
    """start_position != 0: tyr_render goes on from its cursor, mapped mode starts at ticket 0 = pixel 0 -- the header's
    "a uniform map with start_position == 0" is a real condition, and the model has it"""
    name, W, H, N = "cornell36", 40, 24, 700
    m, o = model(orc, name, W, H, N), oracle(orc, name, W, H, N)
    for x in (m, o):
        x.set_budget(333)
        x.launch_kernels()
    assert_same_state(m, o, "a budget of 333")
    assert m.counters()["start_position"] == 333
    surv = m.counters()["primary_ray_cnt"]
    assert 0 < surv < N
    m.set_sample_map(np.full((H, W), 1, np.int32)), m.stage("begin"), m.stage("primary")
    o.set_budget(W * H), o.stage("begin"), o.stage("primary")
    km, ko = m.counters(), o.counters()
    assert km["n_live"] == ko["n_live"] == N
    assert km["start_position"] == ko["start_position"] == (333 + N - surv) % (W * H)  # (it advances by the rays made all the same)
    qm, qo = m.ray_queue(0, N), o.ray_queue(0, N)
    assert qm[:surv].tobytes() == qo[:surv].tobytes()
    assert qm["index"][surv] == 0 and qo["index"][surv] == 333


@pytest.mark.parametrize("rank,nranks", [(0, 1), (1, 3)])
def test_a_random_map_adds_its_counts_to_the_ctxs_rows(orc, rank, nranks):
    """run to completion: exactly c[p] more in the count channel of the ctx's rows, nothing anywhere else (the oracle's blit
    buffer is full-frame on a shard too)"""
    name, W, H, N = "cornell36", 30, 24, 200
    rng = np.random.default_rng(21 + rank)
    m = model(orc, name, W, H, N, rank, nranks)
    m.render(1)
    before = m.blit_buffer()
    c = maps(H, W, rng)["random"]
    k0 = m.counters()
    it = m.render_adaptive(c)
    k1 = m.counters()
    own = np.zeros((H, W), bool)
    own[rank::nranks] = True
    T = int(c[own].sum())
    assert it > 2 and k1["budget_remaining"] == 0 and k1["primary_ray_cnt"] == 0
    assert k1["total_primary_rays"] - k0["total_primary_rays"] == T
    assert k1["start_position"] == (k0["start_position"] + T) % (W * (H // nranks))
    added = (m.blit_buffer() - before)[:, 3].reshape(H, W)
    assert np.array_equal(added[own], c[own].astype(np.float32))
    assert not np.any(added[~own]) and not np.any((m.blit_buffer() - before)[~own.reshape(-1)])


def test_entered_with_survivors_held(orc):
    """after render(2, 2): the survivors keep their slots 0 .. surv - 1, the first new ray behind them is ticket 0 at launch
    index 0, and the budget is the map's"""
    name, W, H, N = "cornell36", 32, 24, 320
    rng = np.random.default_rng(5)
    m = model(orc, name, W, H, N)
    assert m.render(2, 2) == 2
    k = m.counters()
    surv = k["primary_ray_cnt"]
    assert 0 < surv < N and k["budget_remaining"] > 0
    held = m.ray_queue(0, surv)
    c = maps(H, W, rng)["random"]
    c[0, :3] = 0  # (ticket 0 is not pixel 0)
    T = m.set_sample_map(c)
    assert m.counters()["budget_remaining"] == T == int(c.sum()) and m.counters()["primary_ray_cnt"] == surv
    m.stage("begin")
    frame = m.counters()["frame"]
    m.stage("primary")
    k = m.counters()
    assert k["n_live"] == N and k["budget_remaining"] == T - (N - surv)
    q = m.ray_queue(0, N)
    assert q[:surv].tobytes() == held.tobytes()
    L = ar.ticket_list(c.reshape(-1))
    assert L[0] == 3 and np.array_equal(q["index"][surv:], L[: N - surv])
    origin, direction, index = ar.camera_rays(orc.lib(), built_scene(name)[0].camera, W, H, L[:1], [0], frame)
    assert np.array_equal(bits(q["origin"][surv]), bits(origin[0])) and np.array_equal(bits(q["direction"][surv]), bits(direction[0]))
    assert np.all(q["bounces"][surv:] == 0) and np.all(q["direct"][surv:] == 1) and np.all(q["lastSpecular"][surv:] == 1) and np.all(q["geometry_type"][surv:] == 1)
    for st in ("extend", "shade", "connect", "end"):
        m.stage(st)
    # the next launch goes on in the list where this one stopped
    s2 = m.counters()["primary_ray_cnt"]
    m.stage("begin"), m.stage("primary")
    assert np.array_equal(m.ray_queue(0, N)["index"][s2:], L[N - surv: N - surv + N - s2])


def test_an_empty_map_and_one_pixel_at_65535(orc):
    name, W, H, N = "cornell36", 24, 16, 512
    m, o = model(orc, name, W, H, N), oracle(orc, name, W, H, N)
    zero = np.zeros((H, W), np.int32)
    # T == 0 behaves like render(0): on a fresh ctx, after a finished render, and with survivors held
    for prepare in (lambda x: None, lambda x: x.render(1), lambda x: x.render(2, 2)):
        prepare(m), prepare(o)
        assert m.render_adaptive(zero) == o.render(0)
        assert m.counters()["budget_remaining"] == 0 and m.mapped
        assert_same_state(m, o, "an all-zero map")
    one = zero.copy()
    one[5, 7] = 65535
    m.reset_accum()
    it = m.render_adaptive(one)
    assert it >= 65535 // N + 1
    count = m.blit_buffer()[:, 3]
    assert count[5 * W + 7] == 65535 and np.count_nonzero(count) == 1
    assert m.counters()["budget_remaining"] == 0
