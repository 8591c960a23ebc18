"""Refit of the uploaded scene for moving geometry (tyr_scene_refit, hip/refit.hip; Renderer.refit).

The tree keeps its shape; the boxes follow the reference's rule -- a leaf's box is Union folded from BBox{} ({1e10, -1e10},
Bbox.h:5) over its primitives' boxes in array order (bvh.cpp:71-73), an interior node's Union(left, right) (bvh.cpp:222), with
glibc's fmin / fmax (the first argument wins ties).  refit_nodes() below restates that rule in numpy; the CPU tests pin it to the
oracle's builder.  On the GPU the refitted scene must be byte for byte what tyr_scene_upload(refit_nodes(...), moved) makes
(tyr_layout_probe's hashes), and queries and renders on it must match the oracle given the same arrays."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits, built_scene

CSRC = os.path.join(ROOT, "tyrant_amd", "csrc")
TYR_FLAG_COUNT_VISITS, TYR_FLAG_REFIT = 4, 64


# ---- the reference's rule in numpy ------------------------------------------------------------------------------------
def _fmin(a, b):
    return np.where(b < a, b, a)


def _fmax(a, b):
    return np.where(b > a, b, a)


def refit_nodes(nodes: np.ndarray, bboxes: np.ndarray) -> np.ndarray:
    """nodes with every box recomputed from the primitive boxes `bboxes` (build order), level by level"""
    out = nodes.copy()
    n = nodes.shape[0]
    if n == 0:
        return out
    cnt = nodes["primitiveCount"].astype(np.int64)
    off = nodes["offset"].astype(np.int64)
    leaf = cnt > 0
    blo, bhi = bboxes["bounds"][:, 0, :], bboxes["bounds"][:, 1, :]
    lo = np.full((n, 3), 1e10, dtype=np.float32)
    hi = np.full((n, 3), -1e10, dtype=np.float32)
    li = np.nonzero(leaf)[0]
    for j in range(int(cnt.max()) if li.size else 0):
        m = li[cnt[li] > j]
        p = off[m] + j
        lo[m] = _fmin(lo[m], blo[p])
        hi[m] = _fmax(hi[m], bhi[p])
    # the interior nodes level by level (breadth-first), then united deepest level first
    levels = []
    front = np.array([0], dtype=np.int64)
    while front.size:
        inner = front[~leaf[front]]
        levels.append(inner)
        front = np.concatenate([inner + 1, off[inner]])
    for inner in reversed(levels):
        l, r = inner + 1, off[inner]
        lo[inner] = _fmin(lo[l], lo[r])
        hi[inner] = _fmax(hi[l], hi[r])
    out["bounds"][:, 0, :] = lo
    out["bounds"][:, 1, :] = hi
    return out


def tri_bboxes(prims):
    """tyr_triangle_bboxes (what tyr_scene_refit uses when no boxes are given)"""
    from tyrant_amd import binding

    return binding.triangle_bboxes(prims)


def stacked_scene():
    """the Cornell box plus two stacks of identical-centroid triangles: leaves of 40 and 70 primitives"""
    from tyrant_amd import scenes

    def stack(x0, n):
        return scenes.make_triangles(np.tile([x0 - 30, 0, 10], (n, 1)), np.tile([x0 + 30, 0, 10], (n, 1)), np.tile([x0, 0, 70], (n, 1)))

    return np.concatenate([scenes.cornell_box().triangles, stack(-10.0, 40), stack(15.0, 70)])


def signed_zero_scene():
    """triangles whose coordinates include +0.0 and -0.0 on every axis (the tie rule decides which one a box keeps)"""
    from tyrant_amd import scenes

    rng = np.random.default_rng(11)
    n = 64
    v0 = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    v1 = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    v2 = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    z = rng.random((n, 3)) < 0.4
    v0[z] = np.where(rng.random(z.sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
    z = rng.random((n, 3)) < 0.4
    v1[z] = np.where(rng.random(z.sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
    t = scenes.make_triangles(v0, v1, v2)
    t["e1"][rng.random((n, 3)) < 0.3] = np.float32(-0.0)  # vert + (-0) = vert, but vert(-0) + (-0) = -0
    return t


def scene_arrays(name):
    """(nodes, prims, bboxes) built by the oracle's builder"""
    from oracle import pyorc
    from tyrant_amd import scenes

    if name in ("stacked", "one_triangle", "signed_zero"):
        tris = {"stacked": stacked_scene, "signed_zero": signed_zero_scene,
                "one_triangle": lambda: scenes.make_triangles([(0, 0, 0)], [(1, 0, 0)], [(0, 1, 0)])}[name]()
        bb = scenes.triangle_bboxes(tris)
        nodes, prims = pyorc.bvh_build(tris, bb)
        return nodes, prims, bb
    sc, nodes, prims = built_scene(name)
    return nodes, prims, scenes.triangle_bboxes(prims)


# ---- CPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell36", "mesh128", "cornell_soup2k", "stacked", "one_triangle", "signed_zero"])
def test_refit_rule_reproduces_the_builders_boxes(name):
    """refitting unchanged triangles gives the builder's node array bit for bit: the helper is bvh.cpp's rule"""
    nodes, prims, bb = scene_arrays(name)
    if name == "stacked":
        assert nodes["primitiveCount"].max() > 31
    if name == "signed_zero":
        b = bits(nodes["bounds"])
        assert np.any(b == 0x80000000) and np.any(b == 0)
    # the builder reorders the primitives: their boxes in build order
    from tyrant_amd import scenes

    bb_built = scenes.triangle_bboxes(prims)
    r = refit_nodes(nodes, bb_built)
    assert r.tobytes() == nodes.tobytes()


def _refit_resources():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "build", "refit.resources.txt")):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name:"):
            cur = out.setdefault(text.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in text:
            k, v = text.rsplit(":", 1)
            cur[k.strip()] = int(v) if v.strip().lstrip("-").isdigit() else v.strip()
    return out


def test_refit_kernels_do_not_spill():
    """every refit kernel compiles without VGPR spills and without scratch"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("no hipcc: the kernels cannot be built")
    subprocess.run(["make", "-s", "-C", CSRC, "build/refit.s"], check=True, capture_output=True, timeout=900)
    res = _refit_resources()
    names = [n for n in res if "k_refit_" in n]
    assert len(names) == 5, list(res)
    for n in names:
        assert res[n]["VGPRs Spill"] == 0 and res[n]["SGPRs Spill"] == 0, (n, res[n])
        assert res[n]["ScratchSize [bytes/lane]"] == 0, (n, res[n])


# ---- GPU --------------------------------------------------------------------------------------------------------------
def deform(prims, amp=1.5, seed=0):
    """a deterministic wave through the vertices (and a stretch of the edges): same materials, same order"""
    m = prims.copy()
    v = m["vert"].astype(np.float64)
    m["vert"][:, 2] = (v[:, 2] + amp * np.sin(0.21 * v[:, 0] + seed) * np.cos(0.17 * v[:, 1])).astype(np.float32)
    m["vert"][:, 0] = (v[:, 0] + 0.25 * amp * np.cos(0.13 * v[:, 2] + seed)).astype(np.float32)
    m["e1"] = (m["e1"] * np.float32(1.0 + 0.05 * amp)).astype(np.float32)
    return m


PATHS = ("host", "host_pairs", "device", "build_upload")


def upload(hip, path, nodes, prims, flags=TYR_FLAG_REFIT, W=64, H=64, N=4096):
    """a ctx holding (nodes, prims) through one upload path; returns (ctx, nodes, prims) -- build_upload builds its own tree"""
    g = hip.Renderer(W, H, N, flags=flags | (TYR_FLAG_COUNT_VISITS if path == "host_pairs" else 0))
    g.set_tuning(layout_on_device=0 if path in ("host", "host_pairs") else 1)
    if path == "build_upload":
        nodes, prims, _ = g.build_upload(prims)
        if prims.shape[0] == 0:
            nodes = np.zeros(0, dtype=nodes.dtype)
    else:
        g.upload(nodes, prims)
    return g, nodes, prims


def expected_hash(hip, nodes, prims, pairs):
    p = hip.layout_probe(nodes, prims, want_pairs=pairs)
    return p["hash_quads"], p["hash_pairs"], p["hash_tris"]


def held_hash(g):
    h = g.scene_hash()
    return h["hash_quads"], h["hash_pairs"], h["hash_tris"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["mesh128", "stacked", "one_triangle", "empty"])
def test_identity_refit_keeps_the_scene(hip, path, name):
    """refitting the uploaded records changes no byte of the scene, on every upload path"""
    from tyrant_amd import scenes

    if name == "empty":
        nodes, prims = np.zeros(0, dtype=scenes.NODE_DTYPE), np.zeros(0, dtype=scenes.TRIANGLE_DTYPE)
    else:
        nodes, prims, _ = scene_arrays(name)
    g, nodes, prims = upload(hip, path, nodes, prims)
    before = held_hash(g)
    out = g.refit(prims, want_nodes=True)
    assert held_hash(g) == before
    assert out.tobytes() == nodes.tobytes()
    if name != "empty":
        assert held_hash(g) == expected_hash(hip, nodes, prims, path == "host_pairs")
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["mesh706", "stacked", "one_triangle"])
def test_moved_scene_is_the_upload_of_the_refitted_tree(hip, path, name):
    """after a deformation: nodes_out = refit_nodes(...) bit for bit, and the held scene = tyr_layout_probe(nodes', moved)"""
    nodes, prims, _ = scene_arrays(name)
    g, nodes, prims = upload(hip, path, nodes, prims)
    moved = deform(prims, seed=1)
    want = refit_nodes(nodes, tri_bboxes(moved))
    got = g.refit(moved, want_nodes=True)
    assert got.tobytes() == want.tobytes()
    assert held_hash(g) == expected_hash(hip, want, moved, path == "host_pairs")
    # and again from there: a second refit starts from the refitted plan
    moved2 = deform(prims, amp=3.0, seed=2)
    bb2 = tri_bboxes(moved2)
    got2 = g.refit(moved2, bboxes=bb2, want_nodes=True)
    want2 = refit_nodes(nodes, bb2)
    assert got2.tobytes() == want2.tobytes()
    assert held_hash(g) == expected_hash(hip, want2, moved2, path == "host_pairs")
    g.close()


@pytest.mark.gpu
def test_queries_on_the_refitted_scene(orc, hip):
    """closest and any hit after a refit match the reference on (nodes', moved) bit for bit, barycentrics included"""
    from test_ray_query import glm_uv, np_results, oracle_any, oracle_closest, random_dirs

    nodes, prims, _ = scene_arrays("mesh128")
    g, nodes, prims = upload(hip, "device", nodes, prims)
    moved = deform(prims, amp=4.0, seed=3)
    want = g.refit(moved, want_nodes=True)
    rng = np.random.default_rng(7)
    n = 32768
    o = np.stack([rng.uniform(-45, 45, n), rng.uniform(-45, 45, n), rng.uniform(30, 60, n)], axis=1).astype(np.float32)
    d = random_dirs(rng, n)
    d[: n // 2, 2] = -np.abs(d[: n // 2, 2])
    tmax = np.full(n, 1e20, dtype=np.float32)
    t, prim, geom, uv = np_results(g.query_closest(o, d, tmax))
    wt, wp = oracle_closest(orc, want, moved, o, d, tmax)
    assert np.array_equal(bits(t), bits(wt)) and np.array_equal(prim, wp)
    hit = prim >= 0
    assert hit.sum() > n // 4
    u, v = glm_uv(orc, moved, prim[hit], o[hit], d[hit])
    assert np.array_equal(bits(uv[hit, 0]), bits(u)) and np.array_equal(bits(uv[hit, 1]), bits(v))
    tm = np.where(hit, t * np.float32(0.999), np.float32(80.0)).astype(np.float32)
    occ = g.query_any(o, d, tm).cpu().numpy()
    assert np.array_equal(occ, oracle_any(orc, want, moved, o, d, tm))
    g.close()


def _move_lights(prims):
    m = prims.copy()
    light = m["materialType"] == 4
    assert light.any()
    m["vert"][light, 2] -= np.float32(6.0)
    m["vert"][light, 0] += np.float32(3.0)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,N,spp", [("mesh128", 96, 96, 8192, 2), ("cornell_area_light", 128, 96, 8192, 3)])
def test_render_after_refit_matches_the_oracle(orc, hip, name, W, H, N, spp):
    """render(spp) after a refit = the oracle uploaded with (nodes', moved): iterations, counters, accumulation"""
    from test_gpu_parity import assert_accum_close, pair

    sc, nodes, prims = built_scene(name)
    o, g = pair(orc, hip, name, W, H, N, flags=TYR_FLAG_REFIT)
    moved = _move_lights(prims) if name == "cornell_area_light" else deform(prims, amp=2.0, seed=4)
    want = g.refit(moved, want_nodes=True)
    assert want.tobytes() == refit_nodes(nodes, tri_bboxes(moved)).tobytes()
    o.upload(want, moved)
    assert o.render(spp) == g.render(spp)
    ko, kg = o.counters(), g.counters()
    assert kg["device_error"] == 0
    for f in ("total_primary_rays", "total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible", "start_position", "frame"):
        assert ko[f] == kg[f], f
    assert_accum_close(o.blit_buffer(), g.blit_buffer(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"merge_trace": 0}])
def test_refit_between_renders_with_survivors_held(orc, hip, knobs):
    """render with survivors held, refit, render on: the oracle does the same with upload(nodes', moved) in between.  After
    every step: counters, accumulation and work queue as tests/test_render_sequences.py compares them"""
    from test_gpu_parity import assert_accum_close, assert_state_equal, pair
    from test_render_sequences import FIELDS

    name = "mesh128"
    sc, nodes, prims = built_scene(name)
    o, g = pair(orc, hip, name, 64, 64, 4096, flags=TYR_FLAG_REFIT)
    g.set_tuning(**knobs)

    def check(what):
        ko, kg = o.counters(), g.counters()
        assert kg["device_error"] == 0, what
        diff = {f: (ko[f], kg[f]) for f in FIELDS if ko[f] != kg[f]}
        assert not diff, f"{what}: counters differ (oracle, HIP): {diff}"
        assert_accum_close(o.blit_buffer(), g.blit_buffer(), what)
        n = ko["primary_ray_cnt"]
        assert_state_equal(o.ray_queue(0, n), g.ray_queue(0, n), what + ": work queue")
        return ko

    assert o.render(1, 2) == g.render(1, 2)
    assert check("first render")["n_survive"] > 0
    for step, moved in enumerate([deform(prims, amp=2.0, seed=5), deform(prims, amp=1.0, seed=6)]):
        want = g.refit(moved, want_nodes=True)
        o.upload(want, moved)
        check(f"step {step}: after the refit")
        assert o.render(1, 2) == g.render(1, 2)
        check(f"step {step}: after the render")
    assert o.render(1) == g.render(1)
    check("last render")


@pytest.mark.gpu
def test_device_input_from_a_side_stream(hip):
    """torch tensors written on a side stream: the refit waits for that stream and gives the host path's bytes"""
    import torch

    nodes, prims, _ = scene_arrays("mesh128")
    moved = deform(prims, amp=2.5, seed=8)
    g_host, _, _ = upload(hip, "device", nodes, prims)
    g_host.refit(moved)
    want = held_hash(g_host)
    g_host.close()
    for with_boxes in (False, True):
        g, _, _ = upload(hip, "device", nodes, prims)
        side = torch.cuda.Stream()
        raw = torch.from_numpy(moved.view(np.float32).reshape(-1, 10).copy())
        boxes = torch.from_numpy(tri_bboxes(moved).view(np.float32).reshape(-1, 6).copy())
        with torch.cuda.stream(side):
            dev = torch.zeros_like(raw, device="cuda")
            torch.cuda._sleep(2_000_000)  # the copy lands well after the call was made
            dev.copy_(raw.cuda(non_blocking=False))
            bdev = boxes.cuda() if with_boxes else None
        nodes_out = g.refit(dev, bboxes=bdev, stream=side, want_nodes=True)
        assert held_hash(g) == want
        assert nodes_out.tobytes() == refit_nodes(nodes, tri_bboxes(moved)).tobytes()
        g.close()


def _render_state(g):
    g.render(1, 2)
    k = g.counters()
    return held_hash(g), {f: k[f] for f in ("n_live", "total_extend_rays", "total_shadow_rays", "frame")}, g.blit_buffer()


@pytest.mark.gpu
def test_rejected_refits_change_nothing(hip):
    """NaN, a wrong count, a changed materialType or palette byte, no TYR_FLAG_REFIT, no scene: an error, and the scene,
    counters and a following render are those of a ctx that never saw the call"""
    from tyrant_amd import binding, scenes

    sc, nodes, prims = built_scene("mesh128")

    def fresh(flags=TYR_FLAG_REFIT):
        g = hip.Renderer(64, 64, 4096, flags=flags | 1)
        g.load_scene(sc, nodes, prims)
        return g

    ref = fresh()
    want = _render_state(ref)
    ref.close()
    nan = deform(prims)
    nan["vert"][17, 1] = np.nan
    inf_box = tri_bboxes(deform(prims))
    inf_box["bounds"][3, 1, 2] = np.inf
    mat = deform(prims)
    mat["materialType"][5] ^= 1
    pal = deform(prims)
    pal["pad_"][9, 0] = 7
    cases = [(nan, None, binding.TYR_ERR_INVALID), (deform(prims)[:-1], None, binding.TYR_ERR_INVALID), (mat, None, binding.TYR_ERR_INVALID),
             (pal, None, binding.TYR_ERR_INVALID), (deform(prims), inf_box, binding.TYR_ERR_INVALID)]
    for moved, bb, code in cases:
        g = fresh()
        with pytest.raises(binding.TyrError) as e:
            g.refit(moved, bboxes=bb)
        assert e.value.status == code
        got = _render_state(g)
        assert got[0] == want[0] and got[1] == want[1] and np.array_equal(bits(got[2]), bits(want[2]))
        g.close()
    g = fresh(flags=0)
    with pytest.raises(binding.TyrError) as e:
        g.refit(deform(prims))
    assert e.value.status == binding.TYR_ERR_UNSUPPORTED
    got = _render_state(g)
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(bits(got[2]), bits(want[2]))
    g.close()
    g = hip.Renderer(64, 64, 4096, flags=TYR_FLAG_REFIT)
    with pytest.raises(binding.TyrError) as e:
        g.refit(prims)
    assert e.value.status == binding.TYR_ERR_NO_SCENE
    g.upload(np.zeros(0, dtype=scenes.NODE_DTYPE), np.zeros(0, dtype=scenes.TRIANGLE_DTYPE))
    g.refit(np.zeros(0, dtype=scenes.TRIANGLE_DTYPE))  # an empty scene: a no-op
    with pytest.raises(binding.TyrError) as e:
        g.refit(prims[:3])
    assert e.value.status == binding.TYR_ERR_INVALID
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_device_bytes_count_the_plan_only_with_the_flag(hip, path):
    """without TYR_FLAG_REFIT device_bytes is what the upload always reported; with it, the plan is added"""
    nodes, prims, _ = scene_arrays("mesh128")
    g0, _, _ = upload(hip, path, nodes, prims, flags=0)
    g1, _, _ = upload(hip, path, nodes, prims)
    i0, i1 = g0.scene_info(), g1.scene_info()
    pairs = i0["n_pair_nodes"] if path == "host_pairs" else 0
    assert i0["device_bytes"] == i0["n_quad_nodes"] * 128 + pairs * 64 + i0["n_prims"] * 48
    assert i1["device_bytes"] > i0["device_bytes"] + nodes.nbytes
    assert held_hash(g0) == held_hash(g1)
    assert {k: v for k, v in i0.items() if not k.endswith("_s") and k != "device_bytes"} == {k: v for k, v in i1.items() if not k.endswith("_s") and k != "device_bytes"}
    g0.close(), g1.close()
