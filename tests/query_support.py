"""What the test modules of the scene queries share (test_ray_query, test_hit_query, test_point_query, test_point_query_k,
test_occlusion_query, test_winding_query, test_sweep_query, test_box_query, test_query_streams, test_query_shapes): the scenes and inputs more than
one of them is run on, the renderer they ask, the comparison of an answer with its restatement, and the checks every query kind
repeats -- what the compiler made of its kernels, its part of the ABI, that it leaves a render alone.

Every seed, count and constant is an argument of the call site: a fixture here is the same arrays whichever module asks."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import nearest_ref
from conftest import ROOT, bits
from kernel_resources import kernel_resources

F = np.float32
LDS_PER_CU, LDS_GRANULE = 163840, 1280
OFFSET = np.array([4096.0, -4096.0, 8192.0], F)


# ---- scenes and inputs (numpy only) -----------------------------------------------------------------------------------
def build(tris):
    from tyrant_amd import binding

    return binding.bvh_build(tris)


def no_triangles():
    """(nodes, prims) of a scene without triangles"""
    from tyrant_amd import scenes

    return np.zeros(0, dtype=scenes.NODE_DTYPE), np.zeros(0, dtype=scenes.TRIANGLE_DTYPE)


def unit(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F)


def tri(vert, e1, e2):
    """one triangle record from vert, e1, e2 as given"""
    from tyrant_amd import scenes

    t = np.zeros(1, dtype=scenes.TRIANGLE_DTYPE)
    t["vert"], t["e1"], t["e2"] = np.array(vert, F), np.array(e1, F), np.array(e2, F)
    return t


def box(lo=(-10.0, -10.0, 5.0), hi=(10.0, 10.0, 25.0)):
    """the 12 outward-facing triangles of an axis-aligned box: a closed mesh"""
    from tyrant_amd import scenes

    c = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)], F)
    v0, v1, v2 = [], [], []
    for a, b, cc, d in ((0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)):  # outward
        v0 += [c[a], c[a]]
        v1 += [c[b], c[cc]]
        v2 += [c[cc], c[d]]
    return scenes.make_triangles(np.array(v0), np.array(v1), np.array(v2))


def stack40():
    """40 identical triangles in the plane y = 0, facing -y: one over-long leaf behind synthetic records"""
    from tyrant_amd import scenes

    return scenes.make_triangles(np.tile([-30, 0, 10], (40, 1)), np.tile([30, 0, 10], (40, 1)), np.tile([0, 0, 70], (40, 1)))


def root_box(prims, inflate=0.1):
    vert, e1, e2 = nearest_ref.records(prims)
    allv = np.concatenate([vert, vert + e1, vert + e2])
    lo, hi = allv.min(axis=0), allv.max(axis=0)
    pad = (hi - lo) * F(inflate)
    return (lo - pad).astype(F), (hi + pad).astype(F)


def box_points(rng, prims, n):
    lo, hi = root_box(prims)
    return (lo + (hi - lo) * rng.random((n, 3))).astype(F)


def surface_points(rng, prims, n, noise):
    """a point of a seeded triangle plus noise"""
    vert, e1, e2 = nearest_ref.records(prims)
    i = rng.integers(0, len(prims), n)
    u = rng.random(n)
    v = rng.random(n) * (1 - u)
    p = vert[i].astype(np.float64) + u[:, None] * e1[i] + v[:, None] * e2[i]
    return (p + rng.normal(size=(n, 3)) * noise).astype(F)


def grid_points(cells):
    """the points at z = 40 above every vertex of heightfield(cells)"""
    xs = np.linspace(-50.0, 50.0, cells + 1)
    X, Y = np.meshgrid(xs, xs, indexing="xy")
    return np.stack([X.reshape(-1), Y.reshape(-1), np.full(X.size, 40.0)], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def lattice(cells, seed):
    """heightfield(cells): (nodes, prims, grid points above every vertex at z = 40, 4096 seeded points in the inflated root box)"""
    from tyrant_amd import scenes

    nodes, prims = build(scenes.heightfield(cells))
    return nodes, prims, grid_points(cells), box_points(np.random.default_rng(seed), prims, 4096)


@functools.lru_cache(maxsize=None)
def duplicated(seed, n):
    """heightfield(16) concatenated with itself: (nodes, prims, points, twin) -- the grid points and n seeded ones; twin[i] is the
    index of i's equal record"""
    from tyrant_amd import scenes

    h = scenes.heightfield(16)
    nodes, prims = build(np.concatenate([h, h]))
    pts = np.concatenate([grid_points(16), box_points(np.random.default_rng(seed), prims, n)])
    raw = np.ascontiguousarray(prims).view(np.uint8).reshape(len(prims), -1)
    twins = np.lexsort(raw.T[::-1]).reshape(-1, 2)  # equal records are neighbours in the sorted order: pairs
    assert np.array_equal(raw[twins[:, 0]], raw[twins[:, 1]])
    twin = np.empty(len(prims), np.int64)
    twin[twins[:, 0]], twin[twins[:, 1]] = twins[:, 1], twins[:, 0]
    return nodes, prims, pts, twin


def offset_soup(slivers):
    """random_soup(2000) moved by OFFSET; slivers: every tenth triangle's e2 = 0.75 e1 + a perpendicular of 1e-5 |e1|"""
    from tyrant_amd import scenes

    t = scenes.random_soup(2000)
    if slivers:
        e1 = t["e1"][::10].astype(np.float64)
        perp = np.cross(e1, [0.3, -0.5, 0.8])
        perp *= 1e-5 * np.linalg.norm(e1, axis=1, keepdims=True) / np.linalg.norm(perp, axis=1, keepdims=True)
        t["e2"][::10] = (0.75 * e1 + perp).astype(F)
    t["vert"] = (t["vert"] + OFFSET).astype(F)
    return build(t)


def deformed(prims, amplitude):
    """the records a refit test moves the scene to: a wave of `amplitude` along x added to every vert.z, every e1.z half as long again"""
    moved = prims.copy()
    moved["vert"][:, 2] += (amplitude * np.sin(moved["vert"][:, 0] * 0.2)).astype(F)
    moved["e1"][:, 2] *= F(1.5)
    return moved


# ---- the device ---------------------------------------------------------------------------------------------------------
def renderer(hip, nodes, prims, flags=0, spheres=None, n=4096, **tuning):
    g = hip.Renderer(64, 64, n, flags=flags)
    if tuning:
        g.set_tuning(**tuning)
    g.upload(nodes, prims)
    if spheres is not None:
        g.set_spheres(spheres)
    return g


def on_side_stream(fn):
    """fn(side)'s result, with a new torch stream `side` behind the current one made current for the call and synchronised after it"""
    import torch

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = fn(side)
    side.synchronize()
    return res


def query_exists(*entries):
    """the autouse fixture of a module none of whose tests means anything without its entry points"""
    @pytest.fixture(autouse=True)
    def _the_query_exists(hip):
        for entry in entries:
            assert entry in hip.SYMBOLS and hasattr(hip.lib(), entry)

    return _the_query_exists


# ---- comparing an answer ------------------------------------------------------------------------------------------------
def same(names, got, want, what="", dtype=True):
    """every output of `got` (None: one that was not asked for) against `want`: shape, dtype, and every value -- float32 by bits,
    so that NaN equals the same NaN and -0.0 is not 0.0"""
    for name, a, b in zip(names, got, want):
        if a is None:
            continue
        assert a.shape == b.shape, f"{what}: {name} has shape {a.shape}, not {b.shape}"
        assert not dtype or a.dtype == b.dtype, f"{what}: {name} is {a.dtype}, not {b.dtype}"
        if a.dtype == np.float32:
            a, b = bits(a), bits(b)
        assert np.array_equal(a, b), f"{what}: {name} differs at {np.argwhere(a != b)[:5].tolist()} ({np.count_nonzero(a != b)} values)"


def take(ans, idx):
    return tuple(a[idx] for a in ans)


# ---- what the compiler made of the kernels -----------------------------------------------------------------------------
def launch_bounds_blocks(unit, kernel):
    """the blocks per CU that hip/<unit>.hip's __launch_bounds__(kBlock, N) plans for `kernel`"""
    src = open(os.path.join(ROOT, "tyrant_amd", "csrc", "hip", f"{unit}.hip")).read()
    return int(re.search(rf"__launch_bounds__\(kBlock, (\d+)\) {kernel}", src).group(1))


def check_kernel_budget(res, pattern, count, scratch_max, lds_max=None, planned=5):
    """of kernel_resources' records `res`: exactly `count` kernels whose mangled name matches `pattern`, each without vector
    spills, with at most scratch_max bytes of scratch per lane (and lds_max of LDS per block), and with LDS, rounded up to the
    granule it is handed out in, and an occupancy that admit `planned` blocks per CU.  Returns the records."""
    names = [n for n in res if re.search(pattern, n)]
    assert len(names) == count, (pattern, list(res))
    for name in names:
        k = res[name]
        print(name, k)
        assert k["VGPRs Spill"] == 0, k
        assert k["ScratchSize [bytes/lane]"] <= scratch_max, k
        assert lds_max is None or k["LDS Size [bytes/block]"] <= lds_max, k
        per_block = -(-k["LDS Size [bytes/block]"] // LDS_GRANULE) * LDS_GRANULE
        assert LDS_PER_CU // per_block >= planned and k["Occupancy [waves/SIMD]"] >= planned, k
    return [res[n] for n in names]


def assert_kernel_budget(unit, pattern, count, scratch_max, lds_max=None, planned=5):
    return check_kernel_budget(kernel_resources(unit), pattern, count, scratch_max, lds_max, planned)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def header_code():
    """include/tyr_c.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tyr_c.h")).read(), flags=re.S)


def assert_query_abi(hip, entry, out_type, out_struct, n_pointers, defines=()):
    """the header declares `entry`, its out struct `out_type` and every `#define <regex>` of `defines` at ABI version 5; the library
    exports the entry and reports that version; the binding's `out_struct` is n_pointers pointers"""
    code = header_code()
    assert re.search(rf"\bint\s+{entry}\s*\(", code) and re.search(rf"\}}\s*{out_type}\s*;", code)
    for d in defines:
        assert re.search(rf"#define\s+{d}", code), d
    assert re.search(r"#define\s+TYR_ABI_VERSION\s+5\b", code)
    L = hip.lib()
    assert hasattr(L, entry) and entry in hip.SYMBOLS
    assert L.tyr_abi_version() == 5
    assert C.sizeof(out_struct) == n_pointers * C.sizeof(C.c_void_p)


# ---- isolation from the render ------------------------------------------------------------------------------------------
def assert_render_undisturbed(between, queues=True, flags=(0, 0, 0), also=None):
    """three Cornell-box renders (64 x 64, two tyr_render calls of one sample each), the third with between(g) after the first
    call: the same counters and alpha as the first run's, and the same accumulation buffer (and, with `queues`, ray and shadow
    queues) -- bit for bit if the first two runs are, else within rounding.  flags: each run's ctx flags; also(g): one more
    thing to collect.  Returns the runs' (blit buffer, counters, ray queue, shadow queue, also) for what else a module compares."""
    from tyrant_amd import binding, scenes

    sc = scenes.cornell_box()
    nodes, prims = binding.bvh_build(sc.triangles)

    def run(flags, with_queries):
        g = binding.Renderer(64, 64, 4096, flags=flags)
        g.load_scene(sc, nodes, prims)
        g.render(1)
        if with_queries:
            between(g)
        g.render(1)
        q = (g.ray_queue(0, 4096).tobytes(), g.shadow_queue(4096).tobytes()) if queues else (b"", b"")
        out = (g.blit_buffer(), g.counters()) + q + (also(g) if also else None,)
        g.close()
        return out

    runs = run(flags[0], False), run(flags[1], False), run(flags[2], True)
    (b0, k0, q0, s0, _), (b1, k1, q1, s1, _), (bq, kq, qq, sq, _) = runs
    assert kq == k0, {k: (k0[k], kq[k]) for k in k0 if k0[k] != kq[k]}
    assert np.array_equal(bq[:, 3], b0[:, 3])
    if np.array_equal(bits(b0), bits(b1)) and q0 == q1 and s0 == s1:  # the render is bit-reproducible: so must it be with queries in between
        assert np.array_equal(bits(bq), bits(b0)) and qq == q0 and sq == s0
    else:
        assert np.allclose(bq, b0, rtol=1e-5, atol=1e-6)
    return runs
