"""tyr_query_occlusion (include/tyr_c.h "Occlusion queries") restated in numpy, so that the GPU kernels have a specification
that is not another HIP kernel: uint32 arithmetic for the hash and the xorshift, binary32 everywhere else, one operation per
line.  The pieces the project already pins to the reference come from the oracle: RandomFloat and orthonormal_basis_naive
(orc_sampler_map ops 0, 4 and 5 -- what the device's probe ops 44, 48 and 49 are compared with), the render's sin / cos
(orc_dm_map "sincos"), glm's dot and normalize (orc_glm), and the any-hit traversal itself (the reference's own bvh.h where its
harness is built, else the oracle's restatement of it)."""
from __future__ import annotations

import ctypes as C

import numpy as np

F = np.float32
U = np.uint32
VERY_FAR = F(1e20)
EPSILON = F(1e-3)
TWO_PI = F(2.0) * F(3.1415926535897932)  # (2.f * PI): exact, a power of two times PI


def _pyorc():
    from oracle import pyorc

    pyorc.lib()
    return pyorc


def glm(op, a, b=None):
    """orc_glm on (n, 3) float32 arrays: 0 dot (in column 0), 2 normalize (tests/specular_ref.py)"""
    lib = _pyorc().lib()
    a = np.ascontiguousarray(a, dtype=F).reshape(-1, 3)
    b = a if b is None else np.ascontiguousarray(b, dtype=F).reshape(-1, 3)
    out = np.zeros_like(a)
    if a.shape[0]:
        assert lib.orc_glm(op, a.ctypes.data, b.ctypes.data, a.ctypes.data, a.shape[0], out.ctypes.data) == 0
    return out


def dot(a, b):
    return glm(0, a, b)[:, 0]


def normalize(a):
    return glm(2, a)


def h(x):
    """the hash of the contract on uint32 arrays, wrapping"""
    x = np.array(x, dtype=U)
    x ^= x >> U(16)
    x *= U(0x7FEB352D)
    x ^= x >> U(15)
    x *= U(0x846CA68B)
    x ^= x >> U(16)
    return x


def states(seed, i, s):
    """state(i, s) = h(h(seed ^ i) + s) for index array i (n,) and sample array s (S,): (n, S) uint32"""
    i, s = np.asarray(i, dtype=U), np.asarray(s, dtype=U)
    return h(h(U(seed & 0xFFFFFFFF) ^ i)[:, None] + s[None, :])


def rng_float(state):
    """RandomFloat (kernel.cu:23-36) on a flat uint32 array: (float32 values, states after)"""
    w = np.zeros((state.size, 3), dtype=U)
    w[:, 0] = state.reshape(-1)
    out = _pyorc().sampler_map(0, w)
    return out[:, 0].copy().view(F), out[:, 1].copy()


def basis(w):
    """orthonormal_basis_naive (kernel.cu:181-189) of (n, 3) float32 unit vectors: (u, v)"""
    words = np.ascontiguousarray(w, dtype=F).view(U)
    P = _pyorc()
    return P.sampler_map(4, words).view(F), P.sampler_map(5, words).view(F)


def frames(points, normals, bias):
    """valid (n,), o, w, u, v (n, 3): what a point's samples share"""
    p, nr = np.ascontiguousarray(points, dtype=F), np.ascontiguousarray(normals, dtype=F)
    with np.errstate(all="ignore"):
        nn = dot(nr, nr)
        valid = np.isfinite(p).all(axis=1) & np.isfinite(nr).all(axis=1) & np.isfinite(nn) & (nn > 0)
        safe = np.where(valid[:, None], nr, F([0, 0, 1])).astype(F)
        w = normalize(safe)
        lift = (w * F(bias)).astype(F)
        o = (p + lift).astype(F)
        u, v = basis(w)
    return valid, o, w, u, v


def directions(w, u, v, seed, index, samples):
    """d of every (point, sample): (n, S, 3) float32.  index: the points' indices in the caller's batch"""
    n, S = w.shape[0], int(samples)
    st = states(seed, index, np.arange(S)).reshape(-1)
    u1, st = rng_float(st)
    u2, st = rng_float(st)
    r1 = (TWO_PI * u1).astype(F)
    r2s = np.sqrt(u2).astype(F)
    sc = _pyorc().dm_map("sincos", r1)
    s1, c1 = sc["sin"].view(F), sc["cos"].view(F)
    one_minus = (F(1.0) - u2).astype(F)
    with np.errstate(all="ignore"):
        cz = np.sqrt(one_minus).astype(F)
    rep = lambda a: np.repeat(a, S, axis=0)
    a = ((rep(u) * c1[:, None]).astype(F) * r2s[:, None]).astype(F)
    b = ((rep(v) * s1[:, None]).astype(F) * r2s[:, None]).astype(F)
    c = (rep(w) * cz[:, None]).astype(F)
    with np.errstate(all="ignore"):
        d = normalize(((a + b).astype(F) + c).astype(F))
    return d.reshape(n, S, 3)


# ---- the reference's any-hit, as tests/test_ray_query.py's oracle_any / oracle_spheres_any get it --------------------------
def oracle_any(nodes, prims, o, d, tmax):
    """intersectSimple(ray, closestAllowed = tmax) (bvh.h:213-256)"""
    from tyrant_amd import scenes

    orc = _pyorc()
    n = o.shape[0]
    s = np.zeros(n, dtype=scenes.SHADOW_DTYPE)
    s["origin"], s["direction"], s["closestDistance"] = o, d, tmax
    nodes, prims = np.ascontiguousarray(nodes), np.ascontiguousarray(prims)
    hit = np.zeros(n, dtype=np.int32)
    if nodes.shape[0] == 0 or prims.shape[0] == 0:  # a scene without triangles (Scene.cpp:49-52)
        return hit != 0
    R = orc.ref()
    if R is not None:
        R.ref_bvh_intersect_simple(nodes.ctypes.data, prims.ctypes.data, s.ctypes.data, n, hit.ctypes.data_as(C.POINTER(C.c_int)))
    else:
        f = orc.lib().orc_bvh_intersect_simple
        pn, pp, base, size = nodes.ctypes.data, prims.ctypes.data, s.ctypes.data, s.dtype.itemsize
        for i in range(n):
            hit[i] = f(pn, pp, base + i * size, float(tmax[i]), None)
    return hit != 0


def oracle_spheres_any(spheres, nodes, prims, o, d, tmax):
    """intersect_scene_simple (kernel.cu:163-174)"""
    occ = oracle_any(nodes, prims, o, d, tmax)
    f = _pyorc().lib().orc_sphere_intersect
    sp = np.ascontiguousarray(spheres)
    fp = C.POINTER(C.c_float)
    for i in np.nonzero(~occ)[0]:
        oi, di = np.ascontiguousarray(o[i]), np.ascontiguousarray(d[i])
        for k in range(6, -1, -1):
            t = np.float32(f(sp[k:k + 1].ctypes.data, oi.ctypes.data_as(fp), di.ctypes.data_as(fp)))
            with np.errstate(all="ignore"):
                if t != 0 and (t + EPSILON) < tmax[i]:
                    occ[i] = True
                    break
    return occ


def occlusion(nodes, prims, points, normals, samples, max_dist=None, bias=1e-3, seed=0, spheres=None, first=0):
    """(visible uint32 (n,), mask uint32 (n, W), bent float32 (n, 3), origin (n, 3), direction (n, S, 3)) of the contract.
    spheres: the ctx's sphere table with TYR_QUERY_SPHERES, else None.  first: the batch index of points[0]"""
    p = np.ascontiguousarray(points, dtype=F)
    n, S = p.shape[0], int(samples)
    W = (S + 31) // 32
    index = (np.arange(n, dtype=np.uint64) + np.uint64(first)).astype(U)
    valid, o, w, u, v = frames(p, normals, bias)
    d = directions(w, u, v, seed, index, S)
    d[~valid] = 0
    origin = np.where(valid[:, None], o, p).astype(F)
    tmax = np.full(n, VERY_FAR, F) if max_dist is None else np.ascontiguousarray(max_dist, dtype=F)
    ro, rd, rt = np.repeat(origin, S, axis=0), d.reshape(-1, 3), np.repeat(tmax, S)
    is_ray = np.repeat(valid, S) & np.isfinite(ro).all(axis=1) & np.isfinite(rd).all(axis=1)  # (else: a miss, as tyr_query_any)
    blocked = np.zeros(n * S, dtype=bool)
    idx = np.nonzero(is_ray)[0]
    if idx.size:
        if spheres is None:
            blocked[idx] = oracle_any(nodes, prims, ro[idx], rd[idx], rt[idx])
        else:
            blocked[idx] = oracle_spheres_any(spheres, nodes, prims, ro[idx], rd[idx], rt[idx])
    vis = (~blocked).reshape(n, S) & valid[:, None]
    visible = vis.sum(axis=1).astype(U)
    mask = np.zeros((n, W), dtype=U)
    bent = np.zeros((n, 3), dtype=F)
    for s in range(S):
        mask[:, s // 32] |= vis[:, s].astype(U) << U(s % 32)
        bent = np.where(vis[:, s, None], (bent + d[:, s]).astype(F), bent)
    return visible, mask, bent, origin, d
