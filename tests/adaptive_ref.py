"""Adaptive sampling restated in numpy (include/tyr_c.h "Adaptive sampling"): the sample-major ticket list of a sample map and
the allocator's exact rule, with Python integers where the rule says exact integers and float32 where it says binary32."""
import ctypes as C

import numpy as np

QUANT = 1048576


def local_rows(a, rank=0, nranks=1):
    """the rows y = yl * nranks + rank of an (H, W) frame, flattened in local pixel order"""
    return np.ascontiguousarray(np.asarray(a)[rank::nranks]).reshape(-1)


def ticket_list(counts_local):
    """L: pass s = 0, 1, ... lists the local pixels p with c[p] > s in increasing order; the passes end to end"""
    c = np.asarray(counts_local, dtype=np.int64).reshape(-1)
    if c.size == 0 or c.max(initial=0) <= 0:
        return np.zeros(0, dtype=np.uint32)
    passes = [np.nonzero(c > s)[0] for s in range(int(c.max()))]
    return np.concatenate(passes).astype(np.uint32)


def ticket_pixels(counts_local, first, n):
    """L[first : first + n] without building all of L (a map with a large count): the pixels of tickets first .. first + n - 1"""
    c = np.asarray(counts_local, dtype=np.int64).reshape(-1)
    out = []
    t, s = 0, 0
    want_end = first + n
    while t < want_end:
        members = np.nonzero(c > s)[0]
        if members.size == 0:
            break
        # the pass's content only changes where some member's count ends: skip whole runs of equal passes at once
        run = int(c[members].min()) - s
        span = members.size * run
        if t + span > first:
            lo, hi = max(first - t, 0), min(want_end - t, span)
            idx = np.arange(lo, hi)
            out.append(members[idx % members.size])
        t += span
        s += run
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, dtype=np.uint32)


def usable(err_local):
    v = np.asarray(err_local, dtype=np.float32).reshape(-1)
    ok = np.isfinite(v) & (v > 0)
    return np.where(ok, v, np.float32(0)).astype(np.float32)


def weights(err_local):
    v = usable(err_local)
    m = v.max(initial=np.float32(0))
    if m > 0:
        with np.errstate(over="ignore"):
            s = np.float32(QUANT) / np.float32(m)  # one binary32 division
        if not np.isfinite(s):  # m below ~3.1e-33: every usable error gets the full weight
            return np.where(v > 0, QUANT, 0).astype(np.int64)
        f = np.floor((v * s).astype(np.float32))
        return np.where(f < QUANT, f, QUANT).astype(np.int64)
    return np.ones(v.size, dtype=np.int64)


def allocate(err_local, total, min_spp, max_spp):
    """(map over the local pixels, extras before the max_spp clamp), exact integers"""
    q = weights(err_local)
    P = q.size
    Q = [0]
    acc = 0
    for x in q.tolist():
        acc += x
        Q.append(acc)
    E = total - min_spp * P if total > min_spp * P else 0
    Qt = Q[-1]
    extra = np.array([E * Q[i + 1] // Qt - E * Q[i] // Qt for i in range(P)], dtype=np.int64)
    c = np.minimum(min_spp + extra, max_spp)
    return c.astype(np.int64), extra


def two_buffer_error(a, b):
    """per-pixel rgb L2 distance between the means of two blit buffers ((P, 4): rgb sums, count)"""
    ma = a[:, :3] / np.maximum(a[:, 3:4], 1)
    mb = b[:, :3] / np.maximum(b[:, 3:4], 1)
    return np.sqrt(np.sum((ma.astype(np.float64) - mb) ** 2, axis=1)).astype(np.float32)


def box3(e):
    """3 x 3 box filter of an (H, W) field, edges clamped (float32)"""
    e = np.asarray(e, dtype=np.float32)
    p = np.pad(e, 1, mode="edge")
    H, W = e.shape
    return (sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) / np.float32(9)).astype(np.float32)


# ---- the camera rays of kernel.cu:258-297 in float32, with the oracle library's own samplers ---------------------------------


def _f3(a):
    return np.asarray(a, dtype=np.float32).reshape(3)


def _dot(a, b):
    t = a * b  # float32 products, then (x + y) + z
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0], x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], axis=-1)


def _normalize(v):
    return v * (np.float32(1) / np.sqrt(_dot(v, v)))[..., None]  # glm: v * (1 / sqrt(dot(v, v)))


def camera_basis(cam, W, H):
    """orc_stage_begin's rule (kernel.cu:699-700): right = normalize(cross(dir, up)) * 1.5 * (W / H), up = normalize(cross(right, dir)) * 1.5"""
    d, u = _f3(cam.direction), _f3(cam.up)
    right = (_normalize(_cross(d, u)) * np.float32(1.5)) * (np.float32(W) / np.float32(H))
    up = _normalize(_cross(right, d)) * np.float32(1.5)
    return right.astype(np.float32), up.astype(np.float32)


def camera_seed(frame, index, rank=0, nranks=1):
    return ((((frame * 147565741) & 0xFFFFFFFF) * 720898027) & 0xFFFFFFFF) * ((index * nranks + rank) & 0xFFFFFFFF) & 0xFFFFFFFF


def camera_rays(orc_lib, cam, W, H, pixels_local, indices, frame, rank=0, nranks=1):
    """origin, direction (n, 3) float32 and the pixel index y * W + x of the camera rays made at launch `indices` for the local
    pixels `pixels_local` (rows y = yl * nranks + rank), as kernel.cu:258-297 and orc_stage_primary make them"""
    pixels_local = np.asarray(pixels_local, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    n = pixels_local.size
    s2 = np.zeros((n, 2), np.float32)
    lens = np.zeros((n, 2), np.float32)
    disk = np.zeros((n, 2), np.float32)
    seed = C.c_uint32(0)
    out2 = (C.c_float * 2)()
    lu = (C.c_float * 2)()
    for k in range(n):
        seed.value = camera_seed(frame, int(indices[k]), rank, nranks)
        orc_lib.orc_random_2d_stratified_sample(C.byref(seed), out2)
        s2[k] = out2[0], out2[1]
        lu[0] = orc_lib.orc_random_float(C.byref(seed))
        lu[1] = orc_lib.orc_random_float(C.byref(seed))
        orc_lib.orc_concentric_sample_disk(lu, out2)
        lens[k] = lu[0], lu[1]
        disk[k] = out2[0], out2[1]
    x = pixels_local % W
    y = (pixels_local // W) * nranks + rank
    f32 = np.float32
    jx = x.astype(f32) - s2[:, 0]
    jy = y.astype(f32) - s2[:, 1]
    ni = (jx / f32(W)) - f32(0.5)
    nj = ((f32(H) - jy) / f32(H)) - f32(0.5)
    right, up = camera_basis(cam, W, H)
    O, fwd = _f3(cam.position), _f3(cam.direction)
    toward = (fwd[None, :] + ni[:, None] * right[None, :]) + nj[:, None] * up[None, :]
    toward = _normalize(toward)
    focus = O[None, :] + (f32(cam.focalDistance) * f32(3))[None] * toward
    pLx, pLy = f32(cam.lensRadius) * disk[:, 0], f32(cam.lensRadius) * disk[:, 1]
    origin = (O[None, :] + right[None, :] * pLx[:, None]) + up[None, :] * pLy[:, None]
    direction = _normalize(focus - origin)
    return origin.astype(f32), direction.astype(f32), (y * W + x).astype(np.int32)
