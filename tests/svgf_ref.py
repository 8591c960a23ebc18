"""numpy float32 restatement of tyr_svgf (include/tyr_c.h "SVGF"): the reference the GPU tests compare against bit for bit.
Every operation is one binary32 operation in the specified order; sums are explicit left-to-right additions in tap order
(never np.sum, which sums pairwise)."""
import numpy as np

from denoise_ref import TAPS, _shift, inv_square
from tyrant_amd.binding import (SVGF_DEPTH_TOLERANCE, SVGF_MAX_HISTORY, SVGF_NORMAL_COS, SVGF_NORMAL_POWER_LOG2, SVGF_PASSES, SVGF_SIGMA_DEPTH,
                                SVGF_SIGMA_LUMINANCE)

F = np.float32
VERY_FAR = F(1e20)
GAUSS3 = (F(0.25), F(0.5), F(0.25))


class History:
    """the ctx's SVGF history: hu (H * W, 4) = (pass 0's u.xyz, n), hg (H * W, 4) = (normal.xyz, depth), hm (H * W, 2) = (m1, m2)"""

    def __init__(self, hu, hg, hm):
        self.hu, self.hg, self.hm = hu, hg, hm


def luminance(u):
    return ((F(0.2126) * u[..., 0] + F(0.7152) * u[..., 1]).astype(F) + (F(0.0722) * u[..., 2]).astype(F)).astype(F)


def _normal_term(n, nq, m):
    dn = ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]).astype(F)
    g = np.where(dn > 0, dn, F(0.0)).astype(F)
    for _ in range(m):
        g = (g * g).astype(F)
    return g


def _pos(t):
    """max(0, t): t when t > 0, else +0"""
    return np.where(t > 0, t, F(0.0)).astype(F)


def reproject(accum, albedo, normal, depth, motion, prev_depth, hist, W, H, max_history, depth_tolerance, normal_cos):
    """the temporal stage: (A, valid, c, d, v (n, 3), n, m1, m2) per pixel"""
    accum = np.asarray(accum, F).reshape(-1, 4)
    albedo = np.asarray(albedo, F).reshape(-1, 3)
    normal = np.asarray(normal, F).reshape(-1, 3)
    depth = np.asarray(depth, F).reshape(-1)
    motion = np.asarray(motion, F).reshape(-1, 2)
    prev_depth = np.asarray(prev_depth, F).reshape(-1)
    n_pix = W * H
    A = accum[:, 3]
    valid = (A > 0) & (depth < VERY_FAR)
    c = (accum[:, :3] / A[:, None]).astype(F)
    d = np.where(albedo > 0, albedo, F(1.0)).astype(F)
    u = (c / d).astype(F)
    l = luminance(u)
    l2 = (l * l).astype(F)
    v, m1, m2 = u.copy(), l.copy(), l2.copy()
    ln = np.ones(n_pix, F)
    if hist is not None:
        y, x = np.divmod(np.arange(n_pix), W)
        qx = (x.astype(F) + motion[:, 0]).astype(F)
        qy = (y.astype(F) + motion[:, 1]).astype(F)
        pz = prev_depth
        inside = valid & (pz < VERY_FAR) & (qx > F(-1)) & (qx < F(W)) & (qy > F(-1)) & (qy < F(H))
        x0f = np.floor(np.where(inside, qx, F(0))).astype(F)
        y0f = np.floor(np.where(inside, qy, F(0))).astype(F)
        fx = (np.where(inside, qx, F(0)) - x0f).astype(F)
        fy = (np.where(inside, qy, F(0)) - y0f).astype(F)
        gx, gy = (F(1) - fx).astype(F), (F(1) - fy).astype(F)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tol = (F(depth_tolerance) * pz).astype(F)
        S = np.zeros((n_pix, 3), F)
        L, S1, S2, Wb = (np.zeros(n_pix, F) for _ in range(4))
        weights = ((gx * gy).astype(F), (fx * gy).astype(F), (gx * fy).astype(F), (fx * fy).astype(F))
        for t in range(4):
            tx, ty = x0 + (t & 1), y0 + (t >> 1)
            ok = inside & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            q = np.where(ok, ty * W + tx, 0)
            h, g, hm = hist.hu[q], hist.hg[q], hist.hm[q]
            ok &= h[:, 3] > 0
            ok &= np.abs((g[:, 3] - pz).astype(F)) <= tol
            dn = ((g[:, 0] * normal[:, 0] + g[:, 1] * normal[:, 1]) + g[:, 2] * normal[:, 2]).astype(F)
            ok &= dn >= F(normal_cos)
            w = weights[t]
            S = np.where(ok[:, None], (S + w[:, None] * h[:, :3]).astype(F), S)
            L = np.where(ok, (L + w * h[:, 3]).astype(F), L)
            S1 = np.where(ok, (S1 + w * hm[:, 0]).astype(F), S1)
            S2 = np.where(ok, (S2 + w * hm[:, 1]).astype(F), S2)
            Wb = np.where(ok, (Wb + w).astype(F), Wb)
        took = Wb > 0
        safe = np.where(took, Wb, F(1))
        hx = (S / safe[:, None]).astype(F)
        h1 = (S1 / safe).astype(F)
        h2 = (S2 / safe).astype(F)
        np1 = ((L / safe).astype(F) + F(1)).astype(F)
        mh = F(max_history)
        lt = np.where(np1 < mh, np1, mh).astype(F)
        k = (F(1) / lt).astype(F)
        blend = took & (lt > 1)
        v = np.where(blend[:, None], (hx + k[:, None] * (u - hx).astype(F)).astype(F), u).astype(F)
        m1 = np.where(blend, (h1 + k * (l - h1).astype(F)).astype(F), l).astype(F)
        m2 = np.where(blend, (h2 + k * (l2 - h2).astype(F)).astype(F), l2).astype(F)
        ln = np.where(took, lt, F(1)).astype(F)
    return A, valid, c, d, v, ln, m1, m2


def variance(valid, ln, m1, m2, normal, depth, W, H, kz, m):
    """the variance estimate per pixel (flat), 0 on pixels that are not valid"""
    vm = valid.reshape(H, W)
    n = np.asarray(normal, F).reshape(H, W, 3)
    z = np.asarray(depth, F).reshape(H, W)
    M1, M2 = m1.reshape(H, W), m2.reshape(H, W)
    iz = np.where(vm, F(1.0) / np.where(vm, z, F(1.0)), F(0.0)).astype(F)
    S1, S2, Ws = (np.zeros((H, W), F) for _ in range(3))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            take = vm & _shift(vm, dy, dx, False)
            m1q, m2q = _shift(M1, dy, dx, 0), _shift(M2, dy, dx, 0)
            if dx == 0 and dy == 0:
                w = np.ones((H, W), F)
            else:
                g = _normal_term(n, _shift(n, dy, dx, 0), m)
                r = ((_shift(z, dy, dx, 0) - z) * iz).astype(F)
                xz = ((r * r) * kz).astype(F)
                w = (g / (F(1.0) + xz)).astype(F)
            S1 = np.where(take, S1 + w * m1q, S1).astype(F)
            S2 = np.where(take, S2 + w * m2q, S2).astype(F)
            Ws = np.where(take, Ws + w, Ws).astype(F)
    Ws = np.where(Ws > 0, Ws, F(1.0))
    A1, A2 = (S1 / Ws).astype(F), (S2 / Ws).astype(F)
    spatial = (_pos((A2 - A1 * A1).astype(F)) * (F(4.0) / ln.reshape(H, W)).astype(F)).astype(F).reshape(-1)
    temporal = _pos((m2 - m1 * m1).astype(F))
    var = np.where(ln >= 4, temporal, spatial).astype(F)
    return np.where(valid, var, F(0.0)).astype(F)


def atrous(u, var, valid, normal, depth, W, H, passes, sl2, kz, m):
    """the variance-guided passes: (the last pass's u, pass 0's u), both (H * W, 3)"""
    vm = valid.reshape(H, W)
    n = np.asarray(normal, F).reshape(H, W, 3)
    z = np.asarray(depth, F).reshape(H, W)
    u = u.reshape(H, W, 3).copy()
    var = var.reshape(H, W).copy()
    iz = np.where(vm, F(1.0) / np.where(vm, z, F(1.0)), F(0.0)).astype(F)
    first = None
    for j in range(passes):
        s = 1 << j
        gs, gw = np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                take = vm & _shift(vm, dy, dx, False)
                k = F(GAUSS3[dx + 1] * GAUSS3[dy + 1])
                gs = np.where(take, gs + k * _shift(var, dy, dx, 0), gs).astype(F)
                gw = np.where(take, gw + k, gw).astype(F)
        gv = (gs / np.where(gw > 0, gw, F(1.0))).astype(F)
        kl = (F(1.0) / ((sl2 * gv).astype(F) + F(1e-10))).astype(F)
        lum = luminance(u)
        S = np.zeros((H, W, 3), F)
        V, Ws = np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ddy, ddx = dy * s, dx * s
                take = vm & _shift(vm, ddy, ddx, False)
                uq, vq = _shift(u, ddy, ddx, 0), _shift(var, ddy, ddx, 0)
                h = F(TAPS[dx + 2] * TAPS[dy + 2])
                dl = (_shift(lum, ddy, ddx, 0) - lum).astype(F)
                g = _normal_term(n, _shift(n, ddy, ddx, 0), m)
                r = ((_shift(z, ddy, ddx, 0) - z) * iz).astype(F)
                xz = ((r * r) * kz).astype(F)
                den = ((F(1.0) + ((dl * dl).astype(F) * kl).astype(F)) * (F(1.0) + xz)).astype(F)
                w = ((h * g) / den).astype(F)
                S = np.where(take[..., None], S + w[..., None] * uq, S).astype(F)
                V = np.where(take, V + (w * w).astype(F) * vq, V).astype(F)
                Ws = np.where(take, Ws + w, Ws).astype(F)
        took = vm & (Ws > 0)
        safe = np.where(Ws > 0, Ws, F(1.0))
        u = np.where(took[..., None], (S / safe[..., None]).astype(F), u).astype(F)
        var = np.where(took, (V / (safe * safe).astype(F)).astype(F), var).astype(F)
        if j == 0:
            first = u.copy()
    return u.reshape(-1, 3), first.reshape(-1, 3)


def svgf(accum, albedo, normal, depth, motion, prev_depth, hist, W, H, max_history=SVGF_MAX_HISTORY, depth_tolerance=SVGF_DEPTH_TOLERANCE,
         normal_cos=SVGF_NORMAL_COS, passes=SVGF_PASSES, sigma_luminance=SVGF_SIGMA_LUMINANCE, sigma_depth=SVGF_SIGMA_DEPTH, m=SVGF_NORMAL_POWER_LOG2):
    """one call: (out (H * W, 4) linear, variance (H * W,), the next History).  hist None: no history (the first call, or
    TYR_SVGF_RESET)."""
    normal = np.asarray(normal, F).reshape(-1, 3)
    depth = np.asarray(depth, F).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        A, valid, c, d, v, ln, m1, m2 = reproject(accum, albedo, normal, depth, motion, prev_depth, hist, W, H, max_history, depth_tolerance, normal_cos)
        sl2 = F(F(sigma_luminance) * F(sigma_luminance))
        kz = inv_square(sigma_depth)
        var = variance(valid, ln, m1, m2, normal, depth, W, H, kz, m)
        ul, u0 = atrous(np.where(valid[:, None], v, F(0)), var, valid, normal, depth, W, H, passes, sl2, kz, m)
        out = np.zeros((W * H, 4), F)
        out[valid, :3] = (ul[valid] * d[valid]).astype(F)
    bg = (A != 0) & ~valid
    out[bg, :3] = c[bg]
    out[A != 0, 3] = 1
    hu = np.zeros((W * H, 4), F)
    hu[valid, :3] = u0[valid]
    hu[valid, 3] = ln[valid]
    hg = np.concatenate([normal, depth[:, None]], 1).astype(F)
    hm = np.zeros((W * H, 2), F)
    hm[:, 1] = -1
    hm[valid, 0] = m1[valid]
    hm[valid, 1] = m2[valid]
    return out, var, History(hu, hg, hm)
