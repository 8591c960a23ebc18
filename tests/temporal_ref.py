"""numpy float32 restatement of tyr_temporal (include/tyr_c.h "Temporal reprojection"): the reference the GPU tests compare
against bit for bit.  Every operation is one binary32 operation in the specified order; the four taps are summed by explicit
left-to-right additions."""
import numpy as np

from tyrant_amd.binding import TEMPORAL_DEPTH_TOLERANCE, TEMPORAL_MAX_HISTORY, TEMPORAL_NORMAL_COS

F = np.float32
VERY_FAR = F(1e20)


class History:
    """the ctx's history: hu (H * W, 4) = (v.xyz, n), hg (H * W, 4) = (normal.xyz, depth)"""

    def __init__(self, hu, hg):
        self.hu, self.hg = hu, hg


def temporal(accum, albedo, normal, depth, motion, prev_depth, hist, W, H, max_history=TEMPORAL_MAX_HISTORY, depth_tolerance=TEMPORAL_DEPTH_TOLERANCE,
             normal_cos=TEMPORAL_NORMAL_COS):
    """one call: (out (H * W, 4), history length (H * W,), the next History).  hist None: no history (the first call, or
    TYR_TEMPORAL_RESET)."""
    accum = np.asarray(accum, F).reshape(-1, 4)
    albedo = np.asarray(albedo, F).reshape(-1, 3)
    normal = np.asarray(normal, F).reshape(-1, 3)
    depth = np.asarray(depth, F).reshape(-1)
    motion = np.asarray(motion, F).reshape(-1, 2)
    prev_depth = np.asarray(prev_depth, F).reshape(-1)
    n_pix = W * H
    A = accum[:, 3]
    valid = (A > 0) & (depth < VERY_FAR)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        c = (accum[:, :3] / A[:, None]).astype(F)
        d = np.where(albedo > 0, albedo, F(1.0)).astype(F)
        u = (c / d).astype(F)
        v = u.copy()
        n = np.ones(n_pix, F)
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
            L = np.zeros(n_pix, F)
            Wb = np.zeros(n_pix, F)
            weights = ((gx * gy).astype(F), (fx * gy).astype(F), (gx * fy).astype(F), (fx * fy).astype(F))
            for t in range(4):
                tx, ty = x0 + (t & 1), y0 + (t >> 1)
                ok = inside & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                q = np.where(ok, ty * W + tx, 0)
                h, g = hist.hu[q], hist.hg[q]
                ok &= h[:, 3] > 0
                ok &= np.abs((g[:, 3] - pz).astype(F)) <= tol
                dn = ((g[:, 0] * normal[:, 0] + g[:, 1] * normal[:, 1]) + g[:, 2] * normal[:, 2]).astype(F)
                ok &= dn >= F(normal_cos)
                w = weights[t]
                S = np.where(ok[:, None], (S + w[:, None] * h[:, :3]).astype(F), S)
                L = np.where(ok, (L + w * h[:, 3]).astype(F), L)
                Wb = np.where(ok, (Wb + w).astype(F), Wb)
            took = Wb > 0
            safe = np.where(took, Wb, F(1))
            hx = (S / safe[:, None]).astype(F)
            np1 = ((L / safe).astype(F) + F(1)).astype(F)
            mh = F(max_history)
            ln = np.where(np1 < mh, np1, mh).astype(F)
            k = (F(1) / ln).astype(F)
            blend = (hx + k[:, None] * (u - hx).astype(F)).astype(F)
            v = np.where((took & (ln > 1))[:, None], blend, u).astype(F)
            n = np.where(took, ln, F(1)).astype(F)
    out = np.zeros((n_pix, 4), F)
    out[valid, :3] = (v[valid] * d[valid]).astype(F)
    bg = (A != 0) & ~valid
    out[bg, :3] = c[bg]
    out[A != 0, 3] = 1
    length = np.where(valid, n, F(0)).astype(F)
    hu = np.zeros((n_pix, 4), F)
    hu[valid, :3] = v[valid]
    hu[valid, 3] = n[valid]
    hg = np.concatenate([normal, depth[:, None]], 1).astype(F)
    return out, length, History(hu, hg)
