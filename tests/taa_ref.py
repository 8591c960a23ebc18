"""numpy float32 restatement of tyr_taa (include/tyr_c.h "Temporal anti-aliasing"): the reference the GPU tests compare against
bit for bit.  Every operation is one binary32 operation in the specified order; sums are explicit left-to-right additions in
tap order (never np.sum, which sums pairwise); max and min are the compares the header writes."""
import numpy as np

from tyrant_amd.binding import TAA_ALPHA, TAA_GAMMA

F = np.float32
VERY_FAR = F(1e20)
INF = F(np.inf)


class History:
    """the ctx's TAA history: the last call's output, (H * W, 4) = (rgb, validity 1 / 0)"""

    def __init__(self, h):
        self.h = h


def ycocg(rgb):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (((F(0.25) * r).astype(F) + (F(0.5) * g).astype(F)).astype(F) + (F(0.25) * b).astype(F)).astype(F)
    co = ((F(0.5) * r).astype(F) - (F(0.5) * b).astype(F)).astype(F)
    cg = (((F(0.5) * g).astype(F) - (F(0.25) * r).astype(F)).astype(F) - (F(0.25) * b).astype(F)).astype(F)
    return np.stack([y, co, cg], -1)


def rgb_of(k):
    y, co, cg = k[..., 0], k[..., 1], k[..., 2]
    t = (y - cg).astype(F)
    return np.stack([(t + co).astype(F), (y + cg).astype(F), (t - co).astype(F)], -1)


def catmull_rom(f):
    """the four per-axis weights of a fraction f"""
    ff = (f * f).astype(F)
    w0 = (f * (F(-0.5) + (f * (F(1) - (F(0.5) * f).astype(F)).astype(F)).astype(F)).astype(F)).astype(F)
    w1 = (F(1) + (ff * (F(-2.5) + (F(1.5) * f).astype(F)).astype(F)).astype(F)).astype(F)
    w2 = (f * (F(0.5) + (f * (F(2) - (F(1.5) * f).astype(F)).astype(F)).astype(F)).astype(F)).astype(F)
    w3 = (ff * (F(-0.5) + (F(0.5) * f).astype(F)).astype(F)).astype(F)
    return w0, w1, w2, w3


def taa(color, depth, motion, prev_depth, hist, W, H, alpha=TAA_ALPHA, gamma=TAA_GAMMA, bilinear=False, info=None):
    """one call: (out (H * W, 4), the next History).  hist None: no history (the first call, or TYR_TAA_RESET).  info: a dict
    that receives per-pixel masks of the paths taken (flat bool arrays; "clamp_lo" / "clamp_hi" / "unclamped" are (n, 3), per
    YCoCg channel, "lo" / "hi" / "mn" / "mx" the box, "clamped" the clamped history, "taken" the tap whose motion "m" the pixel takes) -- what the coverage tests count."""
    color = np.asarray(color, F).reshape(-1, 4)
    depth = np.asarray(depth, F).reshape(-1)
    motion = np.asarray(motion, F).reshape(-1, 2)
    prev_depth = np.asarray(prev_depth, F).reshape(-1)
    n_pix = W * H
    alpha, gamma = F(alpha), F(gamma)
    seen = color[:, 3] != 0
    c = color[:, :3]
    out = np.zeros((n_pix, 4), F)
    out[seen, :3] = c[seen]
    out[seen, 3] = 1
    masks = {k: np.zeros(n_pix, bool) for k in ("catmull_rom", "bilinear", "no_history", "dilated", "background")}
    for k in ("clamp_lo", "clamp_hi", "unclamped"):
        masks[k] = np.zeros((n_pix, 3), bool)
    if hist is None:
        masks["no_history"] = seen.copy()
        if info is not None:
            info.update(masks)
        return out, History(out.copy())
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        y, x = np.divmod(np.arange(n_pix), W)
        # the 3 x 3 neighbourhood: box statistics and the nearest tap
        S1, S2 = np.zeros((n_pix, 3), F), np.zeros((n_pix, 3), F)
        cnt = np.zeros(n_pix, F)
        mn, mx = np.full((n_pix, 3), INF, F), np.full((n_pix, 3), -INF, F)
        first = np.ones(n_pix, bool)
        bz = np.zeros(n_pix, F)
        bq = np.arange(n_pix)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                tx, ty = x + dx, y + dy
                ok = seen & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                q = np.where(ok, ty * W + tx, 0)
                ok &= seen[q]
                zq = depth[q]
                take = ok & (first | (zq < bz))
                bz = np.where(take, zq, bz)
                bq = np.where(take, q, bq)
                first &= ~ok
                k = ycocg(c[q])
                o3 = ok[:, None]
                S1 = np.where(o3, (S1 + k).astype(F), S1)
                S2 = np.where(o3, (S2 + (k * k).astype(F)).astype(F), S2)
                cnt = np.where(ok, (cnt + F(1)).astype(F), cnt)
                mn = np.where(o3 & (k < mn), k, mn)
                mx = np.where(o3 & (k > mx), k, mx)
        surface = bz < VERY_FAR
        moving = surface & (prev_depth[bq] < VERY_FAR)
        background = seen & (bz == VERY_FAR)
        m = np.where(moving[:, None], motion[bq], F(0)).astype(F)
        ok = seen & (moving | background) & (np.abs(m[:, 0]) < INF) & (np.abs(m[:, 1]) < INF)
        qx = (x.astype(F) + m[:, 0]).astype(F)
        qy = (y.astype(F) + m[:, 1]).astype(F)
        inside = ok & (qx > F(-1)) & (qx < F(W)) & (qy > F(-1)) & (qy < F(H))
        x0f = np.floor(np.where(inside, qx, F(0))).astype(F)
        y0f = np.floor(np.where(inside, qy, F(0))).astype(F)
        fx = (np.where(inside, qx, F(0)) - x0f).astype(F)
        fy = (np.where(inside, qy, F(0)) - y0f).astype(F)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        hb = hist.h
        # Catmull-Rom over the 4 x 4 footprint
        cr = inside & (x0 >= 1) & (x0 + 2 < W) & (y0 >= 1) & (y0 + 2 < H)
        if bilinear:
            cr = np.zeros(n_pix, bool)
        wx, wy = catmull_rom(fx), catmull_rom(fy)
        footprint = cr.copy()
        Sc = np.zeros((n_pix, 3), F)
        for j in range(4):
            for i in range(4):
                q = np.where(footprint, (y0 - 1 + j) * W + (x0 - 1 + i), 0)
                h = hb[q]
                cr &= h[:, 3] != 0
                w = (wx[i] * wy[j]).astype(F)
                Sc = (Sc + (w[:, None] * h[:, :3]).astype(F)).astype(F)
        # the bilinear taps (tyr_temporal's)
        gx, gy = (F(1) - fx).astype(F), (F(1) - fy).astype(F)
        weights = ((gx * gy).astype(F), (fx * gy).astype(F), (gx * fy).astype(F), (fx * fy).astype(F))
        Sb = np.zeros((n_pix, 3), F)
        Wb = np.zeros(n_pix, F)
        for t in range(4):
            tx, ty = x0 + (t & 1), y0 + (t >> 1)
            acc = inside & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            q = np.where(acc, ty * W + tx, 0)
            h = hb[q]
            acc &= h[:, 3] != 0
            w = weights[t]
            Sb = np.where(acc[:, None], (Sb + (w[:, None] * h[:, :3]).astype(F)).astype(F), Sb)
            Wb = np.where(acc, (Wb + w).astype(F), Wb)
        bil = inside & ~cr & (Wb > 0)
        hbil = (Sb / np.where(bil, Wb, F(1))[:, None]).astype(F)
        have = cr | bil
        h = np.where(cr[:, None], Sc, hbil).astype(F)
        # the box and the clamp, per YCoCg channel
        safe = np.where(cnt > 0, cnt, F(1))[:, None]
        mu = (S1 / safe).astype(F)
        var = ((S2 / safe).astype(F) - (mu * mu).astype(F)).astype(F)
        sd = np.sqrt(np.where(var > 0, var, F(0)).astype(F)).astype(F)
        e = (gamma * sd).astype(F)
        tl, th = (mu - e).astype(F), (mu + e).astype(F)
        l0 = np.where(tl > mn, tl, mn)
        lo = np.where(l0 < mx, l0, mx).astype(F)
        h0 = np.where(th < mx, th, mx)
        hi = np.where(h0 > mn, h0, mn).astype(F)
        hk = ycocg(h)
        t = np.where(hk > lo, hk, lo)
        hc = np.where(t < hi, t, hi).astype(F)
        ck = ycocg(c)
        o = (hc + (alpha * (ck - hc).astype(F)).astype(F)).astype(F)
        out[have, :3] = rgb_of(o)[have]
    if info is not None:
        h3 = have[:, None]
        masks.update(catmull_rom=cr, bilinear=bil, no_history=seen & ~have, dilated=have & moving & (bq != np.arange(n_pix)) & np.any(motion[bq] != motion, axis=1),
                     background=have & background, clamp_lo=h3 & (hc != hk) & (hc == lo), clamp_hi=h3 & (hc != hk) & (hc == hi) & (hc != lo), unclamped=h3 & (hc == hk))
        info.update(masks, lo=lo, hi=hi, mn=mn, mx=mx, clamped=hc, taken=bq, m=m)
    return out, History(out.copy())
