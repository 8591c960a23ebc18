"""numpy float32 restatement of tyr_denoise's linear output (include/tyr_c.h "Denoiser"): the reference the GPU tests
compare against bit for bit.  Every operation is one binary32 operation in the specified order; sums are explicit left-to-right
additions (never np.sum, which sums pairwise)."""
import numpy as np

from tyrant_amd.binding import DENOISE_NORMAL_POWER_LOG2, DENOISE_PASSES, DENOISE_SIGMA_COLOR, DENOISE_SIGMA_DEPTH

F = np.float32
VERY_FAR = F(1e20)
TAPS = (F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))


def inv_square(sigma):
    s = F(sigma)
    return F(F(1.0) / F(s * s))


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] inside the frame, `fill` outside"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return b


def prepare(accum, albedo, depth):
    """(u, d, valid, A): the illumination, the albedo divisor, the tap mask and the sample count, per pixel (flat arrays)"""
    accum = np.asarray(accum, F).reshape(-1, 4)
    albedo = np.asarray(albedo, F).reshape(-1, 3)
    depth = np.asarray(depth, F).reshape(-1)
    A = accum[:, 3]
    valid = (A > 0) & (depth < VERY_FAR)
    d = np.where(albedo > 0, albedo, F(1.0)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (accum[:, :3] / A[:, None]).astype(F)
        u = (c / d).astype(F)
    u[A == 0] = 0
    return u, d, valid, A


def denoise(accum, albedo, normal, depth, W, H, passes=DENOISE_PASSES, sigma_color=DENOISE_SIGMA_COLOR, sigma_depth=DENOISE_SIGMA_DEPTH, m=DENOISE_NORMAL_POWER_LOG2):
    """the linear output, (H * W, 4) float32"""
    u, d, valid, A = prepare(accum, albedo, depth)
    n = np.asarray(normal, F).reshape(H, W, 3)
    z = np.asarray(depth, F).reshape(H, W)
    u = u.reshape(H, W, 3)
    valid = valid.reshape(H, W)
    with np.errstate(divide="ignore"):
        iz = np.where(valid, F(1.0) / np.where(valid, z, F(1.0)), F(0.0)).astype(F)
    kc, kz = inv_square(sigma_color), inv_square(sigma_depth)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j in range(passes):
            s = 1 << j
            kcj = F(kc * F(4 ** j))
            S = np.zeros((H, W, 3), F)
            Ws = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    uq = _shift(u, dy * s, dx * s, 0)
                    nq = _shift(n, dy * s, dx * s, 0)
                    zq = _shift(z, dy * s, dx * s, 0)
                    take = valid & _shift(valid, dy * s, dx * s, False)
                    h = F(TAPS[dx + 2] * TAPS[dy + 2])
                    e = (uq - u).astype(F)
                    dc2 = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F)
                    dn = ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]).astype(F)
                    g = np.where(dn > 0, dn, F(0.0)).astype(F)
                    for _ in range(m):
                        g = (g * g).astype(F)
                    r = ((zq - z) * iz).astype(F)
                    xz = ((r * r) * kz).astype(F)
                    den = ((F(1.0) + dc2 * kcj) * (F(1.0) + xz)).astype(F)
                    w = ((h * g) / den).astype(F)
                    S = np.where(take[..., None], S + w[..., None] * uq, S).astype(F)
                    Ws = np.where(take, Ws + w, Ws).astype(F)
            with np.errstate(divide="ignore"):
                new = (S / np.where(Ws > 0, Ws, F(1.0))[..., None]).astype(F)
            u = np.where((valid & (Ws > 0))[..., None], new, u).astype(F)
    out = np.zeros((H * W, 4), F)
    out[:, :3] = (u.reshape(-1, 3) * d).astype(F)
    out[:, 3] = 1
    out[A == 0] = 0
    return out
