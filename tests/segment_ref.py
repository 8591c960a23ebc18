"""numpy restatement of tyr_query_segment (include/tyr_c.h "Closest-segment queries"): the reference the GPU tests compare
against bit for bit.  Every operation is one binary64 operation in the specified order, dot and cross as sweep_ref's, divisions
correctly rounded; inputs are binary32 widened exactly.  The query is an argmin over all triangles with no traversal order in
it, so brute force over the uploaded array, in chunks, is the whole oracle.  `truth` is an independent check of the definition
itself: a ternary search on the point-to-triangle distance along the segment, which is convex, and a Moeller-Trumbore crossing
test.  `key32` is hip/segment.hip's pruning key in numpy binary32, operation by operation."""
import numpy as np

from sweep_ref import _closest, _cross, _dot, _sub, corners, records, true_dist  # noqa: F401  (the shared definitions)

F = np.float32
D = np.float64
INF = F(np.inf)
NAMES = ("dist2", "prim", "s", "feature", "region", "on_segment", "on_triangle")


def _clamp01(v):
    v1 = np.where(v > 0, v, 0.0)
    return np.where(v1 < 1, v1, 1.0)


def pair_value(p, q, vert, e1, e2):
    """(F, s, feature, region, x, y) of segments p -> q against triangles (vert, e1, e2), all of shape (..., 3) that broadcast
    against each other: F, s binary64, feature and region uint8, x and y (..., 3) binary64"""
    A, B, C = corners(vert, e1, e2)
    p, q = np.asarray(p, F).astype(D), np.asarray(q, F).astype(D)
    shape = np.broadcast_shapes(p.shape, q.shape, A.shape)
    P0, P1, A, B, C = (np.moveaxis(np.broadcast_to(a, shape), -1, 0) for a in (p, q, A, B, C))
    sh = shape[:-1]
    with np.errstate(all="ignore"):
        e1, e2 = _sub(B, A), _sub(C, A)
        d = _sub(P1, P0)
        held = {"F": np.full(sh, np.inf, D), "s": np.zeros(sh, D), "feature": np.zeros(sh, np.uint8), "region": np.zeros(sh, np.uint8),
                "x": [np.zeros(sh, D) for _ in range(3)], "y": [np.zeros(sh, D) for _ in range(3)]}

        def at(s):
            return [P0[k] + s * d[k] for k in range(3)]

        def offer(ok, Fv, s, feature, region, x, y):
            win = ok & (Fv < held["F"])  # strict: of equal F the lower feature code stays
            held["F"] = np.where(win, Fv, held["F"])
            held["s"] = np.where(win, s, held["s"])
            held["feature"] = np.where(win, np.uint8(feature), held["feature"])
            held["region"] = np.where(win, region, held["region"]).astype(np.uint8)
            held["x"] = [np.where(win, x[k], held["x"][k]) for k in range(3)]
            held["y"] = [np.where(win, y[k], held["y"][k]) for k in range(3)]

        zero, one, yes = np.zeros(sh, D), np.ones(sh, D), np.ones(sh, bool)
        ap0, ap1 = _sub(P0, A), _sub(P1, A)
        # feature 0: the crossing
        n = _cross(e1, e2)
        nn = _dot(n, n)
        h0, h1 = _dot(n, ap0), _dot(n, ap1)
        s = h0 / (h0 - h1)
        x = at(s)
        w = _sub(x, A)
        bv, bw = _dot(_cross(w, e2), n), _dot(_cross(e1, w), n)
        sides = ((h0 <= 0) & (h1 >= 0)) | ((h0 >= 0) & (h1 <= 0))
        offer((nn > 0) & (h0 != h1) & sides & (bv >= 0) & (bw >= 0) & ((bv + bw) <= nn), zero, s, 0, np.uint8(0), x, x)
        # features 1 and 2: the endpoints
        for feature, s, ap in ((1, zero, ap0), (2, one, ap1)):
            Fv, region, c = _closest(ap, e1, e2, A)
            offer(yes, Fv, s, feature, region, at(s), c)
        # features 3, 4 and 5: the edges
        a = _dot(d, d)
        for feature, Q0, Q1, code, code0, code1 in ((3, A, B, 4, 1, 2), (4, A, C, 5, 1, 3), (5, B, C, 6, 2, 3)):
            e, r = _sub(Q1, Q0), _sub(P0, Q0)
            ee, f, c, b = _dot(e, e), _dot(e, r), _dot(d, r), _dot(d, e)
            den = a * ee - b * b
            s_gen = np.where(den > 0, _clamp01((b * f - c * ee) / den), 0.0)
            tn = b * s_gen + f
            s_lo, s_hi = _clamp01(-c / a), _clamp01((b - c) / a)
            t_gen = np.where(tn < 0, 0.0, np.where(tn > ee, 1.0, tn / ee))
            s_g = np.where(tn < 0, s_lo, np.where(tn > ee, s_hi, s_gen))
            a0, e0 = a == 0, ee == 0
            s = np.where(a0, 0.0, np.where(e0, s_lo, s_g))
            t = np.where(a0 & e0, 0.0, np.where(a0, _clamp01(f / ee), np.where(e0, 0.0, t_gen)))
            x = at(s)
            y = [Q0[k] + e[k] * t for k in range(3)]
            xy = _sub(x, y)
            region = np.where((t > 0) & (t < 1), code, np.where(t >= 1, code1, code0)).astype(np.uint8)
            offer(yes, _dot(xy, xy), s, feature, region, x, y)
    return held["F"], held["s"], held["feature"], held["region"], np.stack(held["x"], axis=-1), np.stack(held["y"], axis=-1)


def valid_inputs(p, q, max_dist):
    with np.errstate(invalid="ignore"):
        return np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1) & (max_dist >= 0)


def bound2(max_dist, n):
    """max_dist * max_dist in binary32 per segment, +inf for None"""
    if max_dist is None:
        return np.full(n, INF, F)
    md = np.broadcast_to(np.asarray(max_dist, F), (n,))
    with np.errstate(all="ignore"):
        return (md * md).astype(F)


def shortlist(p, q, prims, chunk_pairs=1 << 20):
    """(segment index, triangle index) of every pair that can hold the least F32 of its segment, in row-major order.  With dA the
    distance of the corner A to the segment and R the longer of the triangle's edges from A, the triangle inequality gives
    (dA - R)^2 <= F <= dA^2; a triangle whose lower bound lies more than 1e-6 (sixteen binary32 steps) above the least upper bound
    of its segment has a larger F32 than that triangle and is neither the winner nor tied with it."""
    vert, e1, e2 = records(prims)
    A, B, C = corners(vert, e1, e2)
    R = np.sqrt(np.maximum(((B - A) ** 2).sum(-1), ((C - A) ** 2).sum(-1)))
    P0, d = p.astype(D), q.astype(D) - p.astype(D)
    dd = (d * d).sum(-1)
    rows, cols = [], []
    step = max(1, chunk_pairs // max(len(A), 1))
    for s in range(0, len(P0), step):
        m = A[None, :, :] - P0[s:s + step, None, :]
        ds, dds = d[s:s + step, None, :], dd[s:s + step, None]
        t = np.clip((m * ds).sum(-1) / np.where(dds > 0, dds, 1.0), 0.0, 1.0)
        dA = np.sqrt(((m - t[..., None] * ds) ** 2).sum(-1))
        lower = np.maximum(dA - R[None, :], 0.0) ** 2
        least = (dA ** 2).min(axis=1, keepdims=True)
        i, j = np.nonzero(lower <= least * (1 + 1e-6) + 1e-30)
        rows.append(i + s)
        cols.append(j)
    return np.concatenate(rows), np.concatenate(cols)


def brute_values(p, q, b2, prims, chunk_pairs=1 << 18, cull=True):
    """(n segments, m triangles) -> per segment: the smallest F32 below b2, the lowest index that has it (-1: none), how many
    triangles have it.  cull: only the pairs of `shortlist` are evaluated (test_shortlist_keeps_every_winner compares the two)."""
    vert, e1, e2 = records(prims)
    n, m = p.shape[0], vert.shape[0]
    if cull and n and m:
        i, j = shortlist(p, q, prims)
        Fv = pair_value(p[i], q[i], vert[j], e1[j], e2[j])[0]
        with np.errstate(over="ignore"):
            F32 = Fv.astype(F)
        F32 = np.where(F32 < b2[i], F32, INF)
        order = np.lexsort((j, F32, i))  # per segment: by value, then by index
        i, j, F32 = i[order], j[order], F32[order]
        head = np.concatenate([[True], i[1:] != i[:-1]])
        best, arg, ties = np.full(n, INF, F), np.full(n, -1, np.int64), np.zeros(n, np.int64)
        found = F32[head] < INF
        seg = i[head][found]
        best[seg], arg[seg] = F32[head][found], j[head][found]
        np.add.at(ties, i, (F32 == best[i]) & (F32 < INF))
        return best, arg, ties
    best = np.full(n, INF, F)
    arg = np.full(n, -1, np.int64)
    ties = np.zeros(n, np.int64)
    step = max(1, chunk_pairs // max(n, 1))
    for s in range(0, m, step):
        Fv = pair_value(p[:, None, :], q[:, None, :], vert[None, s:s + step], e1[None, s:s + step], e2[None, s:s + step])[0]
        with np.errstate(over="ignore"):
            F32 = Fv.astype(F)
        F32 = np.where(F32 < b2[:, None], F32, INF)
        lo = F32.min(axis=1)
        first = F32.argmin(axis=1) + s  # argmin: the first of equal values
        cnt = (F32 == lo[:, None]).sum(axis=1)
        found = lo < INF
        better = found & (lo < best)  # an earlier chunk keeps a tie: the lowest index wins
        ties = np.where(better, cnt, np.where(found & (lo == best), ties + cnt, ties))
        arg = np.where(better, first, arg)
        best = np.where(better, lo, best)
    return best, arg, ties


def answers(p, q, b2, ok, arg, prims):
    """the seven outputs from the winners `arg` (-1: none) of segments whose validity is `ok` and bound is b2"""
    n = p.shape[0]
    dist2 = np.where(ok, b2, INF).astype(F)
    prim = np.full(n, -1, np.int32)
    s = np.zeros(n, F)
    feature, region = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    on_segment, on_triangle = p.copy(), p.copy()
    hit = ok & (arg >= 0)
    if hit.any():
        vert, e1, e2 = records(prims)
        w = arg[hit]
        Fv, sv, fe, re, x, y = pair_value(p[hit], q[hit], vert[w], e1[w], e2[w])
        dist2[hit], prim[hit], s[hit], feature[hit], region[hit] = Fv.astype(F), w.astype(np.int32), sv.astype(F), fe, re
        on_segment[hit], on_triangle[hit] = x.astype(F), y.astype(F)
    return dist2, prim, s, feature, region, on_segment, on_triangle


def segment(p, q, prims, max_dist=None, chunk_pairs=1 << 18):
    """tyr_query_segment's seven outputs: dist2 (n), prim (n) int32, s (n), feature (n) uint8, region (n) uint8, on_segment (n, 3),
    on_triangle (n, 3)"""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    q = np.ascontiguousarray(q, F).reshape(-1, 3)
    n = p.shape[0]
    md = np.full(n, INF, F) if max_dist is None else np.broadcast_to(np.asarray(max_dist, F), (n,))
    ok = valid_inputs(p, q, md)
    b2 = bound2(max_dist, n)
    sp, sq = np.where(ok[:, None], p, F(0)), np.where(ok[:, None], q, F(0))
    if len(prims):
        best, arg, _ = brute_values(sp, sq, np.where(ok, b2, F(0)), prims, chunk_pairs)
    else:
        best, arg = np.full(n, INF, F), np.full(n, -1, np.int64)
    out = answers(p, q, b2, ok, arg, prims)
    hit = ok & (arg >= 0)
    assert np.array_equal(out[0][hit].view(np.uint32), best[hit].view(np.uint32))
    return out


# ---- an independent truth for the definition -----------------------------------------------------------------------------
def truth(p, q, vert, e1, e2, steps=200):
    """(dist, crossing, margin) per pair in binary64: the least distance of a point of the segment to the triangle, by ternary
    search on s in [0, 1] (the distance to a convex set along a straight path is convex), 0 where the segment crosses the
    triangle; crossing by Moeller-Trumbore; margin: how far the crossing is from the rim and from the segment's ends, the least
    of the three barycentric coordinates, t and 1 - t (-1 where the segment is parallel to the plane or a point)"""
    A, B, C = corners(vert, e1, e2)
    p, q = np.asarray(p, F).astype(D), np.asarray(q, F).astype(D)
    d = q - p

    def f(s):
        return true_dist(p + s[:, None] * d, A, B, C)

    n = p.shape[0]
    a, b = np.zeros(n, D), np.ones(n, D)
    for _ in range(steps):
        m1, m2 = a + (b - a) / 3.0, b - (b - a) / 3.0
        left = f(m1) <= f(m2)
        b = np.where(left, m2, b)
        a = np.where(left, a, m1)
    dist = np.minimum(np.minimum(f(np.zeros(n, D)), f(np.ones(n, D))), f(0.5 * (a + b)))
    E1, E2 = B - A, C - A
    with np.errstate(all="ignore"):
        pv = np.cross(d, E2)
        det = (E1 * pv).sum(-1)
        tv = p - A
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, E1)
        v = (d * qv).sum(-1) / det
        t = (E2 * qv).sum(-1) / det
        margin = np.minimum.reduce([u, v, 1.0 - (u + v), t, 1.0 - t])
    margin = np.where(np.isfinite(margin), margin, -1.0)
    crossing = margin >= 0
    return np.where(crossing, 0.0, dist), crossing, margin


# ---- the pruning key ---------------------------------------------------------------------------------------------------
def key32(p, q, lo, hi, slack, floor, big=2.0 ** 60, tiny=2.0 ** -100):
    """hip/segment.hip's segment_key in numpy binary32, operation by operation, for segments p -> q (n, 3) and boxes lo, hi (n, 3):
    (key, D, E) -- the squared reduced bound, the distance bound before the reduction, and the reduction"""
    p, q, lo, hi = (np.asarray(a, F) for a in (p, q, lo, hi))
    with np.errstate(all="ignore"):
        d = (q - p).astype(F)
        dd = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
        m3 = np.maximum(np.abs(p), np.abs(q))
        ms = ((m3[:, 0] + m3[:, 1]).astype(F) + m3[:, 2]).astype(F)
        rdd = np.where((dd >= F(tiny)) & (ms < F(big)), (F(1) / dd).astype(F), F(np.nan)).astype(F)
        g = np.fmax(F(0), np.fmax((lo - np.maximum(p, q)).astype(F), (np.minimum(p, q) - hi).astype(F))).astype(F)
        da = np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(F) + g[:, 2] * g[:, 2]).astype(F)).astype(F)
        c = (F(0.5) * (lo + hi).astype(F)).astype(F)
        h = (F(0.5) * (hi - lo).astype(F)).astype(F)
        hd = np.sqrt(((h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]).astype(F) + h[:, 2] * h[:, 2]).astype(F)).astype(F)
        m = (c - p).astype(F)
        t0 = (((m[:, 0] * d[:, 0] + m[:, 1] * d[:, 1]).astype(F) + m[:, 2] * d[:, 2]).astype(F) * rdd).astype(F)
        t1 = np.where(t0 > 0, t0, F(0))
        t = np.where(t1 < 1, t1, F(1)).astype(F)
        w = (m - (t[:, None] * d).astype(F)).astype(F)
        db = (np.sqrt(((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]).astype(F) + w[:, 2] * w[:, 2]).astype(F)).astype(F) - hd).astype(F)
        b3 = np.maximum(np.abs(lo), np.abs(hi))
        M = (ms + ((b3[:, 0] + b3[:, 1]).astype(F) + b3[:, 2]).astype(F)).astype(F)
        Dv = np.where(~np.isnan(rdd) & (M < F(big)) & (db > da), db, da).astype(F)
        E = ((F(slack) * M).astype(F) + F(floor)).astype(F)
        l0 = (Dv - E).astype(F)
        lb = np.where(l0 > 0, l0, F(0)).astype(F)
        key = (lb * lb).astype(F)
    return key, Dv, E

