"""numpy restatement of tyr_query_sweep_capsule (include/tyr_c.h "Swept-capsule queries"): the reference the GPU tests compare
against bit for bit.  Every operation is one binary64 operation in the specified order, dot and cross as sweep_ref's, divisions
and square roots correctly rounded; inputs are binary32 widened exactly.  The query is an argmin over all triangles with no
traversal order in it, so brute force over the uploaded array is the whole oracle; `shortlist` leaves out only pairs whose
boxes are apart, which have no value.  `truth` is an independent check of the definition itself: the clearance of the moved
axis (segment_ref's pair distance minus r) sampled along the path and bisected.  `key32` is hip/sweep_capsule.hip's pruning
key in numpy binary32, operation by operation."""
import numpy as np

import segment_ref
from sweep_ref import _cross, _dot, _sub, corners, records

F = np.float32
D = np.float64
INF = F(np.inf)
NAMES = ("t", "prim", "s", "feature", "region", "point", "center", "normal")


def pair_value(p, q, d, radius, tmax, vert, e1, e2):
    """(hit, t, s, feature, region, point) of capsules (p, q, d, radius, tmax) against triangles (vert, e1, e2): p, q, d, vert,
    e1, e2 of shape (..., 3) and radius, tmax of shape (...) that broadcast against each other.  t is binary64 (+inf where the
    pair has no value), s binary64, feature and region uint8, point (..., 3) binary64."""
    p32, q32 = np.asarray(p, F), np.asarray(q, F)
    A, B, C = corners(vert, e1, e2)
    p, q, d = p32.astype(D), q32.astype(D), np.asarray(d, F).astype(D)
    radius, tmax = np.asarray(radius, F).astype(D), np.asarray(tmax, F).astype(D)
    shape = np.broadcast_shapes(p.shape, q.shape, d.shape, A.shape, radius.shape + (3,), tmax.shape + (3,))
    sh = shape[:-1]
    o, P1, d, A, B, C = (np.moveaxis(np.broadcast_to(x, shape), -1, 0) for x in (p, q, d, A, B, C))
    radius, tmax = np.broadcast_to(radius, sh), np.broadcast_to(tmax, sh)
    with np.errstate(all="ignore"):
        a = _sub(P1, o)
        na = [-a[k] for k in range(3)]
        E1, E2, E3 = _sub(B, A), _sub(C, A), _sub(C, B)
        rr = radius * radius
        dd = _dot(d, d)
        held = {"t": np.full(sh, np.inf, D), "s": np.zeros(sh, D), "feature": np.zeros(sh, np.uint8), "region": np.zeros(sh, np.uint8),
                "point": [np.zeros(sh, D) for _ in range(3)]}
        zero, one = np.zeros(sh, D), np.ones(sh, D)

        def offer(ok, t, feature, s, region, point):
            win = ok & (t >= 0) & (t <= tmax) & (t < held["t"])  # strict: of equal t the lower feature code stays
            held["t"] = np.where(win, t, held["t"])
            held["s"] = np.where(win, s, held["s"])
            held["feature"] = np.where(win, np.uint8(feature), held["feature"])
            held["region"] = np.where(win, np.uint8(region), held["region"])
            held["point"] = [np.where(win, point[k], held["point"][k]) for k in range(3)]

        # the six vertex vectors, with what the vertex and edge candidates share: md = dot(m, d), cv = dot(m, m) - rr
        Am, Bm, Cm = _sub(A, a), _sub(B, a), _sub(C, a)
        mv = {name: _sub(o, V) for name, V in (("A", A), ("B", B), ("C", C), ("Am", Am), ("Bm", Bm), ("Cm", Cm))}
        md = {k: _dot(m, d) for k, m in mv.items()}
        cv = {k: _dot(m, m) - rr for k, m in mv.items()}

        def face(n, O, m, F1, F2):
            """the sweep block's face with the origin O (m = o - O) and the edges F1, F2: (conditions but containment, t, contact, bv, bw, nn)"""
            nn = _dot(n, n)
            ln = np.sqrt(nn)
            h = _dot(n, m)
            sgn = np.where(h >= 0, 1.0, -1.0)
            sdn = sgn * _dot(n, d)
            ah = np.abs(h)
            rl = radius * ln
            t = (ah - rl) / (-sdn)
            k = (sgn * radius) / ln
            c = [(o[i] + t * d[i]) - n[i] * k for i in range(3)]
            w = _sub(c, O)
            bv, bw = _dot(_cross(w, F2), n), _dot(_cross(F1, w), n)
            return (nn > 0) & (sdn < 0) & (ah > rl) & (bv >= 0) & (bw >= 0), t, c, bv, bw, nn

        # features 0 and 1: the cap faces
        n = _cross(E1, E2)
        ok, t, c, bv, bw, nn = face(n, A, mv["A"], E1, E2)
        offer(ok & ((bv + bw) <= nn), t, 0, zero, 0, c)
        ok, t, c, bv, bw, nn = face(n, Am, mv["Am"], E1, E2)
        offer(ok & ((bv + bw) <= nn), t, 1, one, 0, [c[k] + a[k] for k in range(3)])
        # features 2, 3, 4: the side faces
        for feature, O, key, e, region in ((2, A, "A", E1, 4), (3, A, "A", E2, 5), (4, B, "B", E3, 6)):
            ok, t, c, bv, bw, nn = face(_cross(e, na), O, mv[key], e, na)
            u, v = bv / nn, bw / nn
            offer(ok & (bv <= nn) & (bw <= nn), t, feature, v, region, [O[k] + e[k] * u for k in range(3)])
        # features 5 .. 10: the vertices
        for feature, key, V, s, region in ((5, "A", A, zero, 1), (6, "B", B, zero, 2), (7, "C", C, zero, 3), (8, "Am", A, one, 1), (9, "Bm", B, one, 2), (10, "Cm", C, one, 3)):
            b, cc = md[key], cv[key]
            disc = b * b - dd * cc
            t = (-b - np.sqrt(disc)) / dd
            offer((dd > 0) & (b < 0) & (cc > 0) & (disc >= 0), t, feature, s, region, V)

        # features 11 .. 19: the edges
        def edge(key, e):
            m = mv[key]
            ee, de, me = _dot(e, e), _dot(d, e), _dot(m, e)
            qa = ee * dd - de * de
            b = ee * md[key] - de * me
            cc = ee * cv[key] - me * me
            disc = b * b - qa * cc
            t = (-b - np.sqrt(disc)) / qa
            sg = (me + t * de) / ee
            return (ee > 0) & (qa > 0) & (b < 0) & (cc > 0) & (disc >= 0) & (sg >= 0) & (sg <= 1), t, sg

        for feature, key, V0, e, s, region in ((11, "A", A, E1, zero, 4), (12, "A", A, E2, zero, 5), (13, "B", B, E3, zero, 6),
                                               (14, "Am", A, E1, one, 4), (15, "Am", A, E2, one, 5), (16, "Bm", B, E3, one, 6)):
            ok, t, sg = edge(key, e)
            offer(ok, t, feature, s, region, [V0[k] + e[k] * sg for k in range(3)])
        for feature, key, V, region in ((17, "A", A, 1), (18, "B", B, 2), (19, "C", C, 3)):
            ok, t, sg = edge(key, na)
            offer(ok, t, feature, sg, region, V)
        # an initial overlap comes first: the closest-segment block's pair value of the axis at rest
        Fv, sv, _, reg0, _, y = segment_ref.pair_value(np.broadcast_to(p32, shape), np.broadcast_to(q32, shape), np.broadcast_to(np.asarray(vert, F), shape),
                                                       np.broadcast_to(np.asarray(e1, F), shape), np.broadcast_to(np.asarray(e2, F), shape))
        overlap = Fv <= rr
        t = np.where(overlap, zero, held["t"])
        s = np.where(overlap, sv, held["s"])
        feature = np.where(overlap, np.uint8(0), held["feature"]).astype(np.uint8)
        region = np.where(overlap, reg0, held["region"]).astype(np.uint8)
        point = np.stack([np.where(overlap, y[..., k], held["point"][k]) for k in range(3)], axis=-1)
    return np.isfinite(t), t, s, feature, region, point


def valid_inputs(p, q, d, radius, tmax):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1) & np.isfinite(d).all(axis=1)
        ok &= (radius >= 0) & np.isfinite(radius) & (tmax >= 0) & np.isfinite(tmax)
    return ok


def shortlist(p, q, d, radius, tmax, prims, chunk_pairs=1 << 22):
    """(capsule index, triangle index) of every pair that can have a value, in row-major order.  At a contact (and at an initial
    overlap) a point of the moved axis is within r of a point of the triangle, so the box of the four ends p, q, p + tmax d,
    q + tmax d grown by r meets the triangle's corner box; the boxes are compared in binary64 with 1e-6 of the coordinates'
    magnitude to spare, far more than the value's own error."""
    vert, e1, e2 = records(prims)
    A, B, C = corners(vert, e1, e2)
    tlo, thi = np.minimum(np.minimum(A, B), C), np.maximum(np.maximum(A, B), C)
    p, q, d = p.astype(D), q.astype(D), d.astype(D)
    with np.errstate(all="ignore"):
        move = tmax.astype(D)[:, None] * d
        ends = np.stack([p, q, p + move, q + move])
        r = radius.astype(D)[:, None]
        clo, chi = ends.min(axis=0) - r, ends.max(axis=0) + r
        pad = 1e-6 * (np.abs(ends).max(axis=0) + r + 1.0)
    clo, chi = clo - pad, chi + pad
    rows, cols = [], []
    step = max(1, chunk_pairs // max(len(A), 1))
    for s in range(0, len(p), step):
        meet = ((clo[s:s + step, None, :] <= thi[None] + 1e-6 * np.abs(thi[None])) & (chi[s:s + step, None, :] >= tlo[None] - 1e-6 * np.abs(tlo[None]))).all(axis=2)
        i, j = np.nonzero(meet)
        rows.append(i + s)
        cols.append(j)
    return np.concatenate(rows), np.concatenate(cols)


def brute_values(p, q, d, radius, tmax, prims, chunk_pairs=1 << 17, cull=True):
    """(n capsules, m triangles) -> per capsule: the smallest t32, the lowest index that has it (-1: none), how many triangles have
    it.  cull: only the pairs of `shortlist` are evaluated (test_shortlist_keeps_every_winner compares the two)."""
    vert, e1, e2 = records(prims)
    n, m = p.shape[0], vert.shape[0]
    best, arg, ties = np.full(n, INF, F), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    if not n or not m:
        return best, arg, ties
    if cull:
        i, j = shortlist(p, q, d, radius, tmax, prims)
        t32 = np.empty(len(i), F)
        for s in range(0, len(i), chunk_pairs):
            ii, jj = i[s:s + chunk_pairs], j[s:s + chunk_pairs]
            hit, t = pair_value(p[ii], q[ii], d[ii], radius[ii], tmax[ii], vert[jj], e1[jj], e2[jj])[:2]
            t32[s:s + chunk_pairs] = np.where(hit, t, np.inf).astype(F)
        order = np.lexsort((j, t32, i))  # per capsule: by value, then by index
        i, j, t32 = i[order], j[order], t32[order]
        head = np.concatenate([[True], i[1:] != i[:-1]]) if len(i) else np.zeros(0, bool)
        found = t32[head] < INF
        cap = i[head][found]
        best[cap], arg[cap] = t32[head][found], j[head][found]
        np.add.at(ties, i, (t32 == best[i]) & (t32 < INF))
        return best, arg, ties
    step = max(1, chunk_pairs // max(n, 1))
    for s in range(0, m, step):
        hit, t = pair_value(p[:, None, :], q[:, None, :], d[:, None, :], radius[:, None], tmax[:, None], vert[None, s:s + step], e1[None, s:s + step], e2[None, s:s + step])[:2]
        t32 = np.where(hit, t, np.inf).astype(F)
        lo = t32.min(axis=1)
        first = t32.argmin(axis=1) + s  # argmin: the first of equal values
        cnt = (t32 == lo[:, None]).sum(axis=1)
        found = lo < INF
        better = found & (lo < best)  # an earlier chunk keeps a tie: the lowest index wins
        ties = np.where(better, cnt, np.where(found & (lo == best), ties + cnt, ties))
        arg = np.where(better, first, arg)
        best = np.where(better, lo, best)
    return best, arg, ties


def answers(p, q, d, r, tm, ok, arg, prims):
    """the eight outputs from the winners `arg` (-1: none) of capsules whose validity is `ok`"""
    n = p.shape[0]
    so, sd, st = np.where(ok[:, None], p, F(0)), np.where(ok[:, None], d, F(0)), np.where(ok, tm, F(0))
    with np.errstate(all="ignore"):
        end = (so.astype(D) + st.astype(D)[:, None] * sd.astype(D)).astype(F)
    t = np.where(ok, tm, INF).astype(F)
    prim = np.full(n, -1, np.int32)
    s = np.zeros(n, F)
    feature, region = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    center = np.where(ok[:, None], end, p).astype(F)
    point = center.copy()
    normal = np.zeros((n, 3), F)
    hit = ok & (arg >= 0)
    if hit.any():
        vert, e1, e2 = records(prims)
        w = arg[hit]
        h2, tv, sv, fe, re, pt = pair_value(p[hit], q[hit], d[hit], r[hit], tm[hit], vert[w], e1[w], e2[w])
        assert h2.all()
        pd, qd, dv = p[hit].astype(D), q[hit].astype(D), d[hit].astype(D)
        cen = (pd + sv[:, None] * (qd - pd)) + tv[:, None] * dv
        rad = r[hit].astype(D)[:, None]
        with np.errstate(all="ignore"):
            nrm = np.where(rad == 0, 0.0, (cen - pt) / rad)
        t[hit], prim[hit], s[hit], feature[hit], region[hit] = tv.astype(F), w.astype(np.int32), sv.astype(F), fe, re
        point[hit], center[hit], normal[hit] = pt.astype(F), cen.astype(F), nrm.astype(F)
    return t, prim, s, feature, region, point, center, normal


def inputs(p, q, d, radius, tmax):
    p, q, d = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (p, q, d))
    n = p.shape[0]
    r = np.broadcast_to(np.asarray(radius, F), (n,)).copy()
    tm = np.ones(n, F) if tmax is None else np.ascontiguousarray(tmax, F).reshape(n)
    return p, q, d, r, tm


def sweep_capsule(p, q, d, radius, prims, tmax=None, cull=True):
    """tyr_query_sweep_capsule's eight outputs: t (n), prim (n) int32, s (n), feature (n) uint8, region (n) uint8, point (n, 3),
    center (n, 3), normal (n, 3)"""
    p, q, d, r, tm = inputs(p, q, d, radius, tmax)
    ok = valid_inputs(p, q, d, r, tm)
    z3, z1 = ok[:, None], ok
    best, arg, _ = brute_values(np.where(z3, p, F(0)), np.where(z3, q, F(0)), np.where(z3, d, F(0)), np.where(z1, r, F(0)), np.where(z1, tm, F(0)), prims, cull=cull)
    out = answers(p, q, d, r, tm, ok, arg, prims)
    hit = ok & (arg >= 0)
    assert np.array_equal(out[0][hit].view(np.uint32), best[hit].view(np.uint32))
    return out


# ---- an independent truth for the definition -----------------------------------------------------------------------------
def truth(p, q, d, radius, tmax, vert, e1, e2, samples=1000, steps=60):
    """(t, clearance) per pair: the first parameter in [0, tmax] at which the moved axis is within radius of the triangle (+inf:
    never), from `samples` samples of the clearance -- segment_ref's pair distance of the moved axis minus radius -- along the
    path and `steps` bisections of the sign change in front of its minimum; and the path's least clearance.  The distance of two
    convex sets of which one moves along a straight line is convex in t, so the minimum lies next to the least sample."""
    p, q, d = (np.asarray(x, F).astype(D) for x in (p, q, d))
    radius, tmax = np.asarray(radius, F).astype(D), np.asarray(tmax, F).astype(D)
    n = p.shape[0]
    A, B, C = corners(vert, e1, e2)

    def f(t):
        move = t[:, None] * d
        return _axis_distance(p + move, q + move, A, B, C) - radius

    start = f(np.zeros(n, D))
    least, at = start.copy(), np.zeros(n, np.int64)
    for k in range(1, samples + 1):
        cur = f(tmax * (k / samples))
        at = np.where(cur < least, k, at)
        least = np.minimum(least, cur)
    lo, hi = tmax * (np.maximum(at - 1, 0) / samples), tmax * (np.minimum(at + 1, samples) / samples)
    for _ in range(100):
        m1, m2 = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
        left = f(m1) <= f(m2)
        hi = np.where(left, m2, hi)
        lo = np.where(left, lo, m1)
    tmin = 0.5 * (lo + hi)
    low = f(tmin)
    tmin = np.where(low <= least, tmin, tmax * (at / samples))
    least = np.minimum(least, low)
    lo, hi = np.zeros(n, D), tmin.copy()
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        inside = f(mid) <= 0
        hi = np.where(inside, mid, hi)
        lo = np.where(inside, lo, mid)
    t = np.where(start <= 0, 0.0, np.where(least <= 0, hi, np.inf))
    return t, least


def _axis_distance(P0, P1, A, B, C):
    """distance of segments P0 -> P1 to triangles (A, B, C), all binary64 (n, 3): segment_ref's pair value on binary64 corners --
    its six candidates, written here with numpy's own dot and cross so that it shares no code with the restatement"""
    def seg_seg(p0, p1, q0, q1):
        d1, d2, r = p1 - p0, q1 - q0, p0 - q0
        a, e, f = (d1 * d1).sum(-1), (d2 * d2).sum(-1), (d2 * r).sum(-1)
        c, b = (d1 * r).sum(-1), (d1 * d2).sum(-1)
        den = a * e - b * b
        a1, e1 = np.where(a > 0, a, 1.0), np.where(e > 0, e, 1.0)
        s = np.where(den > 0, np.clip((b * f - c * e) / np.where(den > 0, den, 1.0), 0, 1), 0.0)
        s = np.where(a > 0, s, 0.0)
        t = np.where(e > 0, np.clip((b * s + f) / e1, 0, 1), 0.0)
        s = np.where(a > 0, np.clip((b * t - c) / a1, 0, 1), 0.0)
        w = (p0 + s[:, None] * d1) - (q0 + t[:, None] * d2)
        return (w * w).sum(-1)

    from sweep_ref import true_dist

    best = np.minimum(true_dist(P0, A, B, C), true_dist(P1, A, B, C)) ** 2
    for q0, q1 in ((A, B), (A, C), (B, C)):
        best = np.minimum(best, seg_seg(P0, P1, q0, q1))
    # a crossing: Moeller-Trumbore
    E1, E2, dv = B - A, C - A, P1 - P0
    with np.errstate(all="ignore"):
        pv = np.cross(dv, E2)
        det = (E1 * pv).sum(-1)
        tv = P0 - A
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, E1)
        v = (dv * qv).sum(-1) / det
        t = (E2 * qv).sum(-1) / det
        cross = np.isfinite(t) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)
    return np.sqrt(np.where(cross, 0.0, best))


# ---- the pruning key ---------------------------------------------------------------------------------------------------
def recip32(d):
    """hip/sweep.hip's sweep_recip: 1 / d_k, +-inf for a zero, a NaN where the reciprocal is no normal number"""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)
    normal = (np.abs(inv) >= F(2.0 ** -126)) & (np.abs(inv) < INF)
    return np.where((d == 0) | normal, inv, F(np.nan)).astype(F)


def key32(p, q, d, r, best, lo, hi, slack):
    """hip/sweep_capsule.hip's capsule_key in numpy binary32, operation by operation, for capsules (n, 3) and boxes lo, hi (n, 3):
    (near, far, visited)"""
    p, q, d, lo, hi = (np.asarray(x, F) for x in (p, q, d, lo, hi))
    r, best = np.asarray(r, F), np.asarray(best, F)
    inv = recip32(d)
    with np.errstate(all="ignore"):
        a = (q - p).astype(F)
        gl = (r[:, None] + np.maximum(a, F(0))).astype(F)
        gh = (r[:, None] + np.maximum(-a, F(0))).astype(F)
        lo1, hi1 = (lo - gl).astype(F), (hi + gh).astype(F)
        e = (F(slack) * (np.abs(p) + np.maximum(np.abs(lo1), np.abs(hi1))).astype(F)).astype(F)
        t1 = (((lo1 - e).astype(F) - p).astype(F) * inv).astype(F)
        t2 = (((hi1 + e).astype(F) - p).astype(F) * inv).astype(F)
        nan = np.isnan(t1) | np.isnan(t2)
        near = np.where(nan, -np.inf, np.fmin(t1, t2)).astype(F).max(axis=1)
        far = np.where(nan, np.inf, np.fmax(t1, t2)).astype(F).min(axis=1)
    return near, far, (near <= far) & (far >= 0) & (near <= best)
