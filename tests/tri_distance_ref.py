"""numpy restatement of tyr_query_tri_distance (include/tyr_c.h "Closest-triangle queries"): the reference the GPU tests compare
against bit for bit.  Every operation is one binary64 operation in the specified order, with segment_ref's dot, cross, - and
clamp01 and sweep_ref's closest-point rule; inputs are binary32 widened exactly.  The pair value is the least of 21 candidates:
where a candidate is the segment block's with the query's edge as the segment, the operations are segment_ref's, written here on
the shared operands; where the roles are exchanged (codes 3-5 and 9-11) they are written anew.  The query is an argmin over all
triangles with no traversal order in it, so brute force over the uploaded array -- over the pairs a triangle-inequality shortlist
keeps -- is the whole oracle.  `truth` is an independent check of the definition: a nested ternary search over the query's
barycentrics of the binary64 point-to-triangle distance, which is convex.  `key32` is hip/tri_distance.hip's pruning key in numpy
binary32, operation by operation."""
import numpy as np

import nearest_ref
import tri_ref
from segment_ref import _clamp01, bound2  # noqa: F401  (bound2: for the callers)
from sweep_ref import _closest, _cross, _dot, _sub, corners, records, true_dist  # noqa: F401  (the shared definitions)

F = np.float32
D = np.float64
INF = F(np.inf)
NAMES = ("dist2", "prim", "feature", "region", "on_query", "on_triangle")


def _crossing(n, nn, T0, t1, t2, h0, h1, S0, d):
    """the segment block's feature 0 of the segment S0 + s d against the triangle (T0, t1, t2) with normal n: (ok, x);
    h0 = dot(n, S0 - T0) and h1 = dot(n, S1 - T0) are the caller's"""
    s = h0 / (h0 - h1)
    x = [S0[k] + s * d[k] for k in range(3)]
    w = _sub(x, T0)
    bv, bw = _dot(_cross(w, t2), n), _dot(_cross(t1, w), n)
    sides = ((h0 <= 0) & (h1 >= 0)) | ((h0 >= 0) & (h1 <= 0))
    return (nn > 0) & (h0 != h1) & sides & (bv >= 0) & (bw >= 0) & ((bv + bw) <= nn), x


def _edge_pair(S0, d, a, Q0, e, r, code, code0, code1):
    """the segment block's edge rule of the segment S0 + s d (a = dot(d, d)) against the edge Q0 + t e, r = S0 - Q0: (F, region, x, y)"""
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
    x = [S0[k] + s * d[k] for k in range(3)]
    y = [Q0[k] + e[k] * t for k in range(3)]
    xy = _sub(x, y)
    region = np.where((t > 0) & (t < 1), code, np.where(t >= 1, code1, code0)).astype(np.uint8)
    return _dot(xy, xy), region, x, y


def pair_value(a, b, c, vert, e1, e2):
    """(F, feature, region, x, y) of query triangles (a, b, c) against scene triangles (vert, e1, e2), all of shape (..., 3) that
    broadcast against each other: F binary64, feature (the candidate code 0..20) and region uint8, x (on the query) and y (on the
    scene triangle) (..., 3) binary64"""
    A, B, C = corners(vert, e1, e2)
    P = [np.asarray(x, F).astype(D) for x in (a, b, c)]
    shape = np.broadcast_shapes(*(x.shape for x in P), A.shape)
    P0, P1, P2, A, B, C = (list(np.moveaxis(np.broadcast_to(x, shape), -1, 0)) for x in (*P, A, B, C))
    sh = shape[:-1]
    with np.errstate(all="ignore"):
        held = {"F": np.full(sh, np.inf, D), "feature": np.zeros(sh, np.uint8), "region": np.zeros(sh, np.uint8),
                "x": [np.zeros(sh, D) for _ in range(3)], "y": [np.zeros(sh, D) for _ in range(3)]}

        def offer(ok, Fv, feature, region, x, y):
            win = ok & (Fv < held["F"])  # strict: of equal F the lower code stays
            held["F"] = np.where(win, Fv, held["F"])
            held["feature"] = np.where(win, np.uint8(feature), held["feature"])
            held["region"] = np.where(win, region, held["region"]).astype(np.uint8)
            held["x"] = [np.where(win, x[k], held["x"][k]) for k in range(3)]
            held["y"] = [np.where(win, y[k], held["y"][k]) for k in range(3)]

        zero, yes = np.zeros(sh, D), np.ones(sh, bool)
        Pq = [P0, P1, P2]
        e1, e2, e3 = _sub(B, A), _sub(C, A), _sub(C, B)  # the scene triangle's edge vectors G0, G1, G2
        u1, u2 = _sub(P1, P0), _sub(P2, P0)  # the query as a triangle (P0, u1, u2)
        dq = [u1, _sub(P2, P1), _sub(P0, P2)]  # the query's edges E0, E1, E2 as segments
        n, m = _cross(e1, e2), _cross(u1, u2)
        nn, mm = _dot(n, n), _dot(m, m)
        ap = [_sub(Pj, A) for Pj in Pq]  # query corners relative to A
        vp = [_sub(V, P0) for V in (A, B, C)]  # scene corners relative to P0
        # codes 0-2: a query edge crosses the scene triangle
        hn = [_dot(n, x) for x in ap]
        for j in range(3):
            ok, x = _crossing(n, nn, A, e1, e2, hn[j], hn[(j + 1) % 3], Pq[j], dq[j])
            offer(ok, zero, j, np.uint8(0), x, x)
        # codes 3-5: a scene edge crosses the query triangle
        hm = [_dot(m, x) for x in vp]
        for j, (i0, i1, S0, d) in enumerate(((0, 1, A, e1), (0, 2, A, e2), (1, 2, B, e3))):
            ok, x = _crossing(m, mm, P0, u1, u2, hm[i0], hm[i1], S0, d)
            offer(ok, zero, 3 + j, np.uint8(4 + j), x, x)
        # codes 6-8: a query corner against the scene triangle
        for j in range(3):
            Fv, region, y = _closest(ap[j], e1, e2, A)
            offer(yes, Fv, 6 + j, region, Pq[j], y)
        # codes 9-11: a scene corner against the query triangle
        for j, V in enumerate((A, B, C)):
            Fv, _, x = _closest(vp[j], u1, u2, P0)
            offer(yes, Fv, 9 + j, np.uint8(1 + j), x, V)
        # codes 12-20: the edge pairs
        bp = [_sub(Pj, B) for Pj in Pq]
        for i in range(3):
            aa = _dot(dq[i], dq[i])
            for j, (Q0, e, r, codes) in enumerate(((A, e1, ap[i], (4, 1, 2)), (A, e2, ap[i], (5, 1, 3)), (B, e3, bp[i], (6, 2, 3)))):
                Fv, region, x, y = _edge_pair(Pq[i], dq[i], aa, Q0, e, r, *codes)
                offer(yes, Fv, 12 + 3 * i + j, region, x, y)
    return held["F"], held["feature"], held["region"], np.stack(held["x"], axis=-1), np.stack(held["y"], axis=-1)


def valid_inputs(a, b, c, max_dist):
    with np.errstate(invalid="ignore"):
        return tri_ref.valid_queries(a, b, c) & (max_dist >= 0)


def shared_corner(a, b, c, vert, e1, e2):
    """rule 0 of "Triangle-overlap queries" for arrays (..., 3) that broadcast: some query corner equals some scene corner"""
    P = [np.moveaxis(np.asarray(x, F).astype(D), -1, 0) for x in (a, b, c)]
    Q = [np.moveaxis(x, -1, 0) for x in corners(vert, e1, e2)]
    return tri_ref._shared(P, Q)


def shortlist(a, b, c, prims, chunk_pairs=1 << 20):
    """(query index, triangle index) of every pair that can hold the least F32 of its query, in row-major order.  With dA the
    distance of the scene corner A to the query triangle and R the longer of the scene triangle's edges from A, the triangle
    inequality gives (dA - R)^2 <= F <= dA^2; a triangle whose lower bound lies more than 1e-6 (sixteen binary32 steps) above the
    least upper bound of its query has a larger F32 than that triangle and is neither the winner nor tied with it.  Pairs that
    share a corner are kept out of the least upper bound (skip_shared may remove them) but stay on the list."""
    vert, e1, e2 = records(prims)
    A, B, C = corners(vert, e1, e2)
    R = np.sqrt(np.maximum(((B - A) ** 2).sum(-1), ((C - A) ** 2).sum(-1)))
    P0, P1, P2 = (x.astype(D) for x in (a, b, c))
    rows, cols = [], []
    step = max(1, chunk_pairs // max(len(A), 1))
    for s in range(0, len(P0), step):
        t = slice(s, s + step)
        dA = true_dist(A[None, :, :], P0[t, None, :], P1[t, None, :], P2[t, None, :])
        lower = np.maximum(dA - R[None, :], 0.0) ** 2
        sh = shared_corner(a[t, None, :], b[t, None, :], c[t, None, :], vert[None], e1[None], e2[None])
        least = np.where(sh, np.inf, dA ** 2).min(axis=1, keepdims=True)
        i, j = np.nonzero(lower <= least * (1 + 1e-6) + 1e-30)
        rows.append(i + s)
        cols.append(j)
    return np.concatenate(rows), np.concatenate(cols)


def brute_values(a, b, c, b2, prims, skip_shared=False, chunk_pairs=1 << 17, cull=True):
    """(n queries, m triangles) -> per query: the smallest F32 below b2, the lowest index that has it (-1: none), how many
    triangles have it.  cull: only the pairs of `shortlist` are evaluated (test_shortlist_keeps_every_winner compares the two)."""
    vert, e1, e2 = records(prims)
    n, m = a.shape[0], vert.shape[0]
    best, arg, ties = np.full(n, INF, F), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    if cull and n and m:
        i, j = shortlist(a, b, c, prims)
        Fv = np.concatenate([pair_value(a[i[s:s + chunk_pairs]], b[i[s:s + chunk_pairs]], c[i[s:s + chunk_pairs]], vert[j[s:s + chunk_pairs]],
                                        e1[j[s:s + chunk_pairs]], e2[j[s:s + chunk_pairs]])[0] for s in range(0, len(i), chunk_pairs)])
        with np.errstate(over="ignore"):
            F32 = Fv.astype(F)
        F32 = np.where(F32 < b2[i], F32, INF)
        if skip_shared:
            F32 = np.where(shared_corner(a[i], b[i], c[i], vert[j], e1[j], e2[j]), INF, F32)
        order = np.lexsort((j, F32, i))  # per query: by value, then by index
        i, j, F32 = i[order], j[order], F32[order]
        head = np.concatenate([[True], i[1:] != i[:-1]])
        found = F32[head] < INF
        q = i[head][found]
        best[q], arg[q] = F32[head][found], j[head][found]
        np.add.at(ties, i, (F32 == best[i]) & (F32 < INF))
        return best, arg, ties
    step = max(1, chunk_pairs // max(n, 1))
    for s in range(0, m, step):
        t = slice(s, s + step)
        Fv = pair_value(a[:, None, :], b[:, None, :], c[:, None, :], vert[None, t], e1[None, t], e2[None, t])[0]
        with np.errstate(over="ignore"):
            F32 = Fv.astype(F)
        F32 = np.where(F32 < b2[:, None], F32, INF)
        if skip_shared:
            F32 = np.where(shared_corner(a[:, None, :], b[:, None, :], c[:, None, :], vert[None, t], e1[None, t], e2[None, t]), INF, F32)
        lo = F32.min(axis=1)
        first = F32.argmin(axis=1) + s  # argmin: the first of equal values
        cnt = (F32 == lo[:, None]).sum(axis=1)
        found = lo < INF
        better = found & (lo < best)  # an earlier chunk keeps a tie: the lowest index wins
        ties = np.where(better, cnt, np.where(found & (lo == best), ties + cnt, ties))
        arg = np.where(better, first, arg)
        best = np.where(better, lo, best)
    return best, arg, ties


def answers(a, b, c, b2, ok, arg, prims):
    """the six outputs from the winners `arg` (-1: none) of queries whose validity is `ok` and bound is b2"""
    n = a.shape[0]
    dist2 = np.where(ok, b2, INF).astype(F)
    prim = np.full(n, -1, np.int32)
    feature, region = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    on_query, on_triangle = a.copy(), a.copy()
    hit = ok & (arg >= 0)
    if hit.any():
        vert, e1, e2 = records(prims)
        w = arg[hit]
        Fv, fe, re, x, y = pair_value(a[hit], b[hit], c[hit], vert[w], e1[w], e2[w])
        dist2[hit], prim[hit], feature[hit], region[hit] = Fv.astype(F), w.astype(np.int32), fe, re
        on_query[hit], on_triangle[hit] = x.astype(F), y.astype(F)
    return dist2, prim, feature, region, on_query, on_triangle


def tri_distance(a, b, c, prims, max_dist=None, skip_shared=False, cull=True):
    """tyr_query_tri_distance's six outputs: dist2 (n), prim (n) int32, feature (n) uint8, region (n) uint8, on_query (n, 3),
    on_triangle (n, 3)"""
    a, b, c = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (a, b, c))
    n = a.shape[0]
    md = np.full(n, INF, F) if max_dist is None else np.broadcast_to(np.asarray(max_dist, F), (n,))
    ok = valid_inputs(a, b, c, md)
    b2 = bound2(max_dist, n)
    sa, sb, sc = (np.where(ok[:, None], x, F(0)) for x in (a, b, c))
    if len(prims):
        best, arg, _ = brute_values(sa, sb, sc, np.where(ok, b2, F(0)), prims, skip_shared, cull=cull)
    else:
        best, arg = np.full(n, INF, F), np.full(n, -1, np.int64)
    out = answers(a, b, c, b2, ok, arg, prims)
    hit = ok & (arg >= 0)
    assert np.array_equal(out[0][hit].view(np.uint32), best[hit].view(np.uint32))
    return out


# ---- an independent truth for the definition -----------------------------------------------------------------------------
def truth(a, b, c, vert, e1, e2, steps=80):
    """the least distance between the query triangle and the scene triangle per pair, in binary64: a nested ternary search over
    the query's barycentrics (u in [0, 1] outside, v in [0, 1 - u] inside) of nearest_ref.true_dist2 -- the squared distance to
    a convex set is convex along the query, and so is its minimum over v as a function of u.  Pairs that touch are the
    caller's to set to 0 (tri_ref.pair_exact)."""
    A, B, C = corners(vert, e1, e2)
    P0, P1, P2 = (np.asarray(x, F).astype(D) for x in (a, b, c))
    E1, E2 = B - A, C - A
    n = P0.shape[0]

    def inner(u, P0, U1, U2, A, E1, E2):  # min over v of the squared distance at u
        def f(v):
            return nearest_ref.true_dist2(P0 + u[:, None] * U1 + v[:, None] * U2, A, E1, E2)

        lo, hi = np.zeros_like(u), 1.0 - u
        for _ in range(steps):
            m1, m2 = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
            left = f(m1) <= f(m2)
            hi = np.where(left, m2, hi)
            lo = np.where(left, lo, m1)
        return np.minimum(np.minimum(f(np.zeros_like(u)), f(1.0 - u)), f(0.5 * (lo + hi)))

    two = lambda x: np.concatenate([x, x])  # noqa: E731  (both probes of the outer search in one batch)
    args2 = tuple(two(x) for x in (P0, P1 - P0, P2 - P0, A, E1, E2))
    args1 = (P0, P1 - P0, P2 - P0, A, E1, E2)
    lo, hi = np.zeros(n, D), np.ones(n, D)
    for _ in range(steps):
        m1, m2 = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
        g = inner(np.concatenate([m1, m2]), *args2)
        left = g[:n] <= g[n:]
        hi = np.where(left, m2, hi)
        lo = np.where(left, lo, m1)
    best = np.minimum(np.minimum(inner(np.zeros(n, D), *args1), inner(np.ones(n, D), *args1)), inner(0.5 * (lo + hi), *args1))
    return np.sqrt(best)


def touching(a, b, c, vert, e1, e2):
    """per pair whether tri_ref.pair_exact (exact integer arithmetic) calls the two triangles touching"""
    return np.array([tri_ref.pair_exact(a[i], b[i], c[i], vert[i], e1[i], e2[i]) == 0 for i in range(len(a))], bool)


# ---- the pruning key ---------------------------------------------------------------------------------------------------
def key32(a, b, c, lo, hi, slack, floor):
    """hip/tri_distance.hip's tri_distance_key in numpy binary32, operation by operation, for query triangles (n, 3) each and
    boxes lo, hi (n, 3): (key, D, E) -- the squared reduced bound, the distance bound before the reduction, and the reduction"""
    a, b, c, lo, hi = (np.asarray(x, F) for x in (a, b, c, lo, hi))
    with np.errstate(all="ignore"):
        qlo, qhi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        m3 = np.maximum(np.abs(qlo), np.abs(qhi))
        ms = ((m3[:, 0] + m3[:, 1]).astype(F) + m3[:, 2]).astype(F)
        g = np.fmax(F(0), np.fmax((lo - qhi).astype(F), (qlo - hi).astype(F))).astype(F)
        Dv = np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(F) + g[:, 2] * g[:, 2]).astype(F)).astype(F)
        b3 = np.maximum(np.abs(lo), np.abs(hi))
        M = (ms + ((b3[:, 0] + b3[:, 1]).astype(F) + b3[:, 2]).astype(F)).astype(F)
        E = ((F(slack) * M).astype(F) + F(floor)).astype(F)
        l0 = (Dv - E).astype(F)
        lb = np.where(l0 > 0, l0, F(0)).astype(F)
        key = (lb * lb).astype(F)
    return key, Dv, E
