"""numpy restatement of tyr_query_sweep (include/tyr_c.h "Swept-sphere queries"): the reference the GPU tests compare against
bit for bit.  Every operation is one binary64 operation in the specified order, dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z,
cross as the winding block's, divisions and square roots correctly rounded; inputs are binary32 widened exactly.  The query
is an argmin over all triangles with no traversal order in it, so brute force over the uploaded array, in chunks, is the whole
oracle.  `truth` is an independent check of the definition itself: the distance to the triangle sampled along the path and
bisected."""
import numpy as np

F = np.float32
D = np.float64
INF = F(np.inf)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def corners(vert, e1, e2):
    """A = vert, B = the binary32 sum vert + e1, C = the binary32 sum vert + e2, widened: the corners tyr_triangle_bboxes bounds"""
    vert, e1, e2 = (np.asarray(a, F) for a in (vert, e1, e2))
    with np.errstate(all="ignore"):
        return vert.astype(D), (vert + e1).astype(F).astype(D), (vert + e2).astype(F).astype(D)


def _closest(ap, e1, e2, A):
    """Ericson's closest-point test and clamp ("Closest-point queries") in binary64: (F, region, c)"""
    bp, cp = _sub(ap, e1), _sub(ap, e2)
    d1, d2 = _dot(e1, ap), _dot(e2, ap)
    d3, d4 = _dot(e1, bp), _dot(e2, bp)
    d5, d6 = _dot(e1, cp), _dot(e2, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    g = d4 - d3
    h = d5 - d6
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    w = g / (g + h)
    den = one / ((va + vb) + vc)
    rules = [
        ((d1 <= 0) & (d2 <= 0), 1, zero, zero),
        ((d3 >= 0) & (d4 <= d3), 2, one, zero),
        ((vc <= 0) & (d1 >= 0) & (d3 <= 0), 4, d1 / (d1 - d3), zero),
        ((d6 >= 0) & (d5 <= d6), 3, zero, one),
        ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 5, zero, d2 / (d2 - d6)),
        ((va <= 0) & (g >= 0) & (h >= 0), 6, one - w, w),
    ]
    region = np.zeros(d1.shape, np.uint8)
    u, v = vb * den, vc * den
    for cond, code, ru, rv in reversed(rules):  # the first rule that holds wins: applied last
        region = np.where(cond, np.uint8(code), region)
        u = np.where(cond, ru, u)
        v = np.where(cond, rv, v)
    u1 = np.where(u > 0, u, zero)
    u2 = np.where(u1 < 1, u1, one)
    r = one - u2
    v1 = np.where(v > 0, v, zero)
    v2 = np.where(v1 < r, v1, r)
    q = [(ap[k] - e1[k] * u2) - e2[k] * v2 for k in range(3)]
    c = [(A[k] + e1[k] * u2) + e2[k] * v2 for k in range(3)]
    return _dot(q, q), region, c


def pair_value(o, d, radius, tmax, vert, e1, e2):
    """(hit, t, region, contact) of sweeps (o, d, radius, tmax) against triangles (vert, e1, e2): o, d, vert, e1, e2 of shape
    (..., 3) and radius, tmax of shape (...) that broadcast against each other.  t is binary64 (+inf where the pair has no
    value), contact (..., 3) binary64."""
    A, B, C = corners(vert, e1, e2)
    o, d = np.asarray(o, F).astype(D), np.asarray(d, F).astype(D)
    radius, tmax = np.asarray(radius, F).astype(D), np.asarray(tmax, F).astype(D)
    shape = np.broadcast_shapes(o.shape, d.shape, A.shape, radius.shape + (3,), tmax.shape + (3,))
    o, d, A, B, C = (np.moveaxis(np.broadcast_to(a, shape), -1, 0) for a in (o, d, A, B, C))
    radius, tmax = np.broadcast_to(radius, shape[:-1]), np.broadcast_to(tmax, shape[:-1])
    with np.errstate(all="ignore"):
        e1, e2 = _sub(B, A), _sub(C, A)
        ap = _sub(o, A)
        rr = radius * radius
        dist2, reg0, c0 = _closest(ap, e1, e2, A)
        overlap = dist2 <= rr
        dd = _dot(d, d)
        best = np.full(shape[:-1], np.inf, D)
        region = np.zeros(shape[:-1], np.uint8)
        contact = [np.zeros(shape[:-1], D) for _ in range(3)]

        def offer(ok, t, code, point):
            nonlocal best, region, contact
            win = ok & (t >= 0) & (t <= tmax) & (t < best)  # strict: of equal t the lower region code stays
            best = np.where(win, t, best)
            region = np.where(win, np.uint8(code), region)
            contact = [np.where(win, point[k], contact[k]) for k in range(3)]

        # the face
        n = _cross(e1, e2)
        nn = _dot(n, n)
        ln = np.sqrt(nn)
        h = _dot(n, ap)
        s = np.where(h >= 0, 1.0, -1.0)
        sdn = s * _dot(n, d)
        ah = np.abs(h)
        rl = radius * ln
        t = (ah - rl) / (-sdn)
        k = (s * radius) / ln
        q = [(o[i] + t * d[i]) - n[i] * k for i in range(3)]
        w = _sub(q, A)
        bv, bw = _dot(_cross(w, e2), n), _dot(_cross(e1, w), n)
        offer((nn > 0) & (sdn < 0) & (ah > rl) & (bv >= 0) & (bw >= 0) & ((bv + bw) <= nn), t, 0, q)
        # the vertices
        for code, P in ((1, A), (2, B), (3, C)):
            m = _sub(o, P)
            b = _dot(m, d)
            c = _dot(m, m) - rr
            disc = b * b - dd * c
            t = (-b - np.sqrt(disc)) / dd
            offer((dd > 0) & (b < 0) & (c > 0) & (disc >= 0), t, code, P)
        # the edges
        for code, P0, P1 in ((4, A, B), (5, A, C), (6, B, C)):
            e = _sub(P1, P0)
            m = _sub(o, P0)
            ee, de, me = _dot(e, e), _dot(d, e), _dot(m, e)
            md, mm = _dot(m, d), _dot(m, m)
            a = ee * dd - de * de
            b = ee * md - de * me
            c = ee * (mm - rr) - me * me
            disc = b * b - a * c
            t = (-b - np.sqrt(disc)) / a
            sg = (me + t * de) / ee
            offer((ee > 0) & (a > 0) & (b < 0) & (c > 0) & (disc >= 0) & (sg >= 0) & (sg <= 1), t, code, [P0[i] + e[i] * sg for i in range(3)])
        # an initial overlap comes first
        zero = np.zeros(shape[:-1], D)
        best = np.where(overlap, zero, best)
        region = np.where(overlap, reg0, region)
        contact = [np.where(overlap, c0[k], contact[k]) for k in range(3)]
    return np.isfinite(best), best, region, np.stack(contact, axis=-1)


def records(prims):
    """(vert, e1, e2) of a TRIANGLE_DTYPE array as float32 (n, 3) arrays"""
    return (np.ascontiguousarray(prims[k], F).reshape(-1, 3) for k in ("vert", "e1", "e2"))


def valid_inputs(origins, directions, radius, tmax):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(origins).all(axis=1) & np.isfinite(directions).all(axis=1)
        ok &= (radius >= 0) & np.isfinite(radius) & (tmax >= 0) & np.isfinite(tmax)
    return ok


def brute_values(o, d, radius, tmax, prims, chunk_pairs=1 << 18):
    """(n sweeps, m triangles) -> per sweep: the smallest t32, the lowest index that has it (-1: none), how many triangles have it"""
    vert, e1, e2 = records(prims)
    n, m = o.shape[0], vert.shape[0]
    best = np.full(n, INF, F)
    arg = np.full(n, -1, np.int64)
    ties = np.zeros(n, np.int64)
    step = max(1, chunk_pairs // max(n, 1))
    for s in range(0, m, step):
        hit, t, _, _ = pair_value(o[:, None, :], d[:, None, :], radius[:, None], tmax[:, None], vert[None, s:s + step], e1[None, s:s + step], e2[None, s:s + step])
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


def sweep(origins, directions, radius, prims, tmax=None, chunk_pairs=1 << 18):
    """tyr_query_sweep's six outputs: t (n), prim (n) int32, region (n) uint8, point (n, 3), center (n, 3), normal (n, 3)"""
    o = np.ascontiguousarray(origins, F).reshape(-1, 3)
    d = np.ascontiguousarray(directions, F).reshape(-1, 3)
    n = o.shape[0]
    r = np.broadcast_to(np.asarray(radius, F), (n,)).copy()
    tm = np.ones(n, F) if tmax is None else np.ascontiguousarray(tmax, F).reshape(n)
    ok = valid_inputs(o, d, r, tm)
    so, sd = np.where(ok[:, None], o, F(0)), np.where(ok[:, None], d, F(0))
    sr, st = np.where(ok, r, F(0)), np.where(ok, tm, F(0))
    best, arg, _ = brute_values(so, sd, sr, st, prims, chunk_pairs) if len(prims) else (np.full(n, INF, F), np.full(n, -1, np.int64), None)
    hit = ok & (arg >= 0)
    with np.errstate(all="ignore"):
        end = (so.astype(D) + st.astype(D)[:, None] * sd.astype(D)).astype(F)
    t = np.where(ok, tm, INF).astype(F)
    prim = np.full(n, -1, np.int32)
    region = np.zeros(n, np.uint8)
    center = np.where(ok[:, None], end, o).astype(F)
    point = center.copy()
    normal = np.zeros((n, 3), F)
    if hit.any():
        vert, e1, e2 = records(prims)
        w = arg[hit]
        h2, tv, reg, c = pair_value(o[hit], d[hit], r[hit], tm[hit], vert[w], e1[w], e2[w])
        assert h2.all() and np.array_equal(tv.astype(F).view(np.uint32), best[hit].view(np.uint32))
        cen = o[hit].astype(D) + tv[:, None] * d[hit].astype(D)
        rad = r[hit].astype(D)[:, None]
        with np.errstate(all="ignore"):
            nrm = np.where(rad == 0, 0.0, (cen - c) / rad)
        t[hit], prim[hit], region[hit] = tv.astype(F), w.astype(np.int32), reg
        point[hit], center[hit], normal[hit] = c.astype(F), cen.astype(F), nrm.astype(F)
    return t, prim, region, point, center, normal


# ---- an independent truth for the definition -----------------------------------------------------------------------------
def true_dist(p, A, B, C):
    """distance of points p (..., 3) to the triangles (A, B, C) in binary64: the minimum over the three edges and, where the
    projection falls inside, the plane"""
    def seg(a, b):
        e = b - a
        ee = (e * e).sum(-1)
        t = np.clip(np.where(ee > 0, ((p - a) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0), 0.0, 1.0)
        q = p - (a + t[..., None] * e)
        return (q * q).sum(-1)

    edges = np.minimum(np.minimum(seg(A, B), seg(A, C)), seg(B, C))
    e1, e2 = B - A, C - A
    n = np.cross(e1, e2)
    nn = (n * n).sum(-1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    ap = p - A
    u = (np.cross(ap, e2) * n).sum(-1) / nn1
    v = (np.cross(e1, ap) * n).sum(-1) / nn1
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    plane = ((ap * n).sum(-1)) ** 2 / nn1
    return np.sqrt(np.where(inside, np.minimum(plane, edges), edges))


def truth(o, d, radius, tmax, vert, e1, e2, samples=4000, steps=60):
    """(t, clearance) per pair: the first parameter in [0, tmax] at which the centre is within radius of the triangle (+inf:
    never), from `samples` samples of the distance along the path and `steps` bisections of the sign change in front of its
    minimum; and the path's least distance minus radius"""
    A, B, C = corners(vert, e1, e2)
    o, d = np.asarray(o, F).astype(D), np.asarray(d, F).astype(D)
    radius, tmax = np.asarray(radius, F).astype(D), np.asarray(tmax, F).astype(D)
    n = o.shape[0]

    def f(t):
        return true_dist(o + t[:, None] * d, A, B, C) - radius

    start = f(np.zeros(n, D))
    least, at = start.copy(), np.zeros(n, np.int64)
    for k in range(1, samples + 1):
        cur = f(tmax * (k / samples))
        at = np.where(cur < least, k, at)
        least = np.minimum(least, cur)
    # the distance to a convex set along a straight path is convex in t: its minimum lies next to the least sample, and the
    # clearance changes sign once in front of it.  The minimum by ternary search, so that a contact shorter than a step counts
    a, b = tmax * (np.maximum(at - 1, 0) / samples), tmax * (np.minimum(at + 1, samples) / samples)
    for _ in range(100):
        m1, m2 = a + (b - a) / 3.0, b - (b - a) / 3.0
        left = f(m1) <= f(m2)
        b = np.where(left, m2, b)
        a = np.where(left, a, m1)
    tmin = 0.5 * (a + b)
    low = f(tmin)
    tmin = np.where(low <= least, tmin, tmax * (at / samples))
    least = np.minimum(least, low)
    a, b = np.zeros(n, D), tmin.copy()
    for _ in range(steps):
        mid = 0.5 * (a + b)
        inside = f(mid) <= 0
        b = np.where(inside, mid, b)
        a = np.where(inside, a, mid)
    t = np.where(start <= 0, 0.0, np.where(least <= 0, b, np.inf))
    return t, least


def truth_point(o, d, tmax, vert, e1, e2):
    """(t, margin) per pair for a swept point (radius 0): where the segment crosses the triangle's plane inside the triangle
    (+inf: nowhere), in binary64; margin is the least barycentric coordinate of the crossing -- near 0 the segment grazes an edge"""
    A, B, C = corners(vert, e1, e2)
    o, d, tmax = np.asarray(o, F).astype(D), np.asarray(d, F).astype(D), np.asarray(tmax, F).astype(D)
    n = np.cross(B - A, C - A)
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        t = ((A - o) * n).sum(-1) / (n * d).sum(-1)
        w = o + t[:, None] * d - A
        u = (np.cross(w, C - A) * n).sum(-1) / nn
        v = (np.cross(B - A, w) * n).sum(-1) / nn
        margin = np.minimum(np.minimum(u, v), 1.0 - (u + v))
        inside = np.isfinite(t) & (t >= 0) & (t <= tmax) & (margin >= 0)
    return np.where(inside, t, np.inf), np.where(np.isfinite(margin), margin, 1.0)
