"""numpy float32 restatement of tyr_query_nearest (include/tyr_c.h "Closest-point queries"): the reference the GPU tests compare
against bit for bit.  Every operation is one binary32 operation in the specified order, dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z,
divisions correctly rounded.  The query is an argmin over all triangles with no traversal order in it, so brute force over
the uploaded array, in chunks, is the whole oracle."""
import numpy as np

F = np.float32
INF = F(np.inf)


def _dot(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]).astype(F)


def pair_value(p, vert, e1, e2):
    """(F, u2, v2, region, c) of points p against triangles (vert, e1, e2): arrays of shape (..., 3) that broadcast against
    each other.  Returns arrays of the broadcast shape (c: (..., 3))."""
    p, vert, e1, e2 = (np.asarray(a, F) for a in (p, vert, e1, e2))
    shape = np.broadcast_shapes(p.shape, vert.shape, e1.shape, e2.shape)
    p, vert, e1, e2 = (np.moveaxis(np.broadcast_to(a, shape), -1, 0) for a in (p, vert, e1, e2))
    with np.errstate(all="ignore"):
        ap = (p - vert).astype(F)
        bp = (ap - e1).astype(F)
        cp = (ap - e2).astype(F)
        d1, d2 = _dot(e1, ap), _dot(e2, ap)
        d3, d4 = _dot(e1, bp), _dot(e2, bp)
        d5, d6 = _dot(e1, cp), _dot(e2, cp)
        vc = (d1 * d4 - d3 * d2).astype(F)
        vb = (d5 * d2 - d1 * d6).astype(F)
        va = (d3 * d6 - d5 * d4).astype(F)
        g = (d4 - d3).astype(F)
        h = (d5 - d6).astype(F)
        zero, one = np.zeros(shape[:-1], F), np.ones(shape[:-1], F)
        w = (g / (g + h).astype(F)).astype(F)
        den = (one / ((va + vb).astype(F) + vc).astype(F)).astype(F)
        rules = [
            ((d1 <= 0) & (d2 <= 0), 1, zero, zero),
            ((d3 >= 0) & (d4 <= d3), 2, one, zero),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), 4, (d1 / (d1 - d3).astype(F)).astype(F), zero),
            ((d6 >= 0) & (d5 <= d6), 3, zero, one),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 5, zero, (d2 / (d2 - d6).astype(F)).astype(F)),
            ((va <= 0) & (g >= 0) & (h >= 0), 6, (one - w).astype(F), w),
        ]
        region = np.zeros(shape[:-1], np.uint8)
        u, v = (vb * den).astype(F), (vc * den).astype(F)
        for cond, code, ru, rv in reversed(rules):  # the first rule that holds wins: applied last
            region = np.where(cond, np.uint8(code), region)
            u = np.where(cond, ru, u)
            v = np.where(cond, rv, v)
        u1 = np.where(u > 0, u, zero)
        u2 = np.where(u1 < 1, u1, one)
        r = (one - u2).astype(F)
        v1 = np.where(v > 0, v, zero)
        v2 = np.where(v1 < r, v1, r)
        q = [((ap[k] - (e1[k] * u2).astype(F)).astype(F) - (e2[k] * v2).astype(F)).astype(F) for k in range(3)]
        val = _dot(q, q)
        c = np.stack([((vert[k] + (e1[k] * u2).astype(F)).astype(F) + (e2[k] * v2).astype(F)).astype(F) for k in range(3)], axis=-1)
    return val, u2.astype(F), v2.astype(F), region, c


def true_dist2(p, vert, e1, e2):
    """the squared distance of p to the triangle (vert, vert + e1, vert + e2) in float64: Ericson's test on float64 values,
    degenerate triangles through the minimum over their three edges.  Shapes as pair_value's."""
    p, vert, e1, e2 = (np.asarray(a, np.float64) for a in (p, vert, e1, e2))

    def seg(a, d):  # squared distance of p to the segment a + t d, t in [0, 1]
        dd = (d * d).sum(-1)
        t = np.clip(np.where(dd > 0, ((p - a) * d).sum(-1) / np.where(dd > 0, dd, 1.0), 0.0), 0.0, 1.0)
        r = p - (a + t[..., None] * d)
        return (r * r).sum(-1)

    edges = np.minimum(np.minimum(seg(vert, e1), seg(vert, e2)), seg(vert + e1, e2 - e1))
    n = np.cross(e1, e2)
    nn = (n * n).sum(-1)
    ap = p - vert
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    # barycentrics of the projection: inside the triangle, the distance is the plane's
    u = (np.cross(ap, e2) * n).sum(-1) / nn1
    v = (np.cross(e1, ap) * n).sum(-1) / nn1
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    plane = ((ap * n).sum(-1)) ** 2 / nn1
    return np.where(inside, np.minimum(plane, edges), edges)


def records(prims):
    """(vert, e1, e2) of a TRIANGLE_DTYPE array as float32 (n, 3) arrays"""
    return (np.ascontiguousarray(prims[k], F).reshape(-1, 3) for k in ("vert", "e1", "e2"))


def valid_inputs(points, max_dist):
    points = np.asarray(points, F)
    ok = np.isfinite(points).all(axis=1)
    if max_dist is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(max_dist, F) >= 0  # false for a NaN
    return ok


def brute_values(points, prims, chunk_pairs=1 << 21):
    """(n points, m triangles) -> per point: the smallest F, the lowest index that has it, and how many triangles have it"""
    points = np.asarray(points, F)
    vert, e1, e2 = records(prims)
    n, m = points.shape[0], vert.shape[0]
    best = np.full(n, INF, F)
    arg = np.full(n, -1, np.int64)
    ties = np.zeros(n, np.int64)
    step = max(1, chunk_pairs // max(n, 1))
    for s in range(0, m, step):
        val = pair_value(points[:, None, :], vert[None, s:s + step], e1[None, s:s + step], e2[None, s:s + step])[0]
        val = np.where(np.isnan(val), INF, val)
        lo = val.min(axis=1)
        first = val.argmin(axis=1) + s  # argmin: the first of equal values
        cnt = (val == lo[:, None]).sum(axis=1)
        better = lo < best  # an earlier chunk keeps a tie: the lowest index wins
        ties = np.where(better, cnt, np.where(lo == best, ties + cnt, ties))
        arg = np.where(better, first, arg)
        best = np.where(better, lo, best)
    return best, arg, ties


def nearest(points, prims, max_dist=None, chunk_pairs=1 << 21):
    """tyr_query_nearest's five outputs: dist2 (n), prim (n) int32, uv (n, 2), region (n) uint8, point (n, 3)"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = points.shape[0]
    ok = valid_inputs(points, max_dist)
    with np.errstate(all="ignore"):
        bound2 = np.full(n, INF, F) if max_dist is None else (np.asarray(max_dist, F) * np.asarray(max_dist, F)).astype(F)
    safe = np.where(ok[:, None], points, F(0))
    best, arg, _ = brute_values(safe, prims, chunk_pairs) if len(prims) else (np.full(n, INF, F), np.full(n, -1, np.int64), None)
    hit = ok & (arg >= 0) & (best < bound2)
    dist2 = np.where(ok, bound2, INF).astype(F)
    prim = np.full(n, -1, np.int32)
    uv = np.zeros((n, 2), F)
    region = np.zeros(n, np.uint8)
    point = points.copy()
    if hit.any():
        vert, e1, e2 = records(prims)
        w = arg[hit]
        val, u2, v2, reg, c = pair_value(points[hit], vert[w], e1[w], e2[w])
        assert np.array_equal(val.view(np.uint32), best[hit].view(np.uint32))
        dist2[hit], prim[hit], region[hit], point[hit] = val, w.astype(np.int32), reg, c
        uv[hit, 0], uv[hit, 1] = u2, v2
    return dist2, prim, uv, region, point
