"""numpy restatement of tyr_query_box (include/tyr_c.h "Box-overlap queries"): the reference the GPU tests compare against bit
for bit.  The member test of a (box, triangle) pair is the separating-axis test over 13 axes in binary64, one IEEE operation per
operation written, dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, cross as the winding block's, min(a, b) = b < a ? b : a and
max(a, b) = b > a ? b : a; inputs are binary32 widened exactly.  The answer per box is a set over all triangles with no traversal
order in it, so brute force over the uploaded array, in chunks, is the whole oracle.  `pair_exact` is an independent check of the
definition itself: the same 13 axes in exact rational arithmetic on the same binary32 inputs."""
from fractions import Fraction

import numpy as np

F = np.float32
D = np.float64
UNITS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _min(a, b):
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(b > a, b, a)


def corners(vert, e1, e2):
    """A = vert, B = the binary32 sum vert + e1, C = the binary32 sum vert + e2, widened: the corners tyr_triangle_bboxes bounds"""
    vert, e1, e2 = (np.asarray(a, F) for a in (vert, e1, e2))
    with np.errstate(all="ignore"):
        return vert.astype(D), (vert + e1).astype(F).astype(D), (vert + e2).astype(F).astype(D)


def records(prims):
    """(vert, e1, e2) of a TRIANGLE_DTYPE array as float32 (n, 3) arrays"""
    return (np.ascontiguousarray(prims[k], F).reshape(-1, 3) for k in ("vert", "e1", "e2"))


def valid_boxes(lo, hi):
    """every component finite and lo_k <= hi_k on every axis"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(lo).all(axis=-1) & np.isfinite(hi).all(axis=-1) & (lo <= hi).all(axis=-1)


def _box_axes(lo, hi, A, B, C):
    """rule 1 on component-major operands: 0 where no box axis separates, else 1, 2, 3 for the first that does"""
    out = np.zeros(np.broadcast_shapes(lo[0].shape, A[0].shape), np.int8)
    for k in (2, 1, 0):  # the first axis that separates wins: applied last
        sep = (_min(A[k], _min(B[k], C[k])) > hi[k]) | (_max(A[k], _max(B[k], C[k])) < lo[k])
        out = np.where(sep, np.int8(k + 1), out)
    return out


def pair(lo, hi, vert, e1, e2):
    """the first separating axis of boxes [lo, hi] against triangles (vert, e1, e2), arrays of shape (..., 3) that broadcast
    against each other: 0 none (the pair is a member), 1-3 the box axes x y z, 4 the triangle's plane, 5-13 the edge axes
    cross(unit_i, f) for i = x, y, z (outer) and f = e1', e2' - e1', e2' (inner)"""
    A, B, C = corners(vert, e1, e2)
    lo, hi = np.asarray(lo, F).astype(D), np.asarray(hi, F).astype(D)
    shape = np.broadcast_shapes(lo.shape, hi.shape, A.shape)
    lo, hi, A, B, C = (np.moveaxis(np.broadcast_to(a, shape), -1, 0) for a in (lo, hi, A, B, C))
    with np.errstate(all="ignore"):
        first = _box_axes(lo, hi, A, B, C).astype(np.int8)
        l, h = _sub(lo, A), _sub(hi, A)
        f1, f2 = _sub(B, A), _sub(C, A)
        zero = np.zeros(shape[:-1], D)

        def separated(a, ps):
            bmin = (_min(a[0] * l[0], a[0] * h[0]) + _min(a[1] * l[1], a[1] * h[1])) + _min(a[2] * l[2], a[2] * h[2])
            bmax = (_max(a[0] * l[0], a[0] * h[0]) + _max(a[1] * l[1], a[1] * h[1])) + _max(a[2] * l[2], a[2] * h[2])
            pmax, pmin = ps[0], ps[0]
            for p in ps[1:]:
                pmax, pmin = _max(pmax, p), _min(pmin, p)
            return (pmax < bmin) | (pmin > bmax)

        tests = [(4, _cross(f1, f2), [zero])]
        for i, unit in enumerate(UNITS):
            u = [np.full(shape[:-1], c, D) for c in unit]
            for j, f in enumerate((f1, _sub(f2, f1), f2)):
                a = _cross(u, f)
                tests.append((5 + 3 * i + j, a, [zero, _dot(a, f1), _dot(a, f2)]))
        for code, a, ps in tests:
            first = np.where((first == 0) & separated(a, ps), np.int8(code), first)
    return first


def members(lo, hi, vert, e1, e2):
    """(n boxes, m triangles) -> bool (n, m): pair(...) == 0, with the plane and edge axes evaluated only for the pairs no box axis
    separates (rule 1 is exact comparisons of the inputs: the same in binary32)"""
    A, B, C = corners(vert, e1, e2)
    cand = _box_axes([lo[:, None, k] for k in range(3)], [hi[:, None, k] for k in range(3)], *([a[None, :, k] for k in range(3)] for a in (A, B, C))) == 0
    bi, ti = np.nonzero(cand)
    out = np.zeros(cand.shape, bool)
    if bi.size:
        out[bi, ti] = pair(lo[bi], hi[bi], vert[ti], e1[ti], e2[ti]) == 0
    return out


def box(lo, hi, prims, max_prims=0, any=False, chunk_pairs=1 << 22):
    """tyr_query_box's answer by brute force over all triangles: (count (n,) int32, prim (n, max_prims) int32, the lowest
    build-order indices of the members ascending, -1 for an unused entry); with any=True the bool array count > 0 alone"""
    lo = np.ascontiguousarray(lo, F).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, F).reshape(-1, 3)
    n, k = lo.shape[0], int(max_prims)
    ok = valid_boxes(lo, hi)
    slo, shi = np.where(ok[:, None], lo, F(1)), np.where(ok[:, None], hi, F(0))  # an invalid box: empty, nothing is inside
    count = np.zeros(n, np.int64)
    fill = np.zeros(n, np.int64)
    prim = np.full((n, k), -1, np.int32)
    vert, e1, e2 = records(prims)
    m = vert.shape[0]
    step = max(1, chunk_pairs // max(n, 1))
    for s in range(0, m, step):
        mem = members(slo, shi, vert[s:s + step], e1[s:s + step], e2[s:s + step]) & ok[:, None]
        per = mem.sum(axis=1)
        if k:
            bi, ti = np.nonzero(mem)  # by box, then ascending triangle
            start = np.concatenate([[0], np.cumsum(per)[:-1]])
            slot = fill[bi] + (np.arange(bi.size) - start[bi])
            keep = slot < k
            prim[bi[keep], slot[keep]] = (ti[keep] + s).astype(np.int32)
            fill = np.minimum(fill + per, k)
        count += per
    if any:
        return count > 0
    return count.astype(np.int32), prim


# ---- the same test in exact rational arithmetic --------------------------------------------------------------------------
def pair_exact(lo, hi, vert, e1, e2):
    """pair() for one box and one triangle (sequences of 3 binary32 values each) in fractions.Fraction: the corners are the
    same binary32 sums, everything behind them is exact"""
    A, B, C = ([Fraction(float(x)) for x in p.tolist()] for p in (a[...].reshape(3) for a in corners(vert, e1, e2)))
    lo, hi = ([Fraction(float(F(x))) for x in p] for p in (lo, hi))
    for k in range(3):
        if min(A[k], B[k], C[k]) > hi[k] or max(A[k], B[k], C[k]) < lo[k]:
            return k + 1
    # binary32 values over a common power-of-two denominator: integers, and every comparison below is between sums of products
    # of the same degree, so the integers' answer is the rationals'
    den = max(x.denominator for x in A + B + C + lo + hi)
    A, B, C, lo, hi = ([int(x * den) for x in p] for p in (A, B, C, lo, hi))
    l, h = _sub(lo, A), _sub(hi, A)
    f1, f2 = _sub(B, A), _sub(C, A)

    def separated(a, ps):
        bmin = sum(min(a[k] * l[k], a[k] * h[k]) for k in range(3))
        bmax = sum(max(a[k] * l[k], a[k] * h[k]) for k in range(3))
        return max(ps) < bmin or min(ps) > bmax

    if separated(_cross(f1, f2), [0]):
        return 4
    for i in range(3):
        u = [1 if k == i else 0 for k in range(3)]
        for j, f in enumerate((f1, _sub(f2, f1), f2)):
            a = _cross(u, f)
            if separated(a, [0, _dot(a, f1), _dot(a, f2)]):
                return 5 + 3 * i + j
    return 0
