"""numpy restatement of tyr_query_tri (include/tyr_c.h "Triangle-overlap queries"): the reference the GPU tests compare against
bit for bit.  The member test of a (query, scene triangle) pair is rule 0 (equal corners, with skip_shared only), rule 1 (the
three coordinate axes, exact comparisons of the binary32 corners) and rule 2 (seventeen axes in binary64, every one of the six
corners projected by the same dot(axis, x)), with tests/box_ref.py's dot, cross, min and max: one IEEE operation per operation
written.  The answer per query is a set over all triangles with no traversal order in it, so brute force over the uploaded
array, in chunks, is the whole oracle.  `pair_exact` is an independent check of the definition itself: the same rules in exact
integer arithmetic on the same binary32 inputs."""
from fractions import Fraction

import numpy as np

from box_ref import _cross, _dot, _max, _min, _sub, corners, records  # noqa: F401  (corners, records: for the callers)

F = np.float32
D = np.float64
SHARED = 21  # pair()'s code for rule 0; 1-3 rule 1's axes x y z; 4-20 rule 2's axes in the header's order
AXES = ["member", "x", "y", "z", "m", "n"] + [f"e{i} x f{j}" for i in range(3) for j in range(3)] + [f"n x e{i}" for i in range(3)] + [f"m x f{j}" for j in range(3)] + ["shared"]


def valid_queries(a, b, c):
    """every component of the three corners finite"""
    return np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1) & np.isfinite(c).all(axis=-1)


def _rule2_axes(p, q):
    """the seventeen axes of rule 2 in the header's order, from the relative corners p = [p0, p1, p2], q = [q0, q1, q2]"""
    e = [_sub(p[1], p[0]), _sub(p[2], p[1]), _sub(p[0], p[2])]
    f = [_sub(q[1], q[0]), _sub(q[2], q[1]), _sub(q[0], q[2])]
    n = _cross(e[0], _sub(p[2], p[0]))
    m = _cross(f[0], _sub(q[2], q[0]))
    return [m, n] + [_cross(e[i], f[j]) for i in range(3) for j in range(3)] + [_cross(n, e[i]) for i in range(3)] + [_cross(m, f[j]) for j in range(3)]


def _fold(op, xs):
    out = xs[0]
    for x in xs[1:]:
        out = op(out, x)
    return out


def _coordinate_rows(P, Q):
    """rule 1 on component-major corners: for k = x, y, z whether that coordinate axis separates"""
    rows = []
    for k in range(3):
        pk, qk = [x[k] for x in P], [x[k] for x in Q]
        rows.append((_fold(_min, pk) > _fold(_max, qk)) | (_fold(_max, pk) < _fold(_min, qk)))
    return rows


def _coordinate_axes(P, Q):
    """0 where no coordinate axis separates, else 1, 2, 3 for the first that does"""
    x, y, z = _coordinate_rows(P, Q)
    return np.where(x, np.int8(1), np.where(y, np.int8(2), np.where(z, np.int8(3), np.int8(0))))


def _shared(P, Q):
    """rule 0 on component-major corners: some Pi equals some Qj on all three components (== on binary32 values: -0 equals +0)"""
    out = False
    for Pi in P:
        for Qj in Q:
            out = out | ((Pi[0] == Qj[0]) & (Pi[1] == Qj[1]) & (Pi[2] == Qj[2]))
    return out


def separating(a, b, c, vert, e1, e2):
    """every axis on its own, for arrays as pair() takes them: (bool (20, ...), row k - 1 whether the axis with pair()'s code k
    separates; bool (...), whether some corners are equal: rule 0's condition)"""
    P = [np.asarray(x, F).astype(D) for x in (a, b, c)]
    Q = list(corners(vert, e1, e2))
    shape = np.broadcast_shapes(*(x.shape for x in P + Q))
    P = [np.moveaxis(np.broadcast_to(x, shape), -1, 0) for x in P]
    Q = [np.moveaxis(np.broadcast_to(x, shape), -1, 0) for x in Q]
    with np.errstate(all="ignore"):
        rows = _coordinate_rows(P, Q)
        p = [_sub(x, Q[0]) for x in P]
        q = [_sub(x, Q[0]) for x in Q]
        for axis in _rule2_axes(p, q):
            pp, qq = [_dot(axis, x) for x in p], [_dot(axis, x) for x in q]
            rows.append((_fold(_max, pp) < _fold(_min, qq)) | (_fold(_max, qq) < _fold(_min, pp)))
    return np.stack(rows), _shared(P, Q)


def pair(a, b, c, vert, e1, e2, skip_shared=False):
    """the first rule that makes query triangles (a, b, c) and scene triangles (vert, e1, e2) non-members, arrays of shape
    (..., 3) that broadcast against each other: 0 none (the pair is a member), 1-3 the coordinate axes x y z, 4 the scene
    triangle's normal m, 5 the query's normal n, 6-14 cross(e_i, f_j) (i outer), 15-17 cross(n, e_i), 18-20 cross(m, f_j), and
    SHARED for rule 0 (with skip_shared only; it comes first)"""
    sep, shared = separating(a, b, c, vert, e1, e2)
    first = np.where(sep.any(axis=0), sep.argmax(axis=0) + 1, 0).astype(np.int8)
    return np.where(shared, np.int8(SHARED), first) if skip_shared else first


def members(a, b, c, vert, e1, e2, skip_shared=False):
    """(n queries, m triangles) -> bool (n, m): pair(...) == 0, with rule 2 evaluated only for the pairs no coordinate axis
    separates (rule 1 is exact comparisons of the inputs)"""
    P = [[x[:, None, k].astype(D) for k in range(3)] for x in (a, b, c)]
    Q = [[x[None, :, k] for k in range(3)] for x in corners(vert, e1, e2)]
    cand = _coordinate_axes(P, Q) == 0
    qi, ti = np.nonzero(cand)
    out = np.zeros(cand.shape, bool)
    if qi.size:
        out[qi, ti] = pair(a[qi], b[qi], c[qi], vert[ti], e1[ti], e2[ti], skip_shared) == 0
    return out


def tri(a, b, c, prims, max_prims=0, any=False, skip_shared=False, chunk_pairs=1 << 22):
    """tyr_query_tri's answer by brute force over all triangles: (count (n,) int32, prim (n, max_prims) int32, the lowest
    build-order indices of the members ascending, -1 for an unused entry); with any=True the bool array count > 0 alone"""
    a, b, c = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (a, b, c))
    n, k = a.shape[0], int(max_prims)
    ok = valid_queries(a, b, c)
    sa, sb, sc = (np.where(ok[:, None], x, F(0)) for x in (a, b, c))  # an invalid query: masked out below
    count = np.zeros(n, np.int64)
    fill = np.zeros(n, np.int64)
    prim = np.full((n, k), -1, np.int32)
    vert, e1, e2 = records(prims)
    m = vert.shape[0]
    step = max(1, chunk_pairs // max(n, 1))
    for s in range(0, m, step):
        mem = members(sa, sb, sc, vert[s:s + step], e1[s:s + step], e2[s:s + step], skip_shared) & ok[:, None]
        per = mem.sum(axis=1)
        if k:
            qi, ti = np.nonzero(mem)  # by query, then ascending triangle
            start = np.concatenate([[0], np.cumsum(per)[:-1]])
            slot = fill[qi] + (np.arange(qi.size) - start[qi])
            keep = slot < k
            prim[qi[keep], slot[keep]] = (ti[keep] + s).astype(np.int32)
            fill = np.minimum(fill + per, k)
        count += per
    if any:
        return count > 0
    return count.astype(np.int32), prim


# ---- the same test in exact integer arithmetic ---------------------------------------------------------------------------
def pair_exact(a, b, c, vert, e1, e2, skip_shared=False):
    """pair() for one query and one scene triangle (sequences of 3 binary32 values each): the corners are the same binary32
    values and sums, scaled to integers over their common power-of-two denominator; everything behind them is exact.  Every
    comparison is between sums of products of the same degree, so the integers' answer is the rationals'."""
    P = [[Fraction(float(F(x))) for x in p] for p in (a, b, c)]
    Q = [[Fraction(float(x)) for x in p.reshape(3).tolist()] for p in corners(vert, e1, e2)]
    if skip_shared and any(Pi == Qj for Pi in P for Qj in Q):
        return SHARED
    for k in range(3):
        pk, qk = [x[k] for x in P], [x[k] for x in Q]
        if min(pk) > max(qk) or max(pk) < min(qk):
            return k + 1
    den = max(x.denominator for pt in P + Q for x in pt)
    P, Q = ([[int(x * den) for x in pt] for pt in T] for T in (P, Q))
    p, q = [_sub(x, Q[0]) for x in P], [_sub(x, Q[0]) for x in Q]
    for code, axis in enumerate(_rule2_axes(p, q), start=4):
        pp, qq = [_dot(axis, x) for x in p], [_dot(axis, x) for x in q]
        if max(pp) < min(qq) or max(qq) < min(pp):
            return code
    return 0
