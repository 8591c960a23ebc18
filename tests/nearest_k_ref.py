"""numpy float32 restatement of tyr_query_nearest_k (include/tyr_c.h "k-nearest queries"): the reference the GPU tests compare
against bit for bit.  The value of a (point, triangle) pair is nearest_ref.pair_value, the restatement of "Closest-point
queries"; the query is a set over all triangles with no traversal order in it, so brute force over the uploaded array, in
chunks, with a stable sort by (F, index) is the whole oracle."""
import numpy as np

from nearest_ref import INF, F, pair_value, records, valid_inputs


def nearest_k(points, prims, k, max_dist=None, chunk_pairs=1 << 21):
    """tyr_query_nearest_k's six outputs: dist2 (n, k), prim (n, k) int32, uv (n, k, 2), region (n, k) uint8, point (n, k, 3) and
    count (n,) int64 -- |W|, not capped by k"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = points.shape[0]
    ok = valid_inputs(points, max_dist)
    with np.errstate(all="ignore"):
        bound2 = np.full(n, INF, F) if max_dist is None else (np.asarray(max_dist, F) * np.asarray(max_dist, F)).astype(F)
    bound2 = np.where(ok, bound2, INF).astype(F)
    safe = np.where(ok[:, None], points, F(0))
    vert, e1, e2 = records(prims)
    m = vert.shape[0]
    best = np.full((n, k), INF, F)  # the k smallest pairs so far, sorted by (F, index); +inf: no member
    arg = np.full((n, k), -1, np.int64)
    count = np.zeros(n, np.int64)
    step = max(1, chunk_pairs // max(n, 1))
    for s in range(0, m, step):
        val = pair_value(safe[:, None, :], vert[None, s:s + step], e1[None, s:s + step], e2[None, s:s + step])[0]
        with np.errstate(invalid="ignore"):
            member = ok[:, None] & (val < bound2[:, None])  # strict; false for a NaN
        count += member.sum(axis=1)
        val = np.where(member, val, INF)
        idx = np.where(member, np.arange(s, s + val.shape[1])[None, :], -1)
        # what is kept has lower indices than the chunk's and is sorted; the chunk is in index order: a stable sort by F alone
        # orders the whole by (F, index)
        allv, alli = np.concatenate([best, val], axis=1), np.concatenate([arg, idx], axis=1)
        order = np.argsort(allv, axis=1, kind="stable")[:, :k]
        best, arg = np.take_along_axis(allv, order, axis=1), np.take_along_axis(alli, order, axis=1)
    kept = arg >= 0
    dist2 = np.where(kept, best, bound2[:, None]).astype(F)
    prim = arg.astype(np.int32)
    uv = np.zeros((n, k, 2), F)
    region = np.zeros((n, k), np.uint8)
    point = np.repeat(points[:, None, :], k, axis=1)
    if kept.any():
        i, j = np.nonzero(kept)
        w = arg[i, j]
        val, u2, v2, reg, c = pair_value(points[i], vert[w], e1[w], e2[w])
        assert np.array_equal(val.view(np.uint32), best[i, j].view(np.uint32))
        region[i, j], point[i, j] = reg, c
        uv[i, j, 0], uv[i, j, 1] = u2, v2
    return dist2, prim, uv, region, point, count
