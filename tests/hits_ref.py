"""numpy float32 restatement of tyr_query_hits (include/tyr_c.h "Multi-hit queries"): the reference the GPU tests compare against
bit for bit.  Every operation is one binary32 operation in the specified order (glm's dot and cross), divisions correctly
rounded.  The query is a set with no visit order in it, so the oracle is: the triangle value over ALL triangles, the accept
rule, the reach filter on the pairs that pass (a walk from the triangle's leaf to the root of the reference node array, every
box tested with the ray's tmax as Bbox.h:38-62 does), and a sort by (t, index)."""
import numpy as np

F = np.float32
EPSILON = F(0.001)        # variables.h:14
DET_MIN = F(0.0000001)    # loader.h:28
VERY_FAR = F(1e20)        # kernel.cu:15


def _dot(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]).astype(F)


def _cross(a, b):
    return [(a[1] * b[2] - b[1] * a[2]).astype(F), (a[2] * b[0] - b[2] * a[0]).astype(F), (a[0] * b[1] - b[0] * a[1]).astype(F)]


def triangle_value(o, d, vert, e1, e2, two_sided):
    """(t, u, v, side) of rays (o, d) against triangles (vert, e1, e2): arrays of shape (..., 3) that broadcast against each
    other.  t = 0 where one of the test's exits is taken (u, v, side are then meaningless); loader.h:21-46 as written, with
    two_sided the same operations for a negative determinant."""
    o, d, vert, e1, e2 = (np.asarray(a, F) for a in (o, d, vert, e1, e2))
    shape = np.broadcast_shapes(o.shape, d.shape, vert.shape, e1.shape, e2.shape)
    o, d, vert, e1, e2 = (np.moveaxis(np.broadcast_to(a, shape), -1, 0) for a in (o, d, vert, e1, e2))
    with np.errstate(all="ignore"):
        pvec = _cross(d, e2)
        det = _dot(e1, pvec)
        out = (np.abs(det) < DET_MIN) if two_sided else (det < DET_MIN)
        side = (det < 0) if two_sided else np.zeros(det.shape, bool)
        inv = (F(1) / det).astype(F)
        tvec = [(o[k] - vert[k]).astype(F) for k in range(3)]
        u = (_dot(tvec, pvec) * inv).astype(F)
        out = out | (u < 0) | (u > 1)
        qvec = _cross(tvec, e1)
        v = (_dot(d, qvec) * inv).astype(F)
        out = out | (v < 0) | ((u + v).astype(F) > 1)
        t = (_dot(e2, qvec) * inv).astype(F)
    return np.where(out, F(0), t), u, v, side.astype(np.uint8)


def _past_first_exits(o, d, vert, e1, e2, two_sided):
    """triangle_value up to its second exit: the pairs that take neither the determinant's exit nor u's"""
    o, d, vert, e1, e2 = (np.moveaxis(a, -1, 0) for a in (o, d, vert, e1, e2))
    with np.errstate(all="ignore"):
        pvec = _cross(d, e2)
        det = _dot(e1, pvec)
        out = (np.abs(det) < DET_MIN) if two_sided else (det < DET_MIN)
        inv = (F(1) / det).astype(F)
        tvec = [(o[k] - vert[k]).astype(F) for k in range(3)]
        u = (_dot(tvec, pvec) * inv).astype(F)
    return ~(out | (u < 0) | (u > 1))


def accepted(t, tmax):
    """bvh.h:229: t > epsilon && (tmax - t) > epsilon, false for a NaN"""
    with np.errstate(all="ignore"):
        return (t > EPSILON) & ((np.asarray(tmax, F) - t).astype(F) > EPSILON)


def records(prims):
    """(vert, e1, e2) of a TRIANGLE_DTYPE array as float32 (n, 3) arrays"""
    return tuple(np.ascontiguousarray(prims[k], F).reshape(-1, 3) for k in ("vert", "e1", "e2"))


def tree_tables(nodes):
    """(parent of every node, -1 for the root; leaf of every primitive) of the reference's depth-first node array
    (bvh.h:55-68: left child = index + 1, right child = offset, a leaf has primitiveCount > 0 and offset = its first primitive)"""
    n = len(nodes)
    parent = np.full(n, -1, np.int64)
    count = nodes["primitiveCount"].astype(np.int64)
    inner = np.nonzero(count == 0)[0]
    parent[inner + 1] = inner
    parent[nodes["offset"][inner]] = inner
    leaves = np.nonzero(count > 0)[0]
    n_prims = int((nodes["offset"][leaves] + count[leaves]).max()) if len(leaves) else 0
    leaf_of = np.full(n_prims, -1, np.int64)
    for i in leaves:
        leaf_of[nodes["offset"][i]:nodes["offset"][i] + count[i]] = i
    return parent, leaf_of


def box_passes(bounds, o, d, tmax):
    """BBox::intersect(origin, invDir, dirIsNeg, tmax) (Bbox.h:38-62) in float32, as oracle/orc_traverse.c restates it: bounds
    (k, 2, 3), o, d (k, 3), tmax (k)"""
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)  # bvh.h:216
        neg = inv < 0               # bvh.h:217
        lo = np.where(neg, bounds[:, 1], bounds[:, 0])
        hi = np.where(neg, bounds[:, 0], bounds[:, 1])
        t_min = ((lo[:, 0] - o[:, 0]) * inv[:, 0]).astype(F)
        t_max = ((hi[:, 0] - o[:, 0]) * inv[:, 0]).astype(F)
        ty_min = ((lo[:, 1] - o[:, 1]) * inv[:, 1]).astype(F)
        ty_max = ((hi[:, 1] - o[:, 1]) * inv[:, 1]).astype(F)
        ok = ~((t_min > ty_max) | (ty_min > t_max))
        t_min = np.where(ty_min > t_min, ty_min, t_min)
        t_max = np.where(ty_max < t_max, ty_max, t_max)
        tz_min = ((lo[:, 2] - o[:, 2]) * inv[:, 2]).astype(F)
        tz_max = ((hi[:, 2] - o[:, 2]) * inv[:, 2]).astype(F)
        ok &= ~((t_min > tz_max) | (tz_min > t_max))
        t_min = np.where(tz_min > t_min, tz_min, t_min)
        t_max = np.where(tz_max < t_max, tz_max, t_max)
        return ok & (t_min < tmax) & (t_max > 0)


def reached(nodes, tables, ray, prim, o, d, tmax):
    """of the pairs (ray[k], prim[k]): those whose triangle is in R(ray) -- the leaf and every ancestor pass the box test"""
    parent, leaf_of = tables
    node = leaf_of[prim]
    alive = np.ones(len(ray), bool)
    bounds = nodes["bounds"].astype(F)
    while True:
        todo = np.nonzero(alive & (node >= 0))[0]
        if todo.size == 0:
            break
        r = ray[todo]
        alive[todo] = box_passes(bounds[node[todo]], o[r], d[r], tmax[r])
        node[todo] = parent[node[todo]]
    return alive


class Hits:
    """every member of H of every ray of a batch, sorted by (ray, t, prim): `answer(max_hits)` cuts tyr_query_hits's six
    outputs from it, for any max_hits"""

    def __init__(self, origins, directions, nodes, prims, tmax=None, two_sided=False, chunk_pairs=1 << 21):
        o = np.ascontiguousarray(origins, F).reshape(-1, 3)
        d = np.ascontiguousarray(directions, F).reshape(-1, 3)
        n = o.shape[0]
        self.n = n
        self.tmax = np.full(n, VERY_FAR, F) if tmax is None else np.ascontiguousarray(tmax, F).reshape(n)
        valid = np.nonzero(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1))[0]
        vert, e1, e2 = records(prims)
        m = vert.shape[0]
        rays, tris = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        step = max(1, chunk_pairs // max(valid.size, 1))
        if valid.size:
            for s in range(0, m, step):
                # the test's first two exits on the whole chunk, the rest of it on the pairs that are left (the same operations)
                r, p = np.nonzero(_past_first_exits(o[valid, None, :], d[valid, None, :], vert[None, s:s + step], e1[None, s:s + step], e2[None, s:s + step], two_sided))
                r, p = valid[r], p + s
                ok = accepted(triangle_value(o[r], d[r], vert[p], e1[p], e2[p], two_sided)[0], self.tmax[r])
                rays.append(r[ok])
                tris.append(p[ok])
        ray, prim = np.concatenate(rays), np.concatenate(tris)
        self.tested = int(ray.size)  # pairs that pass the triangle test and the accept rule, before the reach filter
        if ray.size:
            keep = reached(np.ascontiguousarray(nodes), tree_tables(nodes), ray, prim, o, d, self.tmax)
            ray, prim = ray[keep], prim[keep]
        self.removed = self.tested - int(ray.size)  # ... of which the reach filter removed this many
        t, u, v, side = triangle_value(o[ray], d[ray], vert[prim], e1[prim], e2[prim], two_sided)
        order = np.lexsort((prim, t, ray))
        self.ray, self.prim, self.t, self.u, self.v, self.side = ray[order], prim[order].astype(np.int32), t[order], u[order], v[order], side[order]
        self.count = np.bincount(self.ray, minlength=n).astype(np.uint32)
        self.back_count = np.bincount(self.ray, weights=self.side, minlength=n).astype(np.uint32)
        first = np.concatenate([[0], np.cumsum(self.count)[:-1]]).astype(np.int64)
        self.rank = np.arange(self.ray.size) - first[self.ray]  # place of a hit in its ray's list

    def answer(self, max_hits):
        """(count, t, prim, uv, side, back_count) as tyr_query_hits writes them"""
        n, k = self.n, int(max_hits)
        t = np.repeat(self.tmax[:, None], k, axis=1).astype(F)
        prim = np.full((n, k), -1, np.int32)
        uv = np.zeros((n, k, 2), F)
        side = np.zeros((n, k), np.uint8)
        sel = self.rank < k
        r, j = self.ray[sel], self.rank[sel]
        t[r, j], prim[r, j], side[r, j] = self.t[sel], self.prim[sel], self.side[sel]
        uv[r, j, 0], uv[r, j, 1] = self.u[sel], self.v[sel]
        return self.count.copy(), t, prim, uv, side, self.back_count.copy()


def hits(origins, directions, nodes, prims, tmax=None, max_hits=4, two_sided=False):
    """tyr_query_hits's six outputs"""
    return Hits(origins, directions, nodes, prims, tmax, two_sided).answer(max_hits)
