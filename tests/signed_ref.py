"""numpy restatement of tyr_query_signed and tyr_bake_sdf (include/tyr_c.h "Signed-distance queries"): the reference the GPU tests
compare against bit for bit.  A signed distance is defined through two contracts that have restatements of their own, and this
module only joins them: the closest point is nearest_ref.nearest's, the winding number winding_ref.winding's, and what is added
here is the header's sign, root, gradient, voxel-centre, brick and reach rules, operation by operation."""
import numpy as np

import nearest_ref
import winding_ref

F = np.float32
D = np.float64
QNAN = np.array([0x7FC00000], np.uint32).view(F)[0]
NAMES = ("sd", "prim", "point", "gradient", "w")
BRICK = 4
REACH_CELLS = F(2.625)


def tree_of(nodes, prims):
    """the moment tree of a scene, None for one without triangles"""
    return winding_ref.Tree(nodes, prims) if len(prims) else None


def join(points, max_dist, dist2, prim, point, w, prims):
    """the header's join of tyr_query_nearest's (dist2, prim, point) and tyr_query_winding's w: (sd, prim, point, gradient, w)"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = points.shape[0]
    ok = nearest_ref.valid_inputs(points, max_dist)
    md = np.full(n, np.inf, F) if max_dist is None else np.broadcast_to(np.asarray(max_dist, F), (n,)).copy()
    won = ok & (prim >= 0)
    with np.errstate(all="ignore"):
        inside = w > F(0.5)
        m = np.where(won, np.sqrt(dist2.astype(D)).astype(F), md)
        sd = np.where(inside, -m, m).astype(F)
        # the gradient, in binary64 from the binary32 p and point
        d = points.astype(D) - point.astype(D)
        away = won & (dist2 > 0) & (d != 0).any(axis=1)
        g = np.where(inside[:, None], -d, d)
        e1, e2 = prims["e1"].astype(D), prims["e2"].astype(D)
        idx = np.where(won, prim, 0).astype(np.int64)
        normal = winding_ref.cross(e1[idx], e2[idx]) if len(prims) else np.zeros((n, 3), D)
        g = np.where(away[:, None], g, normal)
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        has = won & (length > 0)
        gradient = np.where(has[:, None], (g / np.where(has, length, D(1.0))[:, None]).astype(F), F(0)).astype(F)
    sd[~ok] = QNAN
    w = w.copy()
    w[~ok] = QNAN
    return sd, np.where(ok, prim, -1).astype(np.int32), np.where(ok[:, None], point, points).astype(F), gradient, w


def signed(points, nodes, prims, max_dist=None, accuracy=2.0, tree=False):
    """tyr_query_signed's five outputs: sd (n), prim (n) int32, point (n, 3), gradient (n, 3), w (n).  tree: the scene's
    tree_of(), for a caller that asks more than once"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    if max_dist is not None:
        max_dist = np.broadcast_to(np.asarray(max_dist, F), (points.shape[0],))
    dist2, prim, _, _, point = nearest_ref.nearest(points, prims, max_dist)
    w, _ = winding_ref.winding(tree_of(nodes, prims) if tree is False else tree, points, accuracy)
    return join(points, max_dist, dist2, prim, point, w, prims)


# ---- the grid ---------------------------------------------------------------------------------------------------------
def voxel_axis(origin, cell, n):
    """origin + cell * ((float)i + 0.5f), every operation rounded to binary32"""
    return (F(origin) + (F(cell) * (np.arange(n).astype(F) + F(0.5)).astype(F)).astype(F)).astype(F)


def brick_axis(origin, cell, nb):
    """origin + cell * (float)(4 b + 2)"""
    return (F(origin) + (F(cell) * (BRICK * np.arange(nb) + 2).astype(F)).astype(F)).astype(F)


def reach(band, cell):
    return F(F(band) + F(REACH_CELLS * F(cell)))


def grid_points(axes):
    """(nz * ny * nx, 3) points of three per-axis arrays (x, y, z), x fastest"""
    x, y, z = axes
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], axis=1).astype(F)


def voxel_centres(origin, cell, dims):
    return grid_points([voxel_axis(origin[k], cell, dims[k]) for k in range(3)])


def bake(nodes, prims, origin, cell, dims, band, accuracy=2.0, tree=False, prims_near=None):
    """tyr_bake_sdf: (sd (nz, ny, nx), prim (nz, ny, nx) int32, stats uint32 (2), far (bz, by, bx) bool).  prims_near: None, or
    ascending indices of a subset of the triangles that holds every triangle within reach of a brick centre (a caller with a
    million triangles and a small window); the winding numbers always take the whole tree."""
    nx, ny, nz = (int(d) for d in dims)
    tree = tree_of(nodes, prims) if tree is False else tree
    sub = prims if prims_near is None else prims[prims_near]
    back = (lambda p: p) if prims_near is None else (lambda p: np.where(p >= 0, np.asarray(prims_near)[np.maximum(p, 0)], -1).astype(np.int32))
    nb = [(d + BRICK - 1) // BRICK for d in (nx, ny, nz)]
    centres = grid_points([brick_axis(origin[k], cell, nb[k]) for k in range(3)])
    r = reach(band, cell)
    _, cprim, _, _, _ = nearest_ref.nearest(centres, sub, np.full(len(centres), r, F))
    far = (cprim < 0).reshape(nb[2], nb[1], nb[0])
    with np.errstate(invalid="ignore"):
        wc = winding_ref.winding(tree, centres, accuracy)[0].reshape(far.shape)
        fill = np.where(wc > F(0.5), -F(band), F(band)).astype(F)
    # every voxel by the point query, then the far bricks' voxels overwritten by their brick's fill
    pts = voxel_centres(origin, cell, (nx, ny, nz))
    up = lambda a: np.repeat(np.repeat(np.repeat(a, BRICK, axis=0), BRICK, axis=1), BRICK, axis=2)[:nz, :ny, :nx]  # noqa: E731
    vfar = up(far)
    sd = up(fill).copy()
    prim = np.full((nz, ny, nx), -1, np.int32)
    near_idx = np.nonzero(~vfar.reshape(-1))[0]
    if near_idx.size:
        p = pts[near_idx]
        md = np.full(len(p), F(band), F)
        dist2, nprim, _, _, point = nearest_ref.nearest(p, sub, md)
        w, _ = winding_ref.winding(tree, p, accuracy)
        s, pr, _, _, _ = join(p, md, dist2, nprim, point, w, sub)
        sd.reshape(-1)[near_idx] = s
        prim.reshape(-1)[near_idx] = back(pr)
    stats = np.array([np.count_nonzero(~far), np.count_nonzero(far)], np.uint32)
    return sd, prim, stats, far
