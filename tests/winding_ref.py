"""numpy restatement of the winding-number contract (include/tyr_c.h "Winding numbers"): the moment tree of a node array and the
stackless walk that sums a point's series, every operation a binary64 numpy operation in the header's order, so that the
device's words can be compared by bits.  Vectorised over points by walking the nodes depth-first with the subset of points
that reach each one: every point's terms are added in that point's own order, leaf triangles one at a time.

Also the truth the definition is held to: truth(), the brute-force binary64 sum over every triangle with numpy.arctan2."""
import numpy as np

D = np.float64
F = np.float32
U = np.uint32

INV_4PI = float.fromhex("0x1.45f306dc9c883p-4")
PI = float.fromhex("0x1.921fb54442d18p+1")
PIO2 = float.fromhex("0x1.921fb54442d18p+0")
PIO4 = float.fromhex("0x1.921fb54442d18p-1")
TAN_PIO8 = float.fromhex("0x1.a827999fcef32p-2")
SERIES = [D((-1.0) ** k) / D(2 * k + 1) for k in range(17)]  # one correctly rounded division each
QNAN = 0x7FC00000


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def max_second(a, b):
    return np.where(b > a, b, a)


def atan2_det(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, D), np.asarray(x, D))
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        steep = ay > ax
        mx, mn = np.where(steep, ay, ax), np.where(steep, ax, ay)
        t = np.where(mx == 0.0, D(0.0), mn / np.where(mx == 0.0, D(1.0), mx))
        fold = t > TAN_PIO8
        u = np.where(fold, (t - 1.0) / (t + 1.0), t)
        z = u * u
        p = np.full(z.shape, SERIES[16], D)
        for k in range(15, -1, -1):
            p = p * z + SERIES[k]
        r = np.where(fold, D(PIO4), D(0.0)) + u * p
        r = np.where(steep, PIO2 - r, r)
        r = np.where(x < 0.0, PI - r, r)
        r = np.where(y < 0.0, -r, r)
    return r


def skips(nodes):
    """skip(i), top-down as the contract words it: nNodes for the root, the parent's offset for a left child, the parent's skip
    for a right child"""
    n = nodes.shape[0]
    out = np.zeros(n, np.int64)
    if n == 0:
        return out
    out[0] = n
    for i in range(n):  # a parent lies in front of its children
        if nodes["primitiveCount"][i] == 0:
            off = int(nodes["offset"][i])
            out[i + 1] = off
            out[off] = out[i]
    return out


class Tree:
    """p (n, 3), N (n, 3), r2 (n), S (n), skip (n) of a node array and its triangles"""

    def __init__(self, nodes, prims):
        n = nodes.shape[0]
        self.nodes, self.prims = nodes, prims
        self.vert, self.e1, self.e2 = (prims[k].astype(D) for k in ("vert", "e1", "e2"))
        with np.errstate(all="ignore"):
            nt = 0.5 * cross(self.e1, self.e2)
            at = np.sqrt(dot(nt, nt))
            ct = self.vert + (self.e1 + self.e2) / 3.0
            mt = at[:, None] * ct
            N, S, M = np.zeros((n, 3), D), np.zeros(n, D), np.zeros((n, 3), D)
            count, offset = nodes["primitiveCount"].astype(np.int64), nodes["offset"].astype(np.int64)
            for i in range(n - 1, -1, -1):  # children lie behind their parent
                if count[i] > 0:
                    for t in range(offset[i], offset[i] + count[i]):
                        N[i] = N[i] + nt[t]
                        S[i] = S[i] + at[t]
                        M[i] = M[i] + mt[t]
                else:
                    N[i], S[i], M[i] = N[i + 1] + N[offset[i]], S[i + 1] + S[offset[i]], M[i + 1] + M[offset[i]]
            lo, hi = nodes["bounds"][:, 0].astype(D), nodes["bounds"][:, 1].astype(D)
            has = S > 0.0
            p = np.where(has[:, None], M / np.where(has, S, D(1.0))[:, None], 0.5 * (lo + hi))
            dl, dh = lo - p, hi - p
            m = max_second(dl * dl, dh * dh)
            self.r2 = (m[:, 0] + m[:, 1]) + m[:, 2]
        self.p, self.N, self.S, self.M = p, N, S, M
        self.skip = skips(nodes)
        self.count, self.offset = count, offset

    def moments(self):
        """what tyr_scene_moments reports: (n, 8) p xyz, N xyz, r2, S"""
        return np.concatenate([self.p, self.N, self.r2[:, None], self.S[:, None]], axis=1)


def omega(q, vert, e1, e2):
    """the solid angle of one triangle at the points q (m, 3)"""
    a, b, c = vert - q, (vert + e1) - q, (vert + e2) - q
    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    det = dot(a, cross(b, c))
    den = ((la * lb) * lc + dot(a, b) * lc) + (dot(b, c) * la + dot(c, a) * lb)
    return 2.0 * atan2_det(det, den)


def winding(tree, points, accuracy):
    """(w float32 (n,), terms uint32 (n, 2)) of the contract's walk; tree: a Tree, or None for a scene without triangles"""
    pts = np.asarray(points, F).reshape(-1, 3)
    n = pts.shape[0]
    ok = np.isfinite(pts).all(axis=1)
    q = pts.astype(D)
    total = np.zeros(n, D)
    terms = np.zeros((n, 2), U)
    B2 = D(F(accuracy)) * D(F(accuracy))
    nn = 0 if tree is None else tree.nodes.shape[0]
    stack = [(0, np.nonzero(ok)[0])] if nn else []
    with np.errstate(all="ignore"):
        while stack:
            i, idx = stack.pop()
            if idx.size == 0:
                continue
            d = tree.p[i] - q[idx]
            d2 = dot(d, d)
            far = d2 > B2 * tree.r2[i]
            f = idx[far]
            if f.size:
                total[f] = total[f] + dot(d[far], tree.N[i]) / (d2[far] * np.sqrt(d2[far]))
                terms[f, 0] += 1
            near = idx[~far]
            if near.size == 0:
                continue
            if tree.count[i] > 0:
                for t in range(tree.offset[i], tree.offset[i] + tree.count[i]):
                    total[near] = total[near] + omega(q[near], tree.vert[t], tree.e1[t], tree.e2[t])
                terms[near, 1] += U(tree.count[i])
            else:
                stack.append((int(tree.offset[i]), near))  # the right child after the whole left subtree
                stack.append((i + 1, near))
        w = (total * INV_4PI).astype(F)
    w[~ok] = np.array([QNAN], U).view(F)[0]
    return w, terms


def truth(prims, points, chunk=256):
    """the winding number as binary64: every triangle's solid angle with numpy.arctan2, summed pairwise by numpy"""
    q = np.asarray(points, F).reshape(-1, 3).astype(D)
    vert, e1, e2 = (prims[k].astype(D) for k in ("vert", "e1", "e2"))
    out = np.zeros(q.shape[0], D)
    for s in range(0, q.shape[0], chunk):
        a = vert[None] - q[s:s + chunk, None]
        b, c = a + e1[None], a + e2[None]
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        det = np.einsum("ijk,ijk->ij", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ijk,ijk->ij", a, b) * lc + np.einsum("ijk,ijk->ij", b, c) * la + np.einsum("ijk,ijk->ij", c, a) * lb
        out[s:s + chunk] = (2.0 * np.arctan2(det, den)).sum(axis=1) / (4.0 * np.pi)
    return out
