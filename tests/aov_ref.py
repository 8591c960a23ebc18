"""What tyr_render_aov's answers are compared with (tests/test_aov.py, tests/test_specular_guides.py, tests/test_query_shapes.py;
tests/specular_ref.py restates the chain pass on top of it): the oracle's first wavefront -- begin, primary, extend with
queue_size = spp * P, every sample's record in ticket order -- and the first-hit guides restated from those records."""
import numpy as np

from conftest import bits

VERY_FAR = np.float32(1e20)


def flags_of(sc):
    return (1 if sc.triangle_materials else 0) | (8 if sc.light_list else 0) | (16 if sc.triangle_colors else 0)


def expected_aov(hip, q, sc, prims, spheres, spp, W, H, colors):
    """the AOVs of a queue of camera-ray records in ticket order (record i = sample i // P of local pixel i % P) after
    extend: shade's albedo and face-forwarded normal per hit (normals through tyr_vecmath_probe, pinned to glm), float32
    sums in s order"""
    P = q.shape[0] // spp
    q = q.reshape(spp, P)
    alb_sum = np.zeros((P, 3), np.float32)
    nrm_sum = np.zeros((P, 3), np.float32)
    tsum = np.zeros(P, np.float32)
    hits = np.zeros(P, np.int64)
    for s in range(spp):
        r = q[s]
        hit = r["distance"] < VERY_FAR
        sph = hit & (r["geometry_type"] == 0)
        tri = hit & (r["geometry_type"] == 1)
        o, d, t = r["origin"].astype(np.float32), r["direction"].astype(np.float32), r["distance"].astype(np.float32)
        alb = np.zeros((P, 3), np.float32)
        n = np.zeros((P, 3), np.float32)
        if sph.any():
            sp = spheres[r["identifier"][sph]]
            at = hip.vecmath_probe(18, o[sph], hip.vecmath_probe(12, d[sph], d[sph], np.repeat(t[sph, None], 3, 1)), o[sph])  # o + d * t
            diff = hip.vecmath_probe(19, at, sp["position"].astype(np.float32), at)
            n[sph] = hip.vecmath_probe(11, diff, diff, np.repeat(sp["radius"].astype(np.float32)[:, None], 3, 1))
            alb[sph] = sp["color"]
        if tri.any():
            tr = prims[r["identifier"][tri]]
            cr = hip.vecmath_probe(1, tr["e1"], tr["e2"], tr["e1"])
            n[tri] = hip.vecmath_probe(2, cr, cr, cr)
            alb[tri] = sc.palette_color[tr["pad_"][:, 0]].astype(np.float32) if colors else 1.0
        if hit.any():
            dn = hip.vecmath_probe(0, n[hit], d[hit], d[hit])[:, 0]
            flip = hip.vecmath_probe(12, n[hit], n[hit], np.full((int(hit.sum()), 3), -1.0, np.float32))
            n[hit] = np.where((dn < 0)[:, None], n[hit], flip)
        alb_sum = (alb_sum + alb).astype(np.float32)
        nrm_sum = (nrm_sum + n).astype(np.float32)
        tsum = np.where(hit, (tsum + t).astype(np.float32), tsum).astype(np.float32)
        hits += hit
    f = np.float32(spp)
    pix = q[0]["index"]  # y * W + x of local pixel p
    out = {
        "albedo": (alb_sum / f).astype(np.float32),
        "normal": (nrm_sum / f).astype(np.float32),
        "depth": np.where(hits > 0, (tsum / np.maximum(hits, 1).astype(np.float32)).astype(np.float32), VERY_FAR).astype(np.float32),
        "prim": np.where(q[0]["distance"] < VERY_FAR, q[0]["identifier"], -1).astype(np.int32),
        "geom": np.where(q[0]["distance"] < VERY_FAR, q[0]["geometry_type"], -1).astype(np.int32),
    }
    return pix, out


def first_wavefront(ctx, n):
    ctx.stage("begin")
    ctx.stage("primary")
    ctx.stage("extend")
    return ctx.ray_queue(0, n)


def oracle_queue(orc, sc, nodes, prims, spp, w, h, frame=None, rank=0, nranks=1):
    """an oracle ctx after begin / primary / extend with queue_size = spp * P, and its queue: every sample's first segment in
    ticket order"""
    n = spp * w * (h // nranks)
    o = orc.Oracle(w, h, n, rank=rank, nranks=nranks, flags=flags_of(sc) & 25)
    o.load_scene(sc, nodes, prims)
    if frame is not None:
        o.set_frame(frame)
    return o, first_wavefront(o, n)


def assert_aov_equal(got, pix, want, what):
    for k in ("albedo", "normal", "depth"):
        g = got[k].reshape(got[k].shape[0], -1)[pix]
        w = want[k].reshape(want[k].shape[0], -1)
        assert np.array_equal(bits(g), bits(w)), f"{what} {k}: {np.count_nonzero((bits(g) != bits(w)).any(axis=-1) if g.ndim > 1 else bits(g) != bits(w))} pixels differ"
    for k in ("prim", "geom"):
        assert np.array_equal(got[k][pix], want[k]), f"{what} {k}"


class OracleMath:
    """expected_aov's vector operations from the oracle's glm restatement (the op codes of tyr_vecmath_probe), so that
    it runs without a GPU"""

    def __init__(self, lib):
        self.lib = lib

    def vecmath_probe(self, op, a, b, c):
        import specular_ref

        return specular_ref.glm(self.lib, op, a, b, c)
