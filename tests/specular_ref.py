"""Specular-chain guides (include/tyr_c.h "Specular-chain guides", tyr_render_aov_chain) restated on the oracle, so that the
GPU pass has a specification that is not another HIP kernel.

Every segment of a chain is the oracle's own `extend`: the continued rays go into its queue by mapped_model.py's two-import
idiom (import_work_queue(q, N) copies the records in, import_work_queue(q, 0) puts primary_ray_cnt back to the 0 the primary
stage left; extend traces the n_live = N records the primary stage counted).  Every step between two segments is float32
numpy, one operation per line, with glm's dot / cross / normalize / reflect taken from the oracle's glm restatement
(oracle/orc_glm.c, pinned to the vendored glm by tests/test_glm_pinning.py) -- nothing here needs a GPU.  The per-pixel sums
follow test_aov.expected_aov.  tests/test_specular_guides.py pins the steps to the oracle's own shade on the CPU."""
from __future__ import annotations

import numpy as np

VERY_FAR = np.float32(1e20)
EPSILON = np.float32(0.001)
DIFF, SPEC, REFR, PHONG, LIGHT = 0, 1, 2, 3, 4
F = np.float32


def glm(lib, op, a, b=None, c=None):
    """orc_glm on (n, 3) float32 arrays: 0 dot (in column 0), 1 cross, 2 normalize, 4 reflect(I = a, N = b)"""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
    c = a if c is None else np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3)
    out = np.zeros_like(a)
    if a.shape[0]:
        assert lib.orc_glm(op, a.ctypes.data, b.ctypes.data, c.ctypes.data, a.shape[0], out.ctypes.data) == 0
    return out


def dot(lib, a, b):
    return glm(lib, 0, a, b)[:, 0]


def surface(lib, r, sc, prims, spheres):
    """shade's quantities of the hit records r (distance < VERY_FAR): at, the face-forwarded normal n, outside, at' = at + n *
    EPSILON, the material and the colour"""
    o, d, t = r["origin"].astype(np.float32), r["direction"].astype(np.float32), r["distance"].astype(np.float32)
    m = r.shape[0]
    step = (d * t[:, None]).astype(np.float32)
    at = (o + step).astype(np.float32)
    n = np.zeros((m, 3), np.float32)
    material = np.full(m, DIFF, np.int64)
    colour = np.ones((m, 3), np.float32)
    sph = r["geometry_type"] == 0
    tri = ~sph
    if sph.any():
        sp = spheres[r["identifier"][sph]]
        diff = (at[sph] - sp["position"].astype(np.float32)).astype(np.float32)
        n[sph] = (diff / sp["radius"].astype(np.float32)[:, None]).astype(np.float32)
        material[sph] = sp["refl"]
        colour[sph] = sp["color"]
    if tri.any():
        tr = prims[r["identifier"][tri]]
        cr = glm(lib, 1, tr["e1"], tr["e2"])
        n[tri] = glm(lib, 2, cr)
        if sc.triangle_materials:
            highest = LIGHT if sc.light_list else PHONG
            mt = tr["materialType"].astype(np.int64)
            material[tri] = np.where(mt <= highest, mt, DIFF)
        if sc.triangle_colors:
            colour[tri] = sc.palette_color[tr["pad_"][:, 0]].astype(np.float32)
    outside = dot(lib, n, d) < 0
    flipped = (n * F(-1.0)).astype(np.float32)
    n = np.where(outside[:, None], n, flipped).astype(np.float32)
    lift = (n * EPSILON).astype(np.float32)
    at2 = (at + lift).astype(np.float32)
    return {"at": at, "n": n, "outside": outside, "at2": at2, "material": material, "colour": colour, "d": d, "t": t}


def spec_step(lib, s):
    """SPEC: o = at', d = reflect(d, n)"""
    return s["at2"], glm(lib, 4, s["d"], s["n"])


def refr_step(lib, s):
    """REFR's two candidates and which one the guide takes: (o_reflect, d_reflect), (o_transmit, d_transmit), total internal
    reflection.  The transmit candidate is NaN where sinT2 > 1 (sqrt of a negative), as in shade; the guide never takes it there."""
    n, d, outside = s["n"], s["d"], s["outside"]
    n1 = np.where(outside, F(1.2), F(1.0)).astype(np.float32)
    n2 = np.where(outside, F(1.0), F(1.2)).astype(np.float32)
    ndotd = dot(lib, n, d)
    cosI = (-ndotd).astype(np.float32)
    eta = (n2 / n1).astype(np.float32)
    eta2 = (eta * eta).astype(np.float32)
    cc = (cosI * cosI).astype(np.float32)
    om = (F(1.0) - cc).astype(np.float32)
    sinT2 = (eta2 * om).astype(np.float32)
    tir = sinT2 > F(1.0)
    n2x = (n * F(2.0)).astype(np.float32)
    back = (n2x * EPSILON).astype(np.float32)
    o_t = (s["at2"] - back).astype(np.float32)
    with np.errstate(invalid="ignore"):
        rad = (F(1.0) - sinT2).astype(np.float32)
        cosT = np.sqrt(rad).astype(np.float32)
        ed = (eta[:, None] * d).astype(np.float32)
        ec = (eta * cosI).astype(np.float32)
        k = (ec - cosT).astype(np.float32)
        kn = (k[:, None] * n).astype(np.float32)
        d_t = (ed + kn).astype(np.float32)
    return (s["at2"], glm(lib, 4, d, n)), (o_t, d_t), tir


def trace(oracle, buf, origin, direction):
    """the oracle's extend of the rays (origin, direction): they replace the first records of buf, a full queue of the ctx"""
    m = origin.shape[0]
    assert m <= buf.shape[0] == oracle.N
    buf["origin"][:m] = origin
    buf["direction"][:m] = direction
    oracle.import_work_queue(buf, oracle.N)
    oracle.import_work_queue(buf, 0)
    oracle.stage("extend")
    return oracle.ray_queue(0, m)


def chain_samples(oracle, q, sc, prims, spheres, max_chain):
    """every sample's chain.  oracle: a ctx whose begin / primary / extend made q, its full queue in ticket order (queue_size =
    spp * P: n_live is the queue).  Returns per sample: albedo, normal, depth (of the end surface; `hit` False: the chain left
    the scene), chain, end_prim, end_geom, and `events`, the counts the coverage test reads."""
    lib = oracle.L
    N = q.shape[0]
    assert N == oracle.N
    T = np.ones((N, 3), np.float32)
    L = np.zeros(N, np.float32)
    k = np.zeros(N, np.int32)
    out = {"albedo": np.zeros((N, 3), np.float32), "normal": np.zeros((N, 3), np.float32), "depth": np.zeros(N, np.float32), "hit": np.zeros(N, bool),
           "chain": np.zeros(N, np.int32), "end_prim": np.full(N, -1, np.int32), "end_geom": np.full(N, -1, np.int32)}
    ev = dict.fromkeys(("spec_sphere", "spec_triangle", "refr_enter", "refr_leave_sphere", "tir", "left_after_bounce", "capped", "coloured_mirror"), 0)
    idx = np.arange(N)
    r = q.copy()
    buf = q.copy()
    while idx.size:
        hit = r["distance"] < VERY_FAR
        gone = idx[~hit]  # albedo +0, normal +0, no depth
        out["chain"][gone] = k[gone]
        ev["left_after_bounce"] += int((k[gone] >= 1).sum())
        idx, r = idx[hit], r[hit]
        if not idx.size:
            break
        s = surface(lib, r, sc, prims, spheres)
        L[idx] = (L[idx] + s["t"]).astype(np.float32)
        specular = (s["material"] == SPEC) | (s["material"] == REFR)
        go = specular & (k[idx] < max_chain)
        ev["capped"] += int((specular & ~go).sum())
        e = idx[~go]
        out["albedo"][e] = (T[e] * s["colour"][~go]).astype(np.float32)
        out["normal"][e] = s["n"][~go]
        out["depth"][e] = L[e]
        out["hit"][e] = True
        out["chain"][e] = k[e]
        out["end_prim"][e] = r["identifier"][~go]
        out["end_geom"][e] = r["geometry_type"][~go]
        if not go.any():
            break
        sg = {key: v[go] for key, v in s.items()}
        c, rg = idx[go], r[go]
        mirror = sg["material"] == SPEC
        T[c[mirror]] = (T[c[mirror]] * sg["colour"][mirror]).astype(np.float32)
        o_s, d_s = spec_step(lib, sg)
        (o_r, d_r), (o_t, d_t), tir = refr_step(lib, sg)
        reflect = mirror | tir
        origin = np.where(mirror[:, None], o_s, np.where(tir[:, None], o_r, o_t)).astype(np.float32)
        direction = np.where(reflect[:, None], np.where(mirror[:, None], d_s, d_r), d_t).astype(np.float32)
        ev["spec_sphere"] += int((mirror & (rg["geometry_type"] == 0)).sum())
        ev["spec_triangle"] += int((mirror & (rg["geometry_type"] == 1)).sum())
        ev["coloured_mirror"] += int((mirror & (T[c] != 1).any(axis=1)).sum())
        ev["tir"] += int((~mirror & tir).sum())
        ev["refr_enter"] += int((~mirror & ~tir & sg["outside"]).sum())
        ev["refr_leave_sphere"] += int((~mirror & ~tir & ~sg["outside"] & (rg["geometry_type"] == 0)).sum())
        k[c] += 1
        idx = c
        r = trace(oracle, buf, origin, direction)
    out["events"] = ev
    return out


def expected_chain(oracle, q, sc, prims, spheres, spp, max_chain):
    """(pixel index, dict) of tyr_render_aov_chain's outputs for the queue q of `oracle` (see chain_samples): the sums of
    test_aov.expected_aov over the end-surface values, sample 0's first-hit ids and chain, the first segments' depth"""
    P = q.shape[0] // spp
    first = q.reshape(spp, P)
    c = chain_samples(oracle, q, sc, prims, spheres, max_chain)
    alb, nrm, dep, hit = c["albedo"].reshape(spp, P, 3), c["normal"].reshape(spp, P, 3), c["depth"].reshape(spp, P), c["hit"].reshape(spp, P)
    alb_sum = np.zeros((P, 3), np.float32)
    nrm_sum = np.zeros((P, 3), np.float32)
    tsum = np.zeros(P, np.float32)
    fsum = np.zeros(P, np.float32)
    hits = np.zeros(P, np.int64)
    fhits = np.zeros(P, np.int64)
    for s in range(spp):
        alb_sum = (alb_sum + alb[s]).astype(np.float32)
        nrm_sum = (nrm_sum + nrm[s]).astype(np.float32)
        tsum = np.where(hit[s], (tsum + dep[s]).astype(np.float32), tsum).astype(np.float32)
        hits += hit[s]
        fh = first[s]["distance"] < VERY_FAR
        fsum = np.where(fh, (fsum + first[s]["distance"]).astype(np.float32), fsum).astype(np.float32)
        fhits += fh
    f = np.float32(spp)
    mean = lambda total, cnt: np.where(cnt > 0, (total / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32), VERY_FAR).astype(np.float32)  # noqa: E731
    h0 = first[0]["distance"] < VERY_FAR
    out = {
        "albedo": (alb_sum / f).astype(np.float32),
        "normal": (nrm_sum / f).astype(np.float32),
        "depth": mean(tsum, hits),
        "prim": np.where(h0, first[0]["identifier"], -1).astype(np.int32),
        "geom": np.where(h0, first[0]["geometry_type"], -1).astype(np.int32),
        "chain": c["chain"][:P],
        "end_prim": c["end_prim"][:P],
        "end_geom": c["end_geom"][:P],
        "length0": np.where(hit[0], dep[0], VERY_FAR).astype(np.float32),
        "depth_first": mean(fsum, fhits),
    }
    return first[0]["index"], out, c["events"]
