"""Crafted inputs for the shade kernel (tests/test_shade_branches.py): a scene whose every material can be hit where the
reference allows it, and batches of work-queue records aimed at single branches of kernel.cu:347-627.

A helper module (no tests, no fixtures): everything here is a pure function of its arguments and seeds.

The scene: seven spheres in a row along x (DIFF, SPEC, a faintly absorbing REFR, PHONG, a LIGHT that next-event estimation never
samples, and a large REFR whose colour absorbs a throughput to (0, 0, 0) over a long chord), spheres[6] -- the emitter
next-event estimation samples -- behind a box of 48 outward-facing triangles 300 units away, with a two-sided screen of four triangles in front of it.  The box's 24 quads carry
materialType 0 .. 4 and 7 (out of range) in turn and palette entries 0 .. 23 of differing colour and emission.  Rays start
outside and INSIDE the spheres; triangles are one-sided (loader.h:28 culls back faces: det = -dot(d, e1 x e2) must exceed 1e-7),
so extend never hands shade a triangle seen from behind.
"""
from __future__ import annotations

import functools

import numpy as np

from tyrant_amd import scenes

EPSILON = np.float32(1e-3)
VERY_FAR = np.float32(1e20)
MAX_BOUNCES = 5
FLAG_SETS = (0, 1, 1 | 16, 1 | 8, 1 | 8 | 16)  # TRIANGLE_MATERIALS = 1, LIGHT_LIST = 8, TRIANGLE_COLORS = 16
SIZES = (1, 63, 64, 65, 255, 256, 257, 2049, 16411)  # a tile is 256 slots, a wave 64; 16411 is prime: no segment ends on a wave
BIG = SIZES[-1]
LARGE_FRAME = 4000000007
ZERO_SEED_FRAME = 0x80000000  # times an even pixel: 0 modulo 2^32 -- every seed of the batch is 0 (frame 0 itself is refused by both sides)
CRITICAL_COS = float(np.sqrt(1.0 - 1.0 / 1.44))  # 0.5528: sinT2 = 1.44 (1 - cosI^2) = 1 for a ray leaving the glass (n = 1.2)

# ---- the oracle's trace bits (oracle/orc.h ORC_TR_*) ----------------------------------------------------------------------
TRACE_BITS = ("HIT", "MISS", "SPHERE", "TRIANGLE", "MAT_DIFF", "MAT_SPEC", "MAT_REFR", "MAT_PHONG", "MAT_LIGHT", "OUTSIDE", "INSIDE", "LIGHT_SEEN", "LIGHT_UNSEEN",
              "NEE_SUN_DIFF", "NEE_EMITTER_DIFF", "NEE_SUN_PHONG", "NEE_EMITTER_PHONG", "REJ_SUN_COS", "REJ_COS_SURFACE", "REJ_COS_LIGHT", "REJ_TRIANGLE_BACK", "REJ_LOBE_SUN",
              "REJ_LOBE_EMITTER", "PICK_SPHERE", "PICK_TRIANGLE", "BOUNCES_BELOW_MAX", "BOUNCES_AT_MAX", "TIR", "FRESNEL_REFLECT", "REFRACT", "PHONG_ONE_ROUND", "PHONG_MORE_ROUNDS",
              "SURVIVED", "DIED_P_EPSILON", "DIED_DRAW", "DIED_BOUNCE_CAP", "MISS_SKY", "MISS_SUNSKY", "ABSORB", "ABSORB_TO_ZERO", "MATERIAL_FALLBACK", "PALETTE", "SHADOW_RAY", "P_CLAMPED")
BIT = {name: np.uint64(1) << np.uint64(i) for i, name in enumerate(TRACE_BITS)}
# decided by where the ray comes from and what it meets, not by its random numbers: the sort key of the "sorted" order
# (DIED_P_EPSILON, P_CLAMPED and ABSORB_TO_ZERO also depend on the record's throughput and on this scene's colours -- both fixed
# inputs, no draw enters them; the key is taken from the first iteration's trace, which is the one the order is applied to)
GEOMETRIC = ("HIT", "MISS", "SPHERE", "TRIANGLE", "MAT_DIFF", "MAT_SPEC", "MAT_REFR", "MAT_PHONG", "MAT_LIGHT", "OUTSIDE", "INSIDE", "LIGHT_SEEN", "LIGHT_UNSEEN", "BOUNCES_BELOW_MAX",
             "BOUNCES_AT_MAX", "TIR", "MISS_SKY", "MISS_SUNSKY", "ABSORB", "ABSORB_TO_ZERO", "MATERIAL_FALLBACK", "PALETTE", "DIED_BOUNCE_CAP", "DIED_P_EPSILON", "P_CLAMPED")
# conjunctions worth a count of their own: (name, bits that must all be set)
COMBOS = (("LIGHT_SEEN on a sphere", ("LIGHT_SEEN", "SPHERE")), ("LIGHT_UNSEEN on a sphere", ("LIGHT_UNSEEN", "SPHERE")), ("LIGHT_SEEN on a triangle", ("LIGHT_SEEN", "TRIANGLE")),
          ("LIGHT_UNSEEN on a triangle", ("LIGHT_UNSEEN", "TRIANGLE")), ("DIFF from inside", ("MAT_DIFF", "INSIDE")), ("SPEC from inside", ("MAT_SPEC", "INSIDE")),
          ("PHONG from inside", ("MAT_PHONG", "INSIDE")), ("LIGHT from inside", ("MAT_LIGHT", "INSIDE")), ("REFR from outside", ("MAT_REFR", "OUTSIDE")),
          ("reflected inside the glass by the draw", ("FRESNEL_REFLECT", "INSIDE")), ("refracted out of the glass", ("REFRACT", "INSIDE")),
          ("SPEC triangle", ("MAT_SPEC", "TRIANGLE")), ("REFR triangle", ("MAT_REFR", "TRIANGLE")), ("PHONG triangle", ("MAT_PHONG", "TRIANGLE")),
          ("diffuse hit at the bounce cap", ("MAT_DIFF", "BOUNCES_AT_MAX")), ("roulette on a clamped p", ("P_CLAMPED", "SURVIVED")))
GEOMETRIC_COMBOS = tuple(name for name, bits in COMBOS if all(b in GEOMETRIC for b in bits))


def possible(flags: int):
    """the trace bits and conjunctions a batch can reach under `flags`, and those it cannot, each with the reason"""
    never = {}
    if not flags & 1:
        for k in ("MATERIAL_FALLBACK", "SPEC triangle", "REFR triangle", "PHONG triangle"):
            never[k] = "without TYR_FLAG_TRIANGLE_MATERIALS every triangle is DIFF and materialType is not read (kernel.cu:380-383)"
    if not flags & 8:
        for k in ("PICK_TRIANGLE", "REJ_TRIANGLE_BACK", "LIGHT_SEEN on a triangle", "LIGHT_UNSEEN on a triangle"):
            never[k] = "without TYR_FLAG_LIGHT_LIST no triangle is LIGHT (materialType 4 falls back to DIFF) and spheres[6] is the only emitter sampled"
    if not flags & 16:
        never["PALETTE"] = "without TYR_FLAG_TRIANGLE_COLORS the palette is not read"
    names = list(TRACE_BITS) + [c[0] for c in COMBOS]
    return [n for n in names if n not in never], never


def has(masks: np.ndarray, name: str) -> np.ndarray:
    """records whose mask has trace bit `name`, or all bits of the conjunction `name`"""
    need = np.uint64(0)
    for b in ((name,) if name in BIT else dict(COMBOS)[name]):
        need |= BIT[b]
    return (masks & need) == need


def longest_run(flag: np.ndarray) -> int:
    best = run = 0
    for f in flag.tolist():
        run = run + 1 if f else 0
        best = max(best, run)
    return best


# ---- the scene ------------------------------------------------------------------------------------------------------------
R = 12.0
ABSORBER = 5  # spheres[5]: the large glass ball whose colour kills a throughput over a long chord
BOX_CENTRE = np.array([0.0, 300.0, 0.0])
BOX_HALF = 30.0
TRIANGLE_MATERIALS = (scenes.DIFF, scenes.SPEC, scenes.REFR, scenes.PHONG, scenes.LIGHT, 7)


def spheres() -> np.ndarray:
    s = np.zeros(7, dtype=scenes.SPHERE_DTYPE)
    s[0] = (R, (-120.0, 0.0, 0.0), (0.8, 0.7, 0.6), (0, 0, 0), scenes.DIFF)
    s[1] = (R, (-80.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0, 0, 0), scenes.SPEC)  # white: p of the roulette is the record's own throughput
    s[2] = (R, (-40.0, 0.0, 0.0), (0.05, 0.03, 0.006), (0, 0, 0), scenes.REFR)
    s[3] = (R, (0.0, 0.0, 0.0), (0.6, 0.5, 0.4), (0, 0, 0), scenes.PHONG)
    s[4] = (R, (40.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 1.5, 1.0), scenes.LIGHT)  # a LIGHT that is not spheres[6]
    s[5] = (60.0, (200.0, 0.0, 0.0), (3.0, 2.5, 4.0), (0, 0, 0), scenes.REFR)  # exp(-3 * 120) = 0 in float32
    s[6] = (9.0, (0.0, 420.0, 0.0), (0.0, 1.0, 0.0), (3.0, 3.0, 3.0), scenes.LIGHT)  # behind the box as seen from spheres 2 .. 4
    return s


def box_triangles() -> np.ndarray:
    """the six faces of the cube BOX_CENTRE +- BOX_HALF, outward-facing, each 2 x 2 quads of two triangles, and a screen of two quads: 52 triangles; quad q has
    materialType TRIANGLE_MATERIALS[q % 6] and palette entry q"""
    tris = []
    q = 0
    for axis in range(3):
        for sign in (-1.0, 1.0):
            n = np.zeros(3)
            n[axis] = sign
            a, b = np.zeros(3), np.zeros(3)
            a[(axis + 1) % 3] = 1.0
            b[(axis + 2) % 3] = 1.0
            if np.dot(np.cross(a, b), n) < 0:
                a, b = b, a
            for i in (-1, 0):
                for j in (-1, 0):
                    p0 = BOX_CENTRE + n * BOX_HALF + a * (i * BOX_HALF) + b * (j * BOX_HALF)
                    p1, p2, p3 = p0 + a * BOX_HALF, p0 + a * BOX_HALF + b * BOX_HALF, p0 + b * BOX_HALF
                    t = scenes.make_triangles([p0, p0], [p1, p2], [p2, p3], TRIANGLE_MATERIALS[q % 6])
                    assert np.all(np.cross(t["e1"], t["e2"]) @ n > 0)
                    t["pad_"][:, 0] = q
                    tris.append(t)
                    q += 1
    # a two-sided screen half-way between the spheres and the box: shadow rays from the spheres to the box's emitters meet it
    for y, ny in ((150.0, -1.0), (151.0, 1.0)):
        c = [(-50.0, y, -20.0), (50.0, y, -20.0), (50.0, y, 20.0), (-50.0, y, 20.0)]
        if ny > 0:
            c = c[::-1]
        t = scenes.make_triangles([c[0], c[0]], [c[1], c[2]], [c[2], c[3]], scenes.DIFF)
        assert np.all(np.cross(t["e1"], t["e2"])[:, 1] * ny > 0)
        t["pad_"][:, 0] = q
        tris.append(t)
        q += 1
    return np.concatenate(tris)


def palette():
    col = np.ones((256, 3), dtype=np.float32)
    em = np.full((256, 3), 3.0, dtype=np.float32)
    k = np.arange(26)
    col[:26] = np.stack([0.35 + 0.6 * scenes.hash_unit(k, 11), 0.35 + 0.6 * scenes.hash_unit(k, 12), 0.35 + 0.6 * scenes.hash_unit(k, 13)], axis=1)
    col[1] = 1.0  # a white mirror quad and a white diffuse one: p of the roulette is the record's own throughput there too
    col[6] = 1.0
    em[:26] = np.stack([0.5 + 5.0 * scenes.hash_unit(k, 21), 0.5 + 5.0 * scenes.hash_unit(k, 22), 0.5 + 5.0 * scenes.hash_unit(k, 23)], axis=1)
    return col, em


@functools.lru_cache(maxsize=None)
def scene(flags: int):
    """(SceneData, nodes, prims) for a ctx created with `flags`; the tree is the oracle's builder's"""
    from oracle import pyorc

    col, em = palette() if flags & 16 else (None, None)
    sc = scenes.SceneData("shade_cases", box_triangles(), spheres(), scenes.Camera(position=(0.0, -200.0, 20.0), direction=(0.0, 1.0, 0.0)), triangle_materials=bool(flags & 1),
                          light_list=bool(flags & 8), triangle_emission=(4.0, 3.5, 3.0), triangle_colors=bool(flags & 16), palette_color=col, palette_emission=em)
    nodes, prims = pyorc.bvh_build(sc.triangles, scenes.triangle_bboxes(sc.triangles))
    return sc, nodes, prims


# ---- the rays -------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tangent(n, rng):
    t = np.cross(n, _unit(rng.normal(size=n.shape)))
    return _unit(t)


def _cosines(rng, k):
    """half uniform in (0, 1), a third log-uniform down to 1e-6 (grazing), the rest within 1e-3 of head-on"""
    c = rng.random(k)
    kind = rng.random(k)
    graze = kind < 0.33
    c[graze] = 10.0 ** (-6.0 * rng.random(int(graze.sum())))
    head = kind > 0.9
    c[head] = 1.0 - 1e-3 * rng.random(int(head.sum()))
    return c


def _toward(n, cos, rng):
    """unit directions d with dot(d, n) = -cos: they arrive at a surface of outward normal n from its front"""
    t = _tangent(n, rng)
    return -n * cos[:, None] + t * np.sqrt(np.maximum(1.0 - cos * cos, 0.0))[:, None]


DIRECT_FORMS = ("zero", "below_eps", "eps", "above_eps", "near_eps", "one", "ones", "above_one", "large", "huge", "denormal", "plain", "negative")


def _directs(rng, k, negative_ok):
    """throughputs in the forms of DIRECT_FORMS: finite everywhere; "negative" (one channel below zero) only where asked"""
    eps = np.float32(1e-3)
    d = (0.05 + 0.95 * rng.random((k, 3))).astype(np.float32)
    form = rng.integers(0, len(DIRECT_FORMS) + 6, k)  # the surplus goes to "plain"
    lead = rng.integers(0, 3, k)  # the channel that carries the form's value; the others stay below it
    rows = np.arange(k)

    def put(sel, value, others):
        d[sel] = (d[sel] * np.float32(others)).astype(np.float32)
        d[rows[sel], lead[sel]] = value

    put(form == 1, np.nextafter(eps, np.float32(0)), 1e-3)
    put(form == 2, eps, 1e-3)
    put(form == 3, np.nextafter(eps, np.float32(1)), 1e-3)
    near = form == 4
    put(near, 0.0, 1e-3)
    d[rows[near], lead[near]] = (eps * (1.0 + 2e-3 * (rng.random(int(near.sum())) - 0.5))).astype(np.float32)
    put(form == 5, np.float32(1.0), 0.9)
    d[form == 6] = 1.0
    put(form == 7, np.nextafter(np.float32(1), np.float32(2)), 0.9)
    put(form == 8, np.float32(2.5), 1.5)
    put(form == 9, np.float32(1e30), 1.0)
    put(form == 10, np.float32(1e-42), 0.0)
    d[form == 0] = 0.0
    neg = form == 12
    if negative_ok:
        d[rows[neg], lead[neg]] = -d[rows[neg], lead[neg]]
    return d


@functools.lru_cache(maxsize=None)
def sun_direction():
    from oracle import pyorc

    return np.array(pyorc.sun_setup().sunDirection[:], dtype=np.float64)


PHONG_SAFE_COS = 0.05


def make_rays(n: int, seed: int, negative_ok: bool, all_safe: bool = False):
    """n work-queue records (no pixel yet): what each is aimed at is drawn per record, so every size holds every kind.
    Also returns `risky`: records aimed at a PHONG surface at a cosine below PHONG_SAFE_COS, which must not meet a zero seed
    (module docstring of tests/test_shade_branches.py, "The Phong loop with seed 0"); all_safe leaves none"""
    rng = np.random.default_rng(seed)
    sp = spheres()
    tris = box_triangles()
    r = np.zeros(n, dtype=scenes.RAY_DTYPE)
    kind = rng.choice(5, n, p=(0.24, 0.38, 0.26, 0.08, 0.04))  # sphere from outside / from inside, triangle, miss, miss toward the sun
    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    d[:, 2] = 1.0

    out = np.nonzero(kind == 0)[0]
    which = rng.choice(7, len(out), p=(0.09, 0.09, 0.12, 0.3, 0.1, 0.14, 0.16))
    nrm = _unit(rng.normal(size=(len(out), 3)))
    p = sp["position"][which].astype(np.float64) + nrm * sp["radius"][which, None]
    risky = np.zeros(n, dtype=bool)
    cos = _cosines(rng, len(out))
    risky[out] = (which == 3) & (cos < PHONG_SAFE_COS)
    if all_safe:
        cos[risky[out]] = PHONG_SAFE_COS + 0.9 * rng.random(int(risky[out].sum()))
    d[out] = _toward(nrm, cos, rng)
    o[out] = p - d[out] * rng.uniform(2.0, 12.0, len(out))[:, None]

    ins = np.nonzero(kind == 1)[0]
    which = rng.choice(7, len(ins), p=(0.09, 0.07, 0.25, 0.23, 0.05, 0.26, 0.05))
    nrm = _unit(rng.normal(size=(len(ins), 3)))
    cos = _cosines(rng, len(ins))
    glass = (which == 2) | (which == ABSORBER)
    at_edge = glass & (rng.random(len(ins)) < 0.75)  # either side of the critical angle: within 0.05, within 1e-5, within 2e-7
    width = rng.choice([0.05, 1e-5, 2e-7], len(ins))
    cos[at_edge] = CRITICAL_COS + (width * rng.uniform(-0.5, 1.0, len(ins)))[at_edge]
    long_path = (which == ABSORBER) & ~at_edge  # long chords through the absorbing glass: the throughput underflows to zero
    cos[long_path] = 1.0 - 0.3 * rng.random(int(long_path.sum()))
    risky[ins] = (which == 3) & (cos < PHONG_SAFE_COS)
    if all_safe:
        cos[risky[ins]] = PHONG_SAFE_COS + 0.9 * rng.random(int(risky[ins].sum()))
    p = sp["position"][which].astype(np.float64) + nrm * sp["radius"][which, None]
    d[ins] = -_toward(nrm, cos, rng)  # dot(d, n) = +cos: the surface is met from inside
    chord = 2.0 * sp["radius"][which] * cos
    back = chord * np.where(long_path, rng.uniform(0.6, 0.95, len(ins)), rng.uniform(0.05, 0.95, len(ins)))
    o[ins] = p - d[ins] * back[:, None]

    tri = np.nonzero(kind == 2)[0]
    which = rng.integers(0, len(tris), len(tri))
    w = rng.dirichlet((1.0, 1.0, 1.0), len(tri)) * 0.94 + 0.02
    e1, e2 = tris["e1"][which].astype(np.float64), tris["e2"][which].astype(np.float64)
    p = tris["vert"][which].astype(np.float64) + e1 * w[:, 1:2] + e2 * w[:, 2:3]
    cos = _cosines(rng, len(tri))
    risky[tri] = (tris["materialType"][which] == scenes.PHONG) & (cos < PHONG_SAFE_COS)
    if all_safe:
        cos[risky[tri]] = PHONG_SAFE_COS + 0.9 * rng.random(int(risky[tri].sum()))
    d[tri] = _toward(_unit(np.cross(e1, e2)), cos, rng)
    o[tri] = p - d[tri] * rng.uniform(5.0, 40.0, len(tri))[:, None]

    miss = np.nonzero(kind == 3)[0]
    o[miss] = np.array([0.0, 150.0, 120.0]) + rng.uniform(-100.0, 100.0, (len(miss), 3))
    up = _unit(rng.normal(size=(len(miss), 3)))
    up[:, 2] = np.abs(up[:, 2]) + 0.3
    d[miss] = _unit(up)

    sun = np.nonzero(kind == 4)[0]
    o[sun] = np.array([0.0, 150.0, 120.0]) + rng.uniform(-100.0, 100.0, (len(sun), 3))
    spread = rng.choice([0.0, 1e-4, 3e-3, 2e-2], len(sun))  # the sun's disc is about 1e-2 wide: on its axis, inside, at its edge, just outside
    d[sun] = _unit(sun_direction() + spread[:, None] * rng.normal(size=(len(sun), 3)))

    r["origin"] = o.astype(np.float32)
    d32 = d.astype(np.float32)
    r["direction"] = (d32 / np.linalg.norm(d32.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    r["direct"] = _directs(rng, n, negative_ok)
    r["distance"] = VERY_FAR
    r["bounces"] = rng.choice([0, 4, 5], n, p=(0.55, 0.2, 0.25))
    r["lastSpecular"] = rng.random(n) < 0.5
    r["geometry_type"] = 1
    return r, (np.zeros_like(risky) if all_safe else risky)


def seeds(rays: np.ndarray, frame: int) -> np.ndarray:
    """kernel.cu:363: the seed of the record in slot i"""
    m = np.uint64(0xFFFFFFFF)
    a = (np.uint64(frame) * rays["index"].astype(np.uint64)) & m
    a = (a * np.uint64(147565741)) & m
    a = (a * np.uint64(720898027)) & m
    return (a * np.arange(len(rays), dtype=np.uint64)) & m


def frame_size(n: int, layout: str, frame: int = 1):
    """(W, H) of the ctx for a batch of n records (twice the pixels where only the even ones are used)"""
    if layout == "piled":
        return 64, 4
    if frame == ZERO_SEED_FRAME:
        n *= 2
    return (max(n, 64), 1) if n <= 512 else (64, (n + 63) // 64 + 1)


def assign_pixels(r: np.ndarray, layout: str, seed: int, frame: int = 1):
    """"one": one record per pixel, pixel 0 and the last pixel among them; "piled": all records on five pixels"""
    n = len(r)
    W, H = frame_size(n, layout, frame)
    even_only = frame == ZERO_SEED_FRAME
    rng = np.random.default_rng(seed + 17)
    if layout == "piled":
        r["index"] = rng.choice(np.array([0, 1, 100, W * H - 2, W * H - 1]), n)
        return
    pix = np.arange(0, W * H, 2) if even_only else np.arange(W * H)
    pick = rng.permutation(len(pix) - 2)[: max(n - 2, 0)] + 1
    chosen = np.concatenate([[0, len(pix) - 1], pick])[:n] if n > 1 else np.array([0])
    r["index"] = pix[rng.permutation(chosen)]


# ---- the oracle on a batch ------------------------------------------------------------------------------------------------
def new_oracle(flags, n, layout, frame=1):
    from oracle import pyorc

    sc, nodes, prims = scene(flags)
    W, H = frame_size(n, layout, frame)
    o = pyorc.Oracle(W, H, n, flags=flags)
    o.load_scene(sc, nodes, prims)
    return o


def load(r, flags):
    sc, nodes, prims = scene(flags)
    r.load_scene(sc, nodes, prims)
    return r


def staged_iteration(r, first, rays=None, frame=None, trace=False):
    """one iteration stage by stage on an oracle or a Renderer; the first one imports `rays` at `frame`.  Returns what shade and
    connect left behind"""
    r.stage("begin")
    if first:
        n = len(rays)
        r.set_frame(frame)
        r.import_work_queue(rays, n)
        r.set_budget(0)
    r.stage("primary")  # budget 0: no camera rays, n_live = the records in the queue
    r.stage("extend")
    live = r.counters()["n_live"]
    out = dict(n_live=live, extended=r.ray_queue(0, live))
    r.stage("shade")
    k = r.counters()
    out.update(ns=k["primary_ray_cnt"], nh=k["shadow_ray_cnt"], n_survive=k["n_survive"], total_shadow_rays=k["total_shadow_rays"], device_error=k.get("device_error", 0))
    out["survivors"], out["shadows"] = r.ray_queue(1, out["ns"]), r.shadow_queue(out["nh"])
    out["accum_shade"] = r.blit_buffer()
    if trace:
        out["trace"] = r.shade_trace(live)
    if hasattr(r, "queue_rank_check"):
        out["rank_check"] = r.queue_rank_check(1)
    r.stage("connect")
    out["visible"], out["accum"] = r.counters()["n_shadow_visible"], r.blit_buffer()
    r.stage("end")
    return out


@functools.lru_cache(maxsize=None)
def batch(flags: int, n: int, layout: str, order: str, frame: int = 1):
    """the records of one batch in their final order, and the oracle's two staged iterations over them with the trace on.
    "shuffled": as drawn (every wave holds every kind); "sorted": by the geometric part of the shuffled batch's trace, so that
    whole waves and tiles go one way"""
    seed = 1000 * n + (1 if layout == "piled" else 0)
    rays, risky = make_rays(n, seed, negative_ok=layout == "one", all_safe=frame == ZERO_SEED_FRAME or n < 16)  # (a batch too small to hold a partner for the trade below)
    assign_pixels(rays, layout, seed, frame)
    if order == "sorted":
        masks = batch(flags, n, layout, "shuffled", frame)["iterations"][0]["trace"]
        key = np.uint64(0)
        for b in GEOMETRIC:
            key |= BIT[b]
        perm = np.argsort(masks & key, kind="stable")
        rays, risky = rays[perm], risky[perm]
    # no risky record on a zero seed: it trades places (origin and direction only) with a record that is neither
    zero = seeds(rays, frame) == 0
    bad, good = np.nonzero(zero & risky)[0], np.nonzero(~zero & ~risky)[0]
    assert len(bad) <= len(good)
    for f in ("origin", "direction"):
        rays[f][bad], rays[f][good[: len(bad)]] = rays[f][good[: len(bad)]].copy(), rays[f][bad].copy()
    assert np.isfinite(rays["origin"]).all() and np.isfinite(rays["direction"]).all() and np.isfinite(rays["direct"]).all()
    o = new_oracle(flags, n, layout, frame)
    o.set_shade_trace(True)
    its = [staged_iteration(o, True, rays, frame, trace=True), staged_iteration(o, False, trace=True)]
    o.close()
    W, H = frame_size(n, layout, frame)
    return dict(rays=rays, iterations=its, W=W, H=H)


# ---- the render loop on a batch ---------------------------------------------------------------------------------------------
LAUNCHES = 3  # the bounded drive: imported records of bounces 0 still have survivors after it, so the exported queue is not empty
RENDER_FIELDS = ("total_extend_rays", "total_shadow_rays", "n_survive", "n_shadow_visible")


def prime(r):
    """a fresh ctx's first iteration finds the camera moved and resets the accumulation and, with it, the work queue
    (kernel.cu:702-718): spend it on an empty iteration, so that the records imported next stay"""
    assert r.render(0, 1) == 1


def drive(r, rays, frame, how):
    """import `rays` at `frame` into a primed oracle or Renderer with no budget and run them through the render loop:
    "render": render(0), unbounded, to completion; "launches": LAUNCHES times launch_kernels, then the work queue.  The
    counters are this drive's own share (a ctx may be driven again and again)"""
    r.reset_accum()
    k0 = r.counters()
    r.set_frame(frame)
    r.import_work_queue(rays, len(rays))
    r.set_budget(0)
    if how == "render":
        it = r.render(0)
    else:
        for _ in range(LAUNCHES):
            r.launch_kernels()
        it = LAUNCHES
    k = r.counters()
    out = dict(iterations=it, accum=r.blit_buffer(), device_error=k.get("device_error", 0), left=k["primary_ray_cnt"], frame=k["frame"])
    out.update({f: k[f] - k0[f] for f in RENDER_FIELDS})
    if how == "launches":
        out["queue"] = r.ray_queue(0, out["left"])
    return out


@functools.lru_cache(maxsize=None)
def driven(flags: int, n: int, layout: str, order: str, frame: int = 1):
    """the oracle's two drives of batch(...), and `addends`: an upper bound, per pixel, of the terms its accumulation receives in
    the unbounded drive (one per shaded record, one per shadow ray)"""
    b = batch(flags, n, layout, order, frame)
    out = {}
    for how in ("render", "launches"):
        o = new_oracle(flags, n, layout, frame)
        prime(o)
        out[how] = drive(o, b["rays"], frame, how)
        o.close()
    o = new_oracle(flags, n, layout, frame)
    prime(o)
    o.set_frame(frame)
    o.import_work_queue(b["rays"], n)
    o.set_budget(0)
    addends = np.zeros(b["W"] * b["H"], dtype=np.int64)
    for _ in range(out["render"]["iterations"]):
        live = o.counters()["primary_ray_cnt"]
        np.add.at(addends, o.ray_queue(0, live)["index"], 1)
        o.launch_kernels()
        np.add.at(addends, o.shadow_queue(o.counters()["shadow_ray_cnt"])["buffer_index"], 1)
    assert o.counters()["primary_ray_cnt"] == 0 and np.array_equal(o.blit_buffer().view(np.uint32), out["render"]["accum"].view(np.uint32))
    o.close()
    out["addends"] = addends
    return out


# ---- what the HIP-only paths of the render loop will meet, from the oracle's own queues -------------------------------------
def _slab_miss(o, d, lo, hi, tmax, margin):
    """rays (float64) that miss the box [lo - margin, hi + margin] within (0, tmax + margin)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t0, t1 = (lo - margin - o) * inv, (hi + margin - o) * inv
    near, far = np.fmin(t0, t1), np.fmax(t0, t1)
    parallel = d == 0
    outside = parallel & ((o < lo - margin) | (o > hi + margin))
    near = np.where(parallel, -np.inf, near)
    far = np.where(parallel, np.inf, far)
    enter, leave = np.maximum(near.max(axis=1), 0.0), np.minimum(far.min(axis=1), tmax + margin)
    return outside.any(axis=1) | (enter > leave)


def folded_path_counts(flags: int, it: dict):
    """counts of the records the render loop's folded paths act on, after one shade of the oracle (module docstring of
    tests/test_shade_branches.py): ghost candidates, shadow rays blocked by a sphere, visible ones clear of the root box, ones
    blocked by a triangle.  "Clearly" = by 1e-2 units in float64 (the scene is O(100) units: float32 resolves 1e-5 there)"""
    import ctypes as C

    from oracle import pyorc

    import layered_scenes as ls

    sc, nodes, prims = scene(flags)
    lo, hi = nodes[0]["bounds"][0].astype(np.float64), nodes[0]["bounds"][1].astype(np.float64)
    sp = np.ascontiguousarray(sc.spheres)
    margin = 1e-2

    def clear_of_spheres(o, d):
        ok = np.ones(len(o), dtype=bool)
        for s in sp:
            op = s["position"].astype(np.float64) - o
            b = np.einsum("ij,ij->i", op, d)
            disc = b * b - np.einsum("ij,ij->i", op, op) + (float(s["radius"]) + margin) ** 2
            true = b * b - np.einsum("ij,ij->i", op, op) + float(s["radius"]) ** 2
            ok &= (disc < 0) | ((true > 0) & (b + np.sqrt(np.maximum(true, 0.0)) < 0.5e-3))  # no root even of the grown sphere, or the far root below half of epsilon
        return ok

    sv, sh = it["survivors"], it["shadows"]
    so, sd = sv["origin"].astype(np.float64), sv["direction"].astype(np.float64)
    ghosts = _slab_miss(so, sd, lo, hi, 1e20, margin) & clear_of_spheres(so, sd)
    ho, hd, hc = np.ascontiguousarray(sh["origin"]), np.ascontiguousarray(sh["direction"]), sh["closestDistance"]
    by_triangle = ls.tree_any(pyorc, nodes, prims, ho, hd, hc) if len(sh) else np.zeros(0, dtype=bool)
    f = pyorc.lib().orc_sphere_intersect
    fp = C.POINTER(C.c_float)
    by_sphere = np.zeros(len(sh), dtype=bool)
    for i in range(len(sh)):
        po, pd = ho[i].ctypes.data_as(fp), hd[i].ctypes.data_as(fp)
        for k in range(7):
            t = np.float32(f(sp[k : k + 1].ctypes.data, po, pd))
            if t != 0 and np.float32(t + EPSILON) < hc[i]:
                by_sphere[i] = True
                break
    visible = ~by_triangle & ~by_sphere
    clear = _slab_miss(ho.astype(np.float64), hd.astype(np.float64), lo, hi, np.minimum(hc.astype(np.float64), 1e20), margin)
    return dict(ghost_candidates=int(ghosts.sum()), blocked_by_sphere=int((by_sphere & ~by_triangle).sum()), sphere_in_the_way=int(by_sphere.sum()),
                visible_clear_of_root=int((visible & clear).sum()), blocked_by_triangle=int(by_triangle.sum()), visible=int(visible.sum()))
