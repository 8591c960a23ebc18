"""Argument sets and the comparison rule of the numeric contract's tests: shared by
tests/test_oracle_math.py (the oracle against numpy's binary64 libm, and a contracted build of the oracle against the
contract's build) and tests/test_numeric_contract.py (hip/detmath.hpp and the samplers on the device against the oracle).

Every set is seeded, built once per process and handed out read-only.
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
TWO20 = F32(1048576.0)


def _ro(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _f32(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(F32)


def _around(v) -> np.ndarray:
    """the float32 values nearest `v` (binary64) and both their neighbours"""
    c = np.asarray(v, dtype=np.float64).astype(F32)
    return np.concatenate([np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))])


def _binade_edges(e_lo: int, e_hi: int, per_binade: int, rng) -> np.ndarray:
    """positive float32 values of the biased exponents e_lo..e_hi (0 = denormals): the first and last two of every binade
    plus `per_binade` seeded mantissas"""
    e = np.arange(e_lo, e_hi + 1, dtype=np.uint32)[:, None] << np.uint32(23)
    edge = np.array([0, 1, 0x7FFFFE, 0x7FFFFF], dtype=np.uint32)[None, :]
    mant = rng.integers(0, 1 << 23, size=(e.shape[0], per_binade), dtype=np.uint32)
    x = _f32(np.concatenate([e | edge, e | mant], axis=1).ravel())
    return x[x != 0]  # (exponent 0, mantissa 0) is zero: among the specials


SPECIALS = _ro(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, TWO20, -TWO20, np.nextafter(TWO20, F32(0)), -np.nextafter(TWO20, F32(0)),
                         np.nextafter(TWO20, F32(np.inf)), 2.0 ** -149, -(2.0 ** -149), 1e30, -1e30, np.finfo(F32).max], dtype=F32))


@functools.lru_cache(maxsize=None)
def sincos_args() -> np.ndarray:
    """sin / cos: the contract's domain |x| < 2^20 and its edge (about 2.9 M arguments)"""
    rng = np.random.default_rng(20)
    uniform = rng.uniform(-2.0 ** 20, 2.0 ** 20, 1 << 19).astype(F32)
    logu = (np.exp2(rng.uniform(-30, 20, 1 << 18)) * rng.choice([-1.0, 1.0], 1 << 18)).astype(F32)
    k = np.arange(0, int(2.0 ** 20 / (np.pi / 2)) + 2, dtype=np.float64)  # the last two lie past 2^20: sin = cos = 0 there
    kpio2 = _around(k * (np.pi / 2))
    binades = _binade_edges(0, 127 + 19, 64, rng)
    return _ro(np.concatenate([uniform, logu, kpio2, -kpio2[::8], binades, -binades, SPECIALS]))


EXP_THRESHOLDS = (-104.5, -104.0, -103.98, -103.28, -87.34, -87.33654, 0.0, 88.72, 88.72284, 88.73, 89.0, 89.5)


@functools.lru_cache(maxsize=None)
def exp_args() -> np.ndarray:
    """exp: [-104.5, 89.5] (0 below -104, denormal results up to -87.34, inf above 88.72 by rounding and above 89 by the
    guard), the path's exp(-20 u), tiny arguments, and every threshold with its neighbours"""
    rng = np.random.default_rng(21)
    x = np.concatenate([rng.uniform(-104.5, 89.5, 1 << 20), -20.0 * rng.uniform(0, 1, 1 << 17), rng.uniform(-1e-3, 1e-3, 1 << 12)]).astype(F32)
    edges = _around(np.array(EXP_THRESHOLDS))
    edges = np.concatenate([edges, np.nextafter(edges, F32(-np.inf)), np.nextafter(edges, F32(np.inf))])
    small = _binade_edges(1, 126, 4, rng)  # exp(+-tiny) rounds to 1 or its neighbours
    return _ro(np.concatenate([x, edges, small, -small, SPECIALS]))


POW_PATH_EXPONENTS = (F32(1.0) / F32(41.0), F32(40.0), F32(1.0) / F32(2.2))


@functools.lru_cache(maxsize=None)
def pow_args() -> tuple[np.ndarray, np.ndarray]:
    """pow: x over every positive binade (denormals included) with y in [-3, 3], the path's three exponents on (0, 1)
    and on every binade, and the special cases of powf_det's guards"""
    rng = np.random.default_rng(22)
    n = 1 << 19
    wide = _f32((rng.integers(0, 255, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32))
    xs, ys = [wide], [rng.uniform(-3, 3, n).astype(F32)]
    edges = _binade_edges(0, 254, 16, rng)
    xs.append(edges)
    ys.append(rng.uniform(-3, 3, edges.shape[0]).astype(F32))
    for y in POW_PATH_EXPONENTS:
        u = rng.uniform(0, 1, 1 << 17).astype(F32)
        for x in (u, edges):
            xs.append(x)
            ys.append(np.full(x.shape[0], y, dtype=F32))
    sx = np.array([0.0, -0.0, np.inf, np.nan, -1.0, -np.inf, 1.0, 2.0 ** -149, np.finfo(F32).max, np.nextafter(F32(1), F32(2)), 0.5, 2.0], dtype=F32)
    sy = np.array([0.0, -0.0, 0.5, -0.5, np.nan, 1.0, -1.0, 3.0, -3.0, 40.0, 126.0, -126.0, 128.0, 129.0, 130.0, -149.0, -150.0, -152.0, -153.0, np.finfo(F32).max], dtype=F32)
    gx, gy = np.meshgrid(sx, sy, indexing="ij")
    xs.append(gx.ravel())
    ys.append(gy.ravel())
    return _ro(np.concatenate(xs)), _ro(np.concatenate(ys))


# ---- sampler inputs (three 32-bit words per element) ---------------------------------------------------------------

def _xorshift(s: np.ndarray) -> np.ndarray:
    s = s.astype(np.uint32)
    s = s ^ (s << np.uint32(13))
    s = s ^ (s >> np.uint32(17))
    return s ^ (s << np.uint32(5))


def _seed_before(draw: np.ndarray) -> np.ndarray:
    """the seed whose next xorshift draw is `draw` (each of the three steps x ^= x << k or x >> k undone by its series)"""
    s = draw.astype(np.uint32)
    for shift, left in ((5, True), (17, False), (13, True)):
        k = shift
        while k < 32:
            s = s ^ ((s << np.uint32(k)) if left else (s >> np.uint32(k)))
            k *= 2
    return s


@functools.lru_cache(maxsize=None)
def rng_seeds() -> np.ndarray:
    """2^20 seeded seeds, seed 0 (a fixed point: camera_seed can produce it), and the 128 seeds whose first draw is
    >= 0xFFFFFF80: there (float)draw is 2^32, rng_float is 1.0 and rng_int_0_max(s, 16) is 16"""
    rng = np.random.default_rng(23)
    top = _seed_before(np.arange(0xFFFFFF80, 0x100000000, dtype=np.uint64).astype(np.uint32))
    assert np.array_equal(_xorshift(top), np.arange(0xFFFFFF80, 0x100000000, dtype=np.uint64).astype(np.uint32))
    below = _seed_before(np.arange(0xFFFFFF70, 0xFFFFFF80, dtype=np.uint32))  # the draws just under the edge
    s = np.concatenate([rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32), np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32), top, below])
    w = np.zeros((s.shape[0], 3), dtype=np.uint32)
    w[:, 0] = s
    return _ro(w)


N_TOP_SEEDS = 128  # rng_seeds()[-(N_TOP_SEEDS + 16):-16] are the seeds at the edge


@functools.lru_cache(maxsize=None)
def disk_inputs() -> np.ndarray:
    """(ux, uy, 0): a seeded unit square and the branch edges of the concentric map"""
    rng = np.random.default_rng(24)
    sq = rng.uniform(0, 1, (1 << 18, 2)).astype(F32)
    t = (rng.integers(0, 1 << 12, 1 << 12).astype(np.float64) / (1 << 12)).astype(F32)  # dyadic: 2t - 1 and 1 - t are exact
    diag = np.concatenate([np.stack([t, t], 1), np.stack([t, F32(1) - t], 1)])  # |ox| == |oy|, equal and opposite signs
    v = rng.uniform(0, 1, 1 << 10).astype(F32)
    half = np.concatenate([np.stack([np.full_like(v, 0.5), v], 1), np.stack([v, np.full_like(v, 0.5)], 1)])  # one offset exactly 0
    e = np.array([0.0, 2.0 ** -24, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24, 1.0], dtype=F32)
    grid = np.stack(np.meshgrid(e, e, indexing="ij"), -1).reshape(-1, 2)
    uv = np.concatenate([sq, diag, half, grid])
    return _ro(np.concatenate([uv, np.zeros((uv.shape[0], 1), dtype=F32)], axis=1))


BASIS_EDGE_X = tuple(s * v for v in (F32(0.9), np.nextafter(F32(0.9), F32(1)), np.nextafter(F32(0.9), F32(0))) for s in (F32(1), F32(-1)))


@functools.lru_cache(maxsize=None)
def basis_inputs() -> np.ndarray:
    """w: seeded unit vectors, the binary64 compare |w.x| > .9 at 0.9f and its neighbours, the axes, and w = 0 (NaNs)"""
    rng = np.random.default_rng(25)
    g = rng.normal(size=(1 << 18, 3))
    unit = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F32)
    phi = rng.uniform(0, 2 * np.pi, 64)
    edge = []
    for wx in BASIS_EDGE_X:
        rest = np.sqrt(1.0 - float(wx) ** 2)
        edge.append(np.stack([np.full(64, wx, dtype=F32), (rest * np.cos(phi)).astype(F32), (rest * np.sin(phi)).astype(F32)], 1))
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(F32)
    return _ro(np.concatenate([unit] + edge + [axes, np.zeros((1, 3), dtype=F32)]))


# ---- the comparison rule -------------------------------------------------------------------------------------------

def differing(got: np.ndarray, want: np.ndarray, integers: bool = False) -> np.ndarray:
    """mask of the elements that differ.  `got` and `want` are bit patterns (uint32 of binary32, uint64 of binary64): finite
    values, zeros with their sign and infinities compare by bits; NaNs compare by class only (an invalid operation's NaN has
    one sign on x86 and may have the other on the GPU).  integers=True: seeds, quadrants and counts, compared as they are."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.dtype in (np.uint32, np.uint64)
    diff = got != want
    if not integers:
        fl = np.float32 if got.dtype == np.uint32 else np.float64
        diff &= ~(np.isnan(got.view(fl)) & np.isnan(want.view(fl)))
    return diff


INTEGER_FIELDS = ("q",)


def count_differing(got: dict, want: dict) -> dict:
    """{field: number of differing elements} of two {field: bit patterns} dicts (oracle.pyorc.dm_map's layout)"""
    assert got.keys() == want.keys()
    return {k: int(differing(got[k], want[k], integers=k in INTEGER_FIELDS).sum()) for k in want}


def first_differing(got: dict, want: dict, args, limit: int = 4) -> str:
    """a readable account of the first differences, for assertion messages"""
    lines = []
    for k in want:
        idx = np.flatnonzero(differing(got[k], want[k], integers=k in INTEGER_FIELDS))
        for i in idx[:limit]:
            at = ", ".join(f"{float(a[i])!r}" for a in args)
            lines.append(f"{k}[{i}] at ({at}): got {int(got[k][i]):#x}, want {int(want[k][i]):#x}")
        if idx.size:
            lines.append(f"{k}: {idx.size} of {want[k].shape[0]} differ")
    return "\n".join(lines)


# ---- the device's side: probe ops 32-43 in oracle.pyorc.dm_map's layout ------------------------------------------------
# field -> (op, column); column 0 is the 32-bit word, column 64 the binary64 value in words 1 and 2 (low word first)
DEVICE_FIELDS = {
    "sin": {"f32": (32, 0), "r": (32, 64), "q": (33, 0), "rounded": (33, 64)},
    "cos": {"f32": (34, 0), "r": (34, 64), "q": (35, 0), "rounded": (35, 64)},
    "sincos": {"sin": (36, 0), "cos": (36, 1)},
    "exp": {"f32": (37, 0), "kd": (37, 64), "r": (38, 64), "rounded": (39, 64)},
    "pow": {"f32": (40, 0), "log2": (40, 64), "t": (41, 64), "w": (42, 64), "rounded": (43, 64)},
}


def device_dm_map(hip, fn: str, x, y=None) -> dict:
    a = np.zeros((x.shape[0], 3), dtype=F32)
    a[:, 0] = x
    b = a
    if y is not None:
        b = np.zeros_like(a)
        b[:, 0] = y
    words, out = {}, {}
    for name, (op, col) in DEVICE_FIELDS[fn].items():
        if op not in words:
            words[op] = hip.contract_probe(op, a, b)
        w = words[op]
        out[name] = (w[:, 1].astype(np.uint64) | (w[:, 2].astype(np.uint64) << np.uint64(32))) if col == 64 else w[:, col].copy()
    return out
