"""Accuracy of the deterministic transcendental layer (oracle/orc_internal.h; the HIP kernels
implement the same contract in hip/detmath.hpp) against numpy's float64 libm.  CPU only.

The bound is DESIGN.md section 2 item 2's own: 0.5001 ulp of binary32 for normal results, 0.5001 denormal steps (2^-149) for
results below 2^-126.  The *_full_domain tests hold it over the contract's whole domain (the argument sets of
tests/contract_args.py, which the device's tests reuse); the measured maxima are in their docstrings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contract_args as ca

ULP_BOUND = 0.5001
DENORMAL_STEP = 2.0 ** -149
MIN_NORMAL = 2.0 ** -126


def _ulp_err(got: np.ndarray, exact: np.ndarray) -> np.ndarray:
    """error of float32 `got` in units of the float32 spacing at `exact`"""
    ex32 = exact.astype(np.float32)
    with np.errstate(over="ignore"):
        spacing = np.spacing(np.abs(ex32)).astype(np.float64)
    spacing = np.where(spacing == 0, np.finfo(np.float32).tiny, spacing)
    spacing = np.where(np.isinf(spacing) & np.isfinite(ex32), 2.0 ** 104, spacing)  # at FLT_MAX itself
    return np.abs(got.astype(np.float64) - exact) / spacing


def _map1(fn, x):
    return np.array([fn(C.c_float(float(v))) for v in x], dtype=np.float32)


def test_sin_cos(orc):
    L = orc.lib()
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-8, 8, 20000), rng.uniform(-0.01, 0.01, 2000), np.linspace(0, 2 * np.pi, 4097)]).astype(np.float32)
    xd = x.astype(np.float64)
    assert _ulp_err(_map1(L.orc_dm_sinf, x), np.sin(xd)).max() <= 0.5001 + 1e-3 * 0  # essentially correctly rounded
    assert _ulp_err(_map1(L.orc_dm_cosf, x), np.cos(xd)).max() <= 0.5001
    # exact symmetries of the kernel
    assert L.orc_dm_sinf(0.0) == 0.0 and L.orc_dm_cosf(0.0) == 1.0
    assert np.isnan(L.orc_dm_sinf(float("inf"))) and np.isnan(L.orc_dm_cosf(float("nan")))


def test_exp(orc):
    L = orc.lib()
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-100, 10, 20000), rng.uniform(-1e-3, 1e-3, 2000), [-87.5, -95.0, -103.0, 88.0, 0.0]]).astype(np.float32)
    got = _map1(L.orc_dm_expf, x)
    exact = np.exp(x.astype(np.float64))
    normal = exact >= MIN_NORMAL
    assert _ulp_err(got[normal], exact[normal]).max() <= 0.5001
    # denormal results: within 0.5001 denormal steps
    assert np.all(np.abs(got[~normal].astype(np.float64) - exact[~normal]) <= ULP_BOUND * DENORMAL_STEP)
    assert L.orc_dm_expf(-1000.0) == 0.0 and L.orc_dm_expf(1000.0) == float("inf") and L.orc_dm_expf(0.0) == 1.0
    assert L.orc_dm_expf(float("-inf")) == 0.0 and np.isnan(L.orc_dm_expf(float("nan")))


def test_pow(orc):
    L = orc.lib()
    rng = np.random.default_rng(2)
    # the three uses on the path: pow(1 - r2, 1/41) and pow(c, 40) (kernel.cu:527, 554), pow(x, 1/2.2) (kernel.cu:661)
    for xs, y in (
        (rng.uniform(0, 1, 20000), np.float32(1.0) / np.float32(41.0)),
        (rng.uniform(1e-3, 1, 20000), np.float32(40.0)),
        (rng.uniform(0, 1, 20000), np.float32(1.0) / np.float32(2.2)),
        (rng.uniform(0, 50, 5000), np.float32(2.5)),
    ):
        x = xs.astype(np.float32)
        got = np.array([L.orc_dm_powf(C.c_float(float(v)), C.c_float(float(y))) for v in x], dtype=np.float32)
        exact = np.power(x.astype(np.float64), np.float64(y))
        ok = exact >= MIN_NORMAL
        assert _ulp_err(got[ok], exact[ok]).max() <= 0.5001
        assert np.all(np.abs(got[~ok].astype(np.float64) - exact[~ok]) <= ULP_BOUND * DENORMAL_STEP)
    assert L.orc_dm_powf(0.0, 0.5) == 0.0 and L.orc_dm_powf(1.0, 123.0) == 1.0
    assert np.isnan(L.orc_dm_powf(float("nan"), 0.4545)) and np.isnan(L.orc_dm_powf(-1.0, 0.4545))
    assert L.orc_dm_powf(float("inf"), 0.4545) == float("inf")


def test_sampling_helpers(orc):
    L = orc.lib()
    fp = C.POINTER(C.c_float)
    # ConcentricSampleDisk (kernel.cu:190-208): inside the unit disk, centre maps to the centre
    rng = np.random.default_rng(3)
    for _ in range(2000):
        u = rng.uniform(0, 1, 2).astype(np.float32)
        out = np.zeros(2, dtype=np.float32)
        L.orc_concentric_sample_disk(u.ctypes.data_as(fp), out.ctypes.data_as(fp))
        assert out[0] ** 2 + out[1] ** 2 <= 1.0 + 1e-6
    c = np.array([0.5, 0.5], dtype=np.float32)
    out = np.ones(2, dtype=np.float32)
    L.orc_concentric_sample_disk(c.ctypes.data_as(fp), out.ctypes.data_as(fp))
    assert out[0] == 0 and out[1] == 0
    # computeOrthonormalBasisNaive (kernel.cu:181-189): orthonormal, right-handed w = u x v up to sign convention
    for _ in range(500):
        w = rng.normal(size=3)
        w = (w / np.linalg.norm(w)).astype(np.float32)
        u = np.zeros(3, dtype=np.float32)
        v = np.zeros(3, dtype=np.float32)
        L.orc_orthonormal_basis_naive(w.ctypes.data_as(fp), u.ctypes.data_as(fp), v.ctypes.data_as(fp))
        assert abs(np.dot(u, w)) < 1e-5 and abs(np.dot(v, w)) < 1e-5 and abs(np.dot(u, v)) < 1e-5
        assert abs(np.linalg.norm(u) - 1) < 1e-5 and abs(np.linalg.norm(v) - 1) < 1e-5
    # Random2DStratifiedSample (kernel.cu:44-65): inside the pixel
    s = C.c_uint32(777)
    for _ in range(2000):
        o = np.zeros(2, dtype=np.float32)
        L.orc_random_2d_stratified_sample(C.byref(s), o.ctypes.data_as(fp))
        assert 0 <= o[0] <= 1.0 and 0 <= o[1] <= 1.0


# ---- the whole contract domain ------------------------------------------------------------------------------------------


def _check_against_libm(got32: np.ndarray, exact: np.ndarray, what: str):
    """`got32` (float32) against `exact` (binary64, finite): 0.5001 ulp where the result is normal, 0.5001 denormal steps below
    2^-126, inf exactly where the exact value rounds to inf.  Returns the two measured maxima."""
    with np.errstate(over="ignore"):
        overflow = np.isinf(exact.astype(np.float32))
    assert np.array_equal(np.isinf(got32), overflow), f"{what}: overflow to inf differs from the rounding of the exact value"
    assert not np.isnan(got32).any(), what
    fin = ~overflow
    normal = fin & (np.abs(exact) >= MIN_NORMAL)
    den = fin & ~normal
    e_norm = float(_ulp_err(got32[normal], exact[normal]).max())
    e_den = float((np.abs(got32[den].astype(np.float64) - exact[den]) / DENORMAL_STEP).max()) if den.any() else 0.0
    print(f"{what}: {int(normal.sum())} normal results, max {e_norm:.9f} ulp; {int(den.sum())} denormal results, max {e_den:.7f} steps")
    assert e_norm <= ULP_BOUND, f"{what}: {e_norm} ulp"
    assert e_den <= ULP_BOUND, f"{what}: {e_den} denormal steps"
    return e_norm, e_den


def _f(bits: np.ndarray) -> np.ndarray:
    return bits.view(np.float32 if bits.dtype == np.uint32 else np.float64)


def test_map_equals_scalar_entry_points(orc):
    """orc_dm_map's binary32 results are those of the scalar entry points the wavefront oracle's code calls"""
    L = orc.lib()
    for fn, scalar, x in (("sin", L.orc_dm_sinf, ca.sincos_args()), ("cos", L.orc_dm_cosf, ca.sincos_args()), ("exp", L.orc_dm_expf, ca.exp_args())):
        xs = np.concatenate([x[::4099], x[-64:]])
        assert not ca.differing(orc.dm_map(fn, xs)["f32"], _map1(scalar, xs).view(np.uint32)).any(), fn
    x, y = ca.pow_args()
    xs, ys = np.concatenate([x[::4099], x[-240:]]), np.concatenate([y[::4099], y[-240:]])
    want = np.array([L.orc_dm_powf(C.c_float(float(a)), C.c_float(float(b))) for a, b in zip(xs, ys)], dtype=np.float32)
    assert not ca.differing(orc.dm_map("pow", xs, ys)["f32"], want.view(np.uint32)).any()
    sc = orc.dm_map("sincos", ca.sincos_args())
    assert np.array_equal(sc["sin"], orc.dm_map("sin", ca.sincos_args())["f32"]) and np.array_equal(sc["cos"], orc.dm_map("cos", ca.sincos_args())["f32"])


def test_sin_cos_full_domain(orc):
    """|x| < 2^20: uniform, log-uniform, every float nearest k pi/2 with both neighbours, every binade's edges.
    Measured (x86-64, gcc, -ffp-contract=off) over 3,059,393 arguments: sin max 0.499999648 ulp, cos max 0.499999980 ulp
    (bound 0.5001); sin's 142 denormal results are exact (sin(x) rounds to x there; bound 0.5001 steps)."""
    x = ca.sincos_args()
    inside = np.abs(x) < ca.TWO20
    xd = x[inside].astype(np.float64)
    for fn, exact in (("sin", np.sin(xd)), ("cos", np.cos(xd))):
        got = orc.dm_map(fn, x)
        _check_against_libm(_f(got["f32"])[inside], exact, fn)
        # |r| <= pi/4 (up to the rounding of the quotient) and q in 0..3: the polynomials' domain
        assert np.abs(_f(got["r"])[inside]).max() <= np.pi / 4 + 1e-9 and got["q"].max() <= 3


def test_sin_cos_defined_departures_from_libm(orc):
    """The contract's definition where it is not libm's: sin(-0.0) = +0.0 (the reduction's
    x - kd * hi is -0.0 - -0.0), and sin(x) = cos(x) = +0.0 for every finite |x| >= 2^20 (x - x); inf and NaN give NaN."""
    x = np.array([-0.0, 0.0, 2.0 ** 20, -(2.0 ** 20), np.nextafter(ca.TWO20, np.float32(np.inf)), 1e30, -1e30, np.finfo(np.float32).max, np.inf, -np.inf, np.nan], dtype=np.float32)
    s, c = orc.dm_map("sin", x), orc.dm_map("cos", x)
    one = np.float32(1).view(np.uint32)
    assert s["f32"][0] == 0 and s["f32"][1] == 0 and c["f32"][0] == one and c["f32"][1] == one  # +0.0, not -0.0
    assert np.all(s["f32"][2:8] == 0) and np.all(c["f32"][2:8] == 0)
    assert np.isnan(_f(s["f32"])[8:]).all() and np.isnan(_f(c["f32"])[8:]).all()
    below = np.array([np.nextafter(ca.TWO20, np.float32(0))], dtype=np.float32)  # the last argument inside: an ordinary value
    assert abs(float(_f(orc.dm_map("sin", below)["f32"])[0]) - np.sin(float(below[0]))) < 1e-7


def test_exp_full_domain(orc):
    """[-104.5, 89.5] with every threshold (0 below -104, denormal results below -87.34, inf from 88.7229 by rounding and
    above 89 by the guard).  Measured over 1,181,608 finite results: normal results max 0.499999985 ulp (bound 0.5001),
    denormal results max 0.4999925 steps of 2^-149 (bound 0.5001)."""
    x = ca.exp_args()
    fin = np.isfinite(x)
    got = _f(orc.dm_map("exp", x)["f32"])
    with np.errstate(over="ignore", under="ignore"):
        exact = np.exp(x[fin].astype(np.float64))
    ok = np.isfinite(exact)  # past 709.78 even binary64 overflows: inf on both sides
    assert np.all(np.isinf(got[fin][~ok]))
    _check_against_libm(got[fin][ok], exact[ok], "exp")
    t = orc.dm_map("exp", np.array([-104.0, np.nextafter(np.float32(-104), np.float32(-200)), 89.0, np.nextafter(np.float32(89), np.float32(100)), -np.inf, np.inf, np.nan, 0.0, -0.0], dtype=np.float32))
    v = _f(t["f32"])
    assert v[0] == 0.0 and t["kd"][0] != 0  # -104 is computed (kd = -150) and rounds to 0; below it the guard answers
    assert v[1] == 0.0 and t["kd"][1] == 0 and np.isinf(v[2]) and t["kd"][2] != 0 and np.isinf(v[3]) and t["kd"][3] == 0
    assert v[4] == 0.0 and np.isinf(v[5]) and np.isnan(v[6]) and v[7] == 1.0 and v[8] == 1.0


def test_pow_full_domain(orc):
    """x over every positive binade, denormals included, y in [-3, 3]; the path's exponents 1/41, 40, 1/2.2.
    Measured over 856,189 finite results: normal results max 0.499999993 ulp (bound 0.5001), denormal results max
    0.5000000 steps of 2^-149 (bound 0.5001; exact ties such as 2^-150 round to even)."""
    x, y = ca.pow_args()
    use = (x > 0) & np.isfinite(x) & np.isfinite(y)
    got = _f(orc.dm_map("pow", x, y)["f32"])[use]
    with np.errstate(over="ignore", under="ignore"):
        exact = np.power(x[use].astype(np.float64), y[use].astype(np.float64))
    ok = np.isfinite(exact)
    assert np.all(np.isinf(got[~ok]))
    _check_against_libm(got[ok], exact[ok], "pow")
    L = orc.lib()
    assert L.orc_dm_powf(0.0, -1.0) == float("inf") and L.orc_dm_powf(0.0, 0.0) == 1.0 and L.orc_dm_powf(float("inf"), -1.0) == 0.0
    assert np.isnan(L.orc_dm_powf(2.0, float("nan"))) and np.isnan(L.orc_dm_powf(float("-inf"), 2.0))


def _has_fma() -> bool:
    try:
        with open("/proc/cpuinfo") as f:
            return any(" fma " in line + " " for line in f if line.startswith("flags"))
    except OSError:
        return False


def test_binary64_comparison_sees_a_contracted_build(orc, tmp_path):
    """Why the device is compared with the oracle in binary64 and not only after the rounding to binary32.

    oracle/orc_dm.c is compiled a second time with -ffp-contract=fast -mfma: the same source, another sequence of IEEE
    operations (fused multiply-adds in the polynomial layer).  The comparison the device tests use
    (contract_args.count_differing) on the device tests' argument sets must report it.

    Measured here (x86-64, gcc) on the path's shapes sin/cos(2 pi u), exp(-20 u), pow(u, 1/2.2), 2^20 arguments each:
    binary32 results that differ: 0 of 4,194,304 (sin 0, cos 0, exp 0, pow 0);
    binary64 values that differ: sin's rounded value 48,034, cos's 47,954, exp's 102,583, pow's 122,450 (its log2: 69,666).
    On the device tests' full argument sets: binary32 0 of 8.2 M; binary64 sin 31,835, cos 32,520, exp 113,998, pow 77,294.
    A test that compares after the rounding passes such a build; one decision in 10^8..10^9 calls then flips in a render."""
    if not _has_fma():
        pytest.skip("this CPU has no FMA")
    so = str(tmp_path / "liborc_dm_contracted.so")
    src = os.path.join(os.path.dirname(orc.__file__), "orc_dm.c")
    cc = os.environ.get("CC", "gcc")
    try:
        done = subprocess.run([cc, "-std=c11", "-O2", "-fPIC", "-ffp-contract=fast", "-mfma", "-shared", "-o", so, src, "-lm"], capture_output=True, text=True)
    except OSError:
        pytest.skip(f"no C compiler ({cc})")
    if done.returncode:
        pytest.skip(f"{cc} does not build with -mfma: {done.stderr[-200:]}")
    contracted = orc.load_dm(so)
    rng = np.random.default_rng(26)
    u = rng.uniform(0, 1, 1 << 20).astype(np.float32)
    path = {"sin": (np.float32(2 * np.pi) * u, None), "cos": (np.float32(2 * np.pi) * u, None), "exp": (np.float32(-20) * u, None), "pow": (u, np.full_like(u, ca.POW_PATH_EXPONENTS[2]))}
    n32 = 0
    for fn, (x, y) in path.items():
        d = ca.count_differing(orc.dm_map(fn, x, y, L=contracted), orc.dm_map(fn, x, y))
        print(f"path {fn}: {d}")
        n32 += d["f32"]
        assert d["rounded"] > 0, f"{fn}: the binary64 comparison does not see the contracted build"
    print(f"path: {n32} binary32 results differ")
    # ... and on the full argument sets of the device tests
    x, y = ca.pow_args()
    for fn, args in (("sin", (ca.sincos_args(),)), ("cos", (ca.sincos_args(),)), ("exp", (ca.exp_args(),)), ("pow", (x, y))):
        d = ca.count_differing(orc.dm_map(fn, *args, L=contracted), orc.dm_map(fn, *args))
        print(f"full {fn}: {d}")
        assert d["rounded"] > 0, fn
    assert ca.count_differing(orc.dm_map("pow", x, y, L=contracted), orc.dm_map("pow", x, y))["log2"] > 0
