"""DESIGN.md section 2, item 2, where it can fail: hip/detmath.hpp's sin / cos / exp / pow and the samplers of
hip/device_common.hpp, evaluated ON THE DEVICE (tyr_vecmath_probe ops 32-49), against the oracle's orc_dm_map /
orc_sampler_map over the argument sets of tests/contract_args.py.

The transcendental functions are compared in BINARY64 -- the reduced argument, the quadrant, log2, and the value that is
rounded -- as well as after the rounding to binary32: a device build whose operation sequence differs (a contracted
multiply-add, another rounding of rint or of the binary64 division) shows in the binary64 values of tens of thousands of
these arguments and in the binary32 results of none (tests/test_oracle_math.py
test_binary64_comparison_sees_a_contracted_build measures that on a contracted build of the oracle).

Comparison rule (contract_args.differing): finite values, signed zeros and infinities by bits; NaNs by class; seeds,
quadrants and counts as integers.
"""
import ctypes as C

import numpy as np
import pytest

import contract_args as ca

ONE = int(np.float32(1).view(np.uint32))


def _f(bits):
    return np.ascontiguousarray(bits).view(np.float32)


# ---- CPU: the oracle's sampler map is the oracle's samplers, and the branch edges are where the inputs say ---------------


def test_sampler_map_equals_scalar_entry_points(orc):
    L = orc.lib()
    fp = C.POINTER(C.c_float)
    seeds = np.concatenate([ca.rng_seeds()[::8191], ca.rng_seeds()[-160:]])
    a, b, st = orc.sampler_map(0, seeds), orc.sampler_map(1, seeds), orc.sampler_map(2, seeds)
    for i, s0 in enumerate(seeds[:, 0]):
        s = C.c_uint32(int(s0))
        assert np.float32(L.orc_random_float(C.byref(s))).view(np.uint32) == a[i, 0] and s.value == a[i, 1]
        s = C.c_uint32(int(s0))
        assert L.orc_random_int_between_0_and_max(C.byref(s), 16) == a[i, 2] and s.value == b[i, 2]
        s = C.c_uint32(int(s0))
        assert np.float32(L.orc_random_float2(C.byref(s))).view(np.uint32) == b[i, 0] and s.value == b[i, 1]
        s = C.c_uint32(int(s0))
        o = np.zeros(2, dtype=np.float32)
        L.orc_random_2d_stratified_sample(C.byref(s), o.ctypes.data_as(fp))
        assert np.array_equal(o.view(np.uint32), st[i, :2]) and s.value == st[i, 2]
    disk = np.concatenate([ca.disk_inputs()[::1021], ca.disk_inputs()[-49:]])
    d = orc.sampler_map(3, disk.view(np.uint32))
    for i, u in enumerate(disk):
        o = np.zeros(2, dtype=np.float32)
        L.orc_concentric_sample_disk(np.ascontiguousarray(u[:2]).ctypes.data_as(fp), o.ctypes.data_as(fp))
        assert np.array_equal(o.view(np.uint32), d[i, :2]) and d[i, 2] == 0
    ws = np.concatenate([ca.basis_inputs()[::1021], ca.basis_inputs()[-400:-1]])
    bu, bv = orc.sampler_map(4, ws.view(np.uint32)), orc.sampler_map(5, ws.view(np.uint32))
    for i, w in enumerate(ws):
        u, v = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        L.orc_orthonormal_basis_naive(np.ascontiguousarray(w).ctypes.data_as(fp), u.ctypes.data_as(fp), v.ctypes.data_as(fp))
        assert np.array_equal(u.view(np.uint32), bu[i]) and np.array_equal(v.view(np.uint32), bv[i])


def test_sampler_branch_edges_in_the_oracle(orc):
    """what the edge inputs are there for, pinned on the oracle (the device is then held to the oracle's bits)"""
    seeds = ca.rng_seeds()
    a, b, st = orc.sampler_map(0, seeds), orc.sampler_map(1, seeds), orc.sampler_map(2, seeds)
    zero = np.flatnonzero(seeds[:, 0] == 0)
    assert zero.size >= 1 and np.all(a[zero] == 0) and np.all(b[zero] == 0) and np.all(st[zero] == 0)  # seed 0 stays 0, every draw is 0
    top = slice(-(ca.N_TOP_SEEDS + 16), -16)
    assert np.all(a[top, 0] == ONE) and np.all(a[top, 2] == 16)  # rng_float == 1.0f (the scale is 2^-32), stratum 16
    assert np.all(_f(a[-16:, 0]) < 1) and np.all(a[-16:, 2] == 16)  # the draws just below: under 1.0f, still stratum 16
    assert np.all(_f(a[:, 0]) <= 1) and a[:, 2].max() == 16 and np.all(_f(b[:, 0]) <= 1) and _f(b[:, 0]).max() == 1
    # stratum 16 aliases stratum 0 (kernel.cu:44-65): the sample of a top seed lies in the first cell, or on its far edge
    assert np.all(_f(st[top, :2]) <= 0.25)
    assert np.all(_f(st[:, :2]) >= 0) and np.all(_f(st[:, :2]) <= 1)

    uv = ca.disk_inputs()
    d = _f(orc.sampler_map(3, uv.view(np.uint32))[:, :2])
    centre = np.flatnonzero((uv[:, 0] == 0.5) & (uv[:, 1] == 0.5))
    assert centre.size >= 1 and np.all(d[centre].view(np.uint32) == 0)
    assert np.all(np.hypot(d[:, 0].astype(np.float64), d[:, 1].astype(np.float64)) <= 1 + 1e-6)
    ox, oy = 2 * uv[:, 0].astype(np.float64) - 1, 2 * uv[:, 1].astype(np.float64) - 1
    diag = (np.abs(ox) == np.abs(oy)) & (ox != 0)
    assert (diag & (ox == oy)).sum() > 1000 and (diag & (ox == -oy)).sum() > 1000
    # on the diagonals the second branch is taken (|ox| > |oy| is false): r = oy, theta = pi/2 -+ pi/4
    assert np.allclose(np.hypot(d[diag, 0], d[diag, 1]), np.abs(oy[diag]), rtol=1e-6)
    assert ((ox == 0) & (oy != 0)).sum() > 500 and ((oy == 0) & (ox != 0)).sum() > 500

    w = ca.basis_inputs()
    u = _f(orc.sampler_map(4, w.view(np.uint32)))
    for wx in ca.BASIS_EDGE_X:
        at = np.flatnonzero(w[:, 0] == wx)[-64:]
        assert at.size == 64
        # (double)|w.x| > .9: false at 0.9f (0.89999998) and below, true at its successor; u = (0,1,0) x w has u.y == 0,
        # u = (1,0,0) x w has u.x == 0
        if abs(float(wx)) > 0.9:
            assert np.all(u[at, 1] == 0) and np.all(u[at, 0] != 0)
        else:
            assert np.all(u[at, 0] == 0) and np.all(u[at, 1] != 0)
    assert abs(float(np.float32(0.9))) < 0.9 < abs(float(np.nextafter(np.float32(0.9), np.float32(1))))
    assert np.isnan(u[-1]).all() and not np.isnan(u[:-1]).any()  # w = 0: normalize(0) is 0 * inf


# ---- GPU ---------------------------------------------------------------------------------------------------------------


def _args(fn):
    if fn == "pow":
        return ca.pow_args()
    return ((ca.exp_args() if fn == "exp" else ca.sincos_args()),)


@pytest.fixture(scope="module")
def oracle_values(orc):
    cache = {}

    def get(fn):
        if fn not in cache:
            cache[fn] = orc.dm_map(fn, *_args(fn))
        return cache[fn]

    return get


@pytest.fixture(scope="module")
def device_values(hip):
    cache = {}

    def get(fn):
        if fn not in cache:
            cache[fn] = ca.device_dm_map(hip, fn, *_args(fn))
        return cache[fn]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["sin", "cos", "exp", "pow"])
def test_device_function_equals_oracle_in_binary64_and_binary32(fn, oracle_values, device_values):
    """the binary32 result, and every binary64 value on the way to it, of sinf_det / cosf_det / expf_det / powf_det over
    the contract's whole domain"""
    got, want = device_values(fn), oracle_values(fn)
    counts = ca.count_differing(got, want)
    print(fn, want["f32"].shape[0], "arguments, differing:", counts)
    assert not any(counts.values()), ca.first_differing(got, want, _args(fn))


@pytest.mark.gpu
def test_device_sincos_equals_the_single_calls(oracle_values, device_values):
    """sincosf_det's two results are sinf_det's and cosf_det's bit for bit (hip/detmath.hpp's promise: the disk map and the
    cone sample use it where the oracle calls dm_sinf and dm_cosf)"""
    got, want = device_values("sincos"), oracle_values("sincos")
    counts = ca.count_differing(got, want)
    assert not any(counts.values()), ca.first_differing(got, want, _args("sincos"))
    assert np.array_equal(got["sin"], device_values("sin")["f32"]) and np.array_equal(got["cos"], device_values("cos")["f32"])


def _words_differ(got, want, float_columns):
    bad = np.zeros(got.shape[0], dtype=bool)
    for c in range(3):
        bad |= ca.differing(got[:, c], want[:, c], integers=c not in float_columns)
    return np.flatnonzero(bad)


def _assert_words(got, want, inputs, float_columns, what):
    bad = _words_differ(got, want, float_columns)
    msg = "\n".join(f"{what}[{i}] in {[hex(int(v)) for v in inputs[i]]}: got {[hex(int(v)) for v in got[i]]}, want {[hex(int(v)) for v in want[i]]}" for i in bad[:4])
    assert bad.size == 0, f"{bad.size} of {got.shape[0]} differ\n{msg}"


@pytest.mark.gpu
def test_device_rng_equals_oracle(hip, orc):
    """rng_float, rng_float2, rng_int_0_max(s, 16) and the seed after each, from 2^20 seeds, seed 0 and the seeds whose first
    draw rounds to 2^32 (rng_float == 1.0f, stratum 16); then the stratified sample built on them"""
    seeds = ca.rng_seeds()
    a = hip.contract_probe(44, seeds)
    _assert_words(a, orc.sampler_map(0, seeds), seeds, (0,), "rng_float / rng_int_0_max")
    _assert_words(hip.contract_probe(45, seeds), orc.sampler_map(1, seeds), seeds, (0,), "rng_float2")
    _assert_words(hip.contract_probe(46, seeds), orc.sampler_map(2, seeds), seeds, (0, 1), "stratified_sample")
    top = slice(-(ca.N_TOP_SEEDS + 16), -16)
    assert np.all(a[top, 0] == ONE) and np.all(a[top, 2] == 16)
    zero = np.flatnonzero(seeds[:, 0] == 0)
    assert np.all(a[zero] == 0)


@pytest.mark.gpu
def test_device_disk_map_equals_oracle(hip, orc):
    """concentric_sample_disk over a unit square and at its branch edges: the centre, |ox| == |oy| with equal and opposite
    signs, one offset exactly 0, and 0, 1 - 2^-24 and 1 in each coordinate"""
    uv = ca.disk_inputs()
    _assert_words(hip.contract_probe(47, uv), orc.sampler_map(3, uv.view(np.uint32)), uv.view(np.uint32), (0, 1, 2), "concentric_sample_disk")


@pytest.mark.gpu
def test_device_orthonormal_basis_equals_oracle(hip, orc):
    """orthonormal_basis_naive over unit vectors, at the binary64 compare |w.x| > .9 (0.9f and both neighbours, both signs), on
    the axes, and for w = 0 (NaNs, by class)"""
    w = ca.basis_inputs()
    wb = w.view(np.uint32)
    _assert_words(hip.contract_probe(48, w), orc.sampler_map(4, wb), wb, (0, 1, 2), "orthonormal_basis_naive u")
    _assert_words(hip.contract_probe(49, w), orc.sampler_map(5, wb), wb, (0, 1, 2), "orthonormal_basis_naive v")
