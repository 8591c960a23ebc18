"""k_shade<false, true> (TYR_TUNE_SHADE_DENSE) under the limits tests/test_kernel_resources.py holds k_shade to: the
dense path's requests and answers live in the staging area of the tile before (no LDS of their own), it runs five blocks per CU
at no more than 96 vector registers, and it spills nothing, neither to scratch nor to vector lanes (round 4 found 113 scalar
values in lanes of k_shade, worth 15 % of the kernel).  What holds that with the present compiler is hand-steered (hip/shade.hip:
the thread id passed through an empty asm per tile, the lane's flags packed into one register through the dense phase, the
arguments read again behind it, per-wave sums in LDS): this file says when it stops holding.  There is no dense kernel for
TYR_FLAG_LIGHT_LIST -- its instantiation kept four scalar values in vector lanes -- and a ctx with that flag runs the lane path."""

import pytest

from kernel_resources import have_hipcc, make_asm, parse_resources
from test_kernel_resources import _blocks_that_fit, _kernel


@pytest.fixture(scope="module")
def resources():
    if not have_hipcc():
        pytest.skip("no hipcc")
    make_asm()
    return parse_resources("shade")


def test_dense_k_shade_spills_nothing_and_runs_five_blocks_per_cu(resources):
    k = _kernel(resources, "k_shadeILb0ELb1EEE")
    assert k["SGPRs Spill"] == 0 and k["VGPRs Spill"] == 0 and k["ScratchSize [bytes/lane]"] == 0, k
    assert k["Occupancy [waves/SIMD]"] >= 5 and k["VGPRs"] + k["AGPRs"] <= 96, k
    assert _blocks_that_fit(k["LDS Size [bytes/block]"]) >= 5, k


def test_the_dense_path_adds_no_lds(resources):
    assert _kernel(resources, "k_shadeILb0ELb1EEE")["LDS Size [bytes/block]"] == _kernel(resources, "k_shadeILb0EEE")["LDS Size [bytes/block]"]


def test_no_dense_kernel_for_the_light_list(resources):
    assert [n for n in resources if "k_shadeILb1ELb" in n] == []
