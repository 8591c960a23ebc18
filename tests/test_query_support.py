"""The checks tests/query_support.py makes for the query test modules still catch what they are there to catch: `same` on a sign
of zero, a shape, a dtype and equal NaNs; the kernel budget on a spill, a byte of scratch, a block of LDS and a missing kernel."""
import numpy as np
import pytest

from query_support import check_kernel_budget, same

F = np.float32


def test_same_compares_float32_by_bits():
    a = np.array([1.0, 0.0, 2.0], F)
    same(("x",), (a,), (a.copy(),))
    with pytest.raises(AssertionError, match=r"x differs at \[\[1\]\] \(1 values\)"):
        same(("x",), (a,), (np.array([1.0, -0.0, 2.0], F),), "a lone -0.0")
    nan = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000], np.uint32).view(F)
    same(("x",), (nan,), (nan.copy(),))  # equal NaN bit patterns are equal
    with pytest.raises(AssertionError):
        same(("x",), (nan,), (nan[::-1].copy(),))  # ... and other NaNs are not


def test_same_compares_shape_and_dtype():
    a = np.zeros((4, 2), np.int32)
    with pytest.raises(AssertionError, match="shape"):
        same(("x",), (a,), (a.reshape(2, 4),))
    with pytest.raises(AssertionError, match="int32, not int64"):
        same(("x",), (a,), (a.astype(np.int64),))
    same(("x",), (a,), (a.astype(np.int64),), dtype=False)
    with pytest.raises(AssertionError, match="float32, not float64"):
        same(("x",), (a.astype(F),), (a.astype(np.float64),))
    same(("x", "y"), (a, None), (a.copy(), a))  # an output that was not asked for


def record(spill=0, scratch=432, lds=31744, occupancy=5):
    return {"VGPRs Spill": spill, "ScratchSize [bytes/lane]": scratch, "LDS Size [bytes/block]": lds, "Occupancy [waves/SIMD]": occupancy}


GOOD = {"_Z7k_queryILb0EEvv": record(), "_Z7k_queryILb1EEvv": record(), "_Z7k_othervv": record(spill=3)}


def test_kernel_budget_passes_what_is_in_budget():
    """31,744 bytes of LDS round up to 25 granules of 1280, 32,000 bytes: five blocks fill 160,000 of a CU's 163,840"""
    assert len(check_kernel_budget(GOOD, "k_query", 2, 432, 31744)) == 2
    check_kernel_budget({"k_query": record(lds=32000)}, "k_query", 1, 432)


@pytest.mark.parametrize("bad,lds_max", [(record(spill=1), 31744), (record(scratch=433), 31744), (record(lds=31745), 31744), (record(lds=32001), None), (record(occupancy=4), 31744)],
                         ids=["a spilled VGPR", "scratch one byte over", "LDS one byte over the cap", "LDS that admits four blocks", "an occupancy of four"])
def test_kernel_budget_catches_each_excess(bad, lds_max):
    with pytest.raises(AssertionError):
        check_kernel_budget({**GOOD, "_Z7k_queryILb1EEvv": bad}, "k_query", 2, 432, lds_max)


def test_kernel_budget_catches_a_wrong_kernel_count_and_follows_planned():
    with pytest.raises(AssertionError):
        check_kernel_budget(GOOD, "k_query", 1, 432, 31744)
    with pytest.raises(AssertionError):
        check_kernel_budget(GOOD, "k_queryILb2E", 1, 432, 31744)
    check_kernel_budget(GOOD, "k_query", 2, 432, 31744, planned=4)
    with pytest.raises(AssertionError):
        check_kernel_budget(GOOD, "k_query", 2, 432, 31744, planned=6)
