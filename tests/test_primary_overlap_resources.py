"""What the compiler made of the two kernels of a split top-up (hip/frame.hip k_primary_window, k_primary_rest; no GPU needed).

k_primary_rest runs beside the traversal launch of its iteration, which host/driver.cpp sizes at three to five 256-thread blocks
per CU for that purpose: it only overlaps anything if its blocks find registers and LDS next to them.  And the path that traces a
stray ray inside k_primary_rest must not cost every other ray a spill or a scratch access."""
import pytest

from kernel_resources import have_hipcc, make_asm, parse_resources

LDS_PER_CU = 163840  # MI355X: 160 KB per CU, handed out in 1280-byte granules
LDS_GRANULE = 1280
VGPRS_PER_SIMD = 512
TRACE_BLOCKS = 3     # the fewest traversal blocks per CU a split iteration may run (TYR_TUNE_OVERLAP_TRACE_BLOCKS)
NEW = ("k_primary_windowENS", "k_primary_restENS")


@pytest.fixture(scope="module")
def resources():
    if not have_hipcc():
        pytest.skip("no hipcc")
    make_asm()
    r = {}
    for unit in ("frame", "traverse_flat"):
        r.update(parse_resources(unit))
    return r


def _kernel(resources, key):
    names = [n for n in resources if key in n]
    assert len(names) == 1, (key, names)
    return resources[names[0]]


def _granules(lds_bytes):
    return -(-lds_bytes // LDS_GRANULE) * LDS_GRANULE


@pytest.mark.parametrize("key", NEW)
def test_no_spill_and_no_scratch(resources, key):
    k = _kernel(resources, key)
    assert k["SGPRs Spill"] == 0 and k["VGPRs Spill"] == 0 and k["ScratchSize [bytes/lane]"] == 0, k


@pytest.mark.parametrize("key", NEW)
def test_a_block_fits_a_cu_beside_three_traversal_blocks(resources, key):
    k, t = _kernel(resources, key), _kernel(resources, "k_trace_flatILi12ELj256E")
    assert _granules(k["LDS Size [bytes/block]"]) + TRACE_BLOCKS * _granules(t["LDS Size [bytes/block]"]) <= LDS_PER_CU, (k, t)
    # a block is one wave per SIMD: this kernel's registers beside those of three traversal waves
    assert k["VGPRs"] + k["AGPRs"] + TRACE_BLOCKS * (t["VGPRs"] + t["AGPRs"]) <= VGPRS_PER_SIMD, (k, t)


def test_the_shared_body_left_k_primary_as_it_was(resources):
    """k_primary is the same body with the window's branches compiled out: no more registers than the window part, no LDS beyond its 44 bytes"""
    k, w = _kernel(resources, "k_primaryENS"), _kernel(resources, "k_primary_windowENS")
    assert k["VGPRs"] <= w["VGPRs"] and k["LDS Size [bytes/block]"] == 44, (k, w)
