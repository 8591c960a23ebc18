"""Instruction budget of the traversal loops (no GPU needed: hipcc cross-compiles gfx950), from `make -C tyrant_amd/csrc asm`.

Once a launch's queue is used up, its drain is bound by the vector and scalar instructions each trip of the traversal loop
issues, summed over the waves of a SIMD.  Two forms of the same loop at one register budget can differ
by a third in instructions per trip and give the same answers, so no parity test notices when a change brings the
exec-mask bookkeeping, the per-lane 64-bit address arithmetic or the reordering of a quad node's four slots back.  This file
counts the static VALU + SALU instructions of the loops (the blocks of a loop and of the loops nested in it, as the
compiler's listing marks them) against budgets set just above today's counts:
  - wide_drain's loop (the drain four lanes to a ray) and its leaf round, and
  - k_trace_flat's descent loop (one pop + one quad node per lane per trip),
and that neither form of k_trace_flat spills vector registers or drops below its waves per SIMD.

The counts are an approximation of the loops' extent: the listing marks loop membership on `.LBB` labels only, so an
unlabelled fall-through block (`; %bb.N:`) is counted with the labelled block before it, even where it lies outside the
loop.  A compiler that lays the blocks out differently can move a few instructions across that line without any change in
what a trip executes: before taking a failure here for a regression, look at the blocks (tools/isa_blocks.py)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tyrant_amd", "csrc")

# static VALU + SALU of the loops (both box-test forms of each are in the count); the counts these replaced: 443 / 169 / 640.
# The descent's count also holds the paths a trip takes only when a lane's stack leaves LDS (the pop's and the pushes' private
# part), which the select form of the pop duplicates: its static total falls less than a trip does (~314 -> ~270 on the path
# a trip with finite 1/d takes).
WIDE_LOOP_BUDGET = 385
WIDE_LEAF_ROUND_BUDGET = 150
DESCENT_LOOP_BUDGET = 620


@pytest.fixture(scope="module")
def listing():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-s", "-C", CSRC, "asm"], check=True, capture_output=True, timeout=900)
    with open(os.path.join(CSRC, "build", "traverse_flat.s")) as f:
        return f.read().split("\n")


def _blocks(lines, key):
    """[name, loop comment, valu, salu] per labelled block of the function whose mangled name contains `key`"""
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and key in l]
    assert len(starts) == 1, (key, len(starts))
    i0 = starts[0]
    end = next(k for k in range(i0 + 1, len(lines)) if lines[k].startswith(".Lfunc_end"))
    out, cur = [], ["entry", "", 0, 0]
    for line in lines[i0:end]:
        m = re.match(r"^\.LBB(\d+_\d+):\s*;?(.*)", line)
        if m:
            out.append(cur)
            cur = ["BB" + m.group(1), m.group(2), 0, 0]
            continue
        t = line.strip()
        if line.startswith("\t") and t and not t.startswith((".", ";")):
            cur[2] += t.startswith("v_")
            cur[3] += t.startswith("s_")
    out.append(cur)
    return out


def _loop_size(blocks, header):
    """VALU + SALU of the loop headed by `header`, the loops nested in it included"""
    inner = {header}
    grew = True
    while grew:
        grew = False
        for name, comment, _, _ in blocks:
            m = re.search(r"Parent Loop (BB\d+_\d+)", comment)
            if m and m.group(1) in inner and name not in inner:
                inner.add(name)
                grew = True
    total = 0
    for name, comment, v, s in blocks:
        m = re.search(r"Header=(BB\d+_\d+)", comment)
        if name in inner or (m and m.group(1) in inner):
            total += v + s
    return total


def _loops(blocks):
    """(header, parent header or None) of every loop"""
    out = []
    for name, comment, _, _ in blocks:
        m = re.search(r"Parent Loop (BB\d+_\d+)", comment)
        if m:
            out.append((name, m.group(1)))
        elif "Loop Header" in comment:
            out.append((name, None))
    return out


def test_wide_drain_loop_meets_its_instruction_budget(listing):
    b = _blocks(listing, "wide_drain")
    loops = _loops(b)
    outer = [h for h, p in loops if p is None]
    assert len(outer) == 1, loops  # one loop: a trip per quad step of the wave's groups
    inner = [h for h, p in loops if p == outer[0]]
    assert len(inner) == 1, loops  # ... with the leaf's rounds of four primitives inside it
    whole, leaf = _loop_size(b, outer[0]), _loop_size(b, inner[0])
    assert leaf <= WIDE_LEAF_ROUND_BUDGET, (leaf, WIDE_LEAF_ROUND_BUDGET)
    assert whole <= WIDE_LOOP_BUDGET, (whole, WIDE_LOOP_BUDGET)


def test_wide_drain_keeps_its_state_in_registers(listing):
    i0 = next(i for i, l in enumerate(listing) if re.match(r"^_Z\w*wide_drain\w*:", l))
    end = next(k for k in range(i0 + 1, len(listing)) if listing[k].startswith(".Lfunc_end"))
    body = [l.strip() for l in listing[i0:end]]
    assert not [l for l in body if l.startswith(("scratch_", "buffer_"))], "wide_drain touches private memory"
    assert not [l for l in body if l.startswith("flat_")], "wide_drain reaches memory through generic pointers"


def test_descent_loop_of_k_trace_flat_meets_its_instruction_budget(listing):
    for key in ("k_trace_flatILi12ELj768E", "k_trace_flatILi12ELj256E"):
        b = _blocks(listing, key)
        # the descent loop is the one that tests quad nodes: the loop nested in the kernel's main loop with the most instructions
        loops = _loops(b)
        nested = [h for h, p in loops if p is not None]
        descent = max(nested, key=lambda h: _loop_size(b, h))
        size = _loop_size(b, descent)
        assert size <= DESCENT_LOOP_BUDGET, (key, size, DESCENT_LOOP_BUDGET)


def _resources():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "build", "traverse_flat.resources.txt")):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name:"):
            cur = out.setdefault(text.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in text:
            k, v = text.rsplit(":", 1)
            cur[k.strip()] = int(v.strip()) if v.strip().lstrip("-").isdigit() else v.strip()
    return out


@pytest.mark.parametrize("key,waves,vgprs", [("k_trace_flatILi12ELj768E", 6, 80), ("k_trace_flatILi12ELj256E", 5, 96)])
def test_trace_kernels_keep_their_occupancy_without_vector_spills(listing, key, waves, vgprs):
    r = _resources()
    names = [n for n in r if key in n]
    assert len(names) == 1, names
    k = r[names[0]]
    assert k["VGPRs Spill"] == 0, k
    assert k["Occupancy [waves/SIMD]"] >= waves and k["VGPRs"] + k["AGPRs"] <= vgprs, k
