"""What the compiler reports for the kernels of a unit (registers, spills, scratch, LDS, occupancy): the parser of
tyrant_amd/csrc/build/<unit>.resources.txt, which `make -C tyrant_amd/csrc asm` writes (-Rpass-analysis=kernel-resource-usage),
for the resource tests of the test modules."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tyrant_amd", "csrc")


def have_hipcc():
    return shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def make_asm():
    subprocess.run(["make", "-s", "-C", CSRC, "asm"], check=True, capture_output=True, timeout=900)


def parse_resources(unit):
    """{mangled kernel name: {field: value}} of an already built unit; numbers as int"""
    res, cur = {}, None
    for line in open(os.path.join(CSRC, "build", f"{unit}.resources.txt")):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name:"):
            cur = res.setdefault(text.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in text:
            k, v = text.rsplit(":", 1)
            cur[k.strip()] = int(v) if v.strip().lstrip("-").isdigit() else v.strip()
    return res


def kernel_resources(unit):
    """builds the listings (a test that needs them fails without a compiler) and parses the unit's"""
    if not have_hipcc():
        pytest.fail("no hipcc: the kernels cannot be built")
    make_asm()
    return parse_resources(unit)
