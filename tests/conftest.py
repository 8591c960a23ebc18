"""Shared fixtures.

`-m "not gpu"`: oracle vs golden vectors / the reference-header harness's answers, host logic,
C-ABI symbol checks -- no GPU, and nothing outside the repository (see `ref_answers`).
`-m gpu`: parity of the HIP path (through the C ABI) against the oracle on an MI355X.
"""
from __future__ import annotations

import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

# PyTorch's wheels bundle their own HIP runtime (libamdhip64.so + ROCr, loaded into the global symbol scope); the product
# library links the ROCm installation's.  A process must end up with ONE of them: when PyTorch is imported first, the
# library's HIP calls bind to PyTorch's copy (what bench.py has always done); loaded the other way round, the process
# holds two runtimes and the second one to initialise finds no device.  The GPU tests that use torch for device memory
# therefore import it here, before any fixture loads the library (tyrant_amd/binding.py lib()).
try:
    import torch  # noqa: F401
except ImportError:  # the library alone: one runtime anyway
    pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (run by the driver with -m gpu)")


# Collection order (round 4).  The driver runs `pytest -m gpu -x -q`: whatever is collected first decides whether anything
# else runs at all.  Kernel parity therefore comes first, host / scene / camera tests next, and tests that only check the
# FORMAT of bench.py's line (child processes, timings of micro-jobs) last: a bench-format assertion can never again
# stand in front of the parity tests (round 3: one rounded timing, `0.0 > 0`, left 101 parity tests unreached).
_ORDER = ("test_gpu_parity", "test_gpu_configs", "test_ref_pins", "test_bvh_build_device", "test_glm_pinning", "test_debug_bvh", "test_dist_native", "test_scene_io",
          "test_camera_input", "test_oracle_golden", "test_oracle_math", "test_oracle_wavefront", "test_host_and_abi", "test_dist_gloo")
_LAST = ("test_bench_contract",)


def pytest_collection_modifyitems(session, config, items):
    def rank(item):
        mod = os.path.splitext(os.path.basename(str(item.fspath)))[0]
        if mod in _LAST:
            return len(_ORDER) + 1 + _LAST.index(mod)
        return _ORDER.index(mod) if mod in _ORDER else len(_ORDER)

    items.sort(key=rank)  # stable: the order inside a module stays the file's


@pytest.fixture(scope="session")
def orc():
    from oracle import pyorc

    pyorc.lib()  # builds oracle/_build/liborc.so on first use
    return pyorc


# The reference-header harness (oracle/_ref/libref_traverse.so, `make -C oracle ref`) can only be built where the
# reference's sources are.  The tests that consult it therefore go through `ref_answers`: where the harness is built
# they ask it live and hold the record to what it says; everywhere else they get what it answered to the same inputs,
# recorded in tests/golden/ref_answers.npz.  With the harness built, TYR_RECORD_REF_ANSWERS=1 rewrites the record of
# every test that runs (python -m pytest -m "not gpu" tests).
REF_ANSWERS = os.path.join(GOLDEN, "ref_answers.npz")


def _digest(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class RefAnswers:
    """answers(key, ask, inputs, needs) -> {name: array}: `ask(harness)` computes them live; `inputs` are the arrays they
    depend on (their digest is recorded with them, so a record is never replayed for other inputs); `needs` names the
    harness exports `ask` calls (an older harness without them is not asked)"""

    def __init__(self, lib):
        self.lib = lib
        self.recording = os.environ.get("TYR_RECORD_REF_ANSWERS") == "1"
        self.recorded = {}
        if os.path.exists(REF_ANSWERS):
            with np.load(REF_ANSWERS) as z:
                self.recorded = dict(z)
        self.new = {}

    def __call__(self, key, ask, inputs=(), needs=()):
        digest = _digest(inputs)
        live = self.lib is not None and all(hasattr(self.lib, n) for n in needs)
        got = {k: np.asarray(v) for k, v in ask(self.lib).items()} if live else None
        if self.recording:
            if not live:
                pytest.fail(f"{key}: recording needs the reference harness (make -C oracle ref)")
            self.new[key] = {"inputs": np.array(digest), **got}
            return got
        rec = {k.split("/", 1)[1]: v for k, v in self.recorded.items() if k.split("/", 1)[0] == key}
        assert rec, f"{key}: no answers of the reference harness recorded in {os.path.relpath(REF_ANSWERS, ROOT)}"
        assert str(rec.pop("inputs")) == digest, f"{key}: the inputs differ from those the reference's answers were recorded for"
        if live:
            assert rec.keys() == got.keys() and all(_same(rec[k], got[k]) for k in got), f"{key}: the recorded answers are not what the reference harness says now"
            return got
        return rec

    def save(self):
        if not self.new:
            return
        keep = {k: v for k, v in self.recorded.items() if k.split("/", 1)[0] not in self.new}
        keep.update({f"{key}/{name}": v for key, d in self.new.items() for name, v in d.items()})
        np.savez_compressed(REF_ANSWERS, **dict(sorted(keep.items())))


@pytest.fixture(scope="session")
def ref_answers(orc):
    r = RefAnswers(orc.ref())
    yield r
    if r.recording:
        r.save()


@pytest.fixture(scope="session")
def golden():
    with open(os.path.join(GOLDEN, "kat.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def built_scene(name: str):
    """(scene, nodes, prims) with the BVH built by the ORACLE's builder (tests only)."""
    from oracle import pyorc
    from tyrant_amd import scenes

    makers = {
        "cornell36": scenes.cornell_box,
        "cornell_soup2k": lambda: scenes.cornell_soup(2000),
        "cornell_soup10k": lambda: scenes.cornell_soup(10000),
        "mesh32": lambda: scenes.mesh_scene(32),
        "mesh128": lambda: scenes.mesh_scene(128),
        "mesh706": lambda: scenes.mesh_scene(706),
        "tyrant_default": scenes.tyrant_default,
        "glass_dof48": lambda: scenes.glass_dof_scene(48),
        "cornell_area_light": scenes.cornell_area_light,
        "cornell_colored": scenes.cornell_colored,
    }
    sc = makers[name]()
    nodes, prims = pyorc.bvh_build(sc.triangles, scenes.triangle_bboxes(sc.triangles))
    return sc, nodes, prims


def bits(a: np.ndarray) -> np.ndarray:
    """float32 array -> uint32 bit patterns (for exact comparisons that treat NaN == NaN)"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="session")
def hip():
    """the product library through its C ABI; GPU tests fail loudly when it is missing"""
    from tyrant_amd import binding

    binding.lib()
    return binding
