"""Host time per call of an entry that runs on the caller's stream: the wall time of CALLS back-to-back calls on one stream, ending
in one synchronise, on work so small that the kernel is negligible -- what is timed is the entry's host path (device scope, the
stream's or the pass's event, launch, record).  By default tyr_query_closest with n = 256 rays on the Cornell box's 36 triangles
(QueryLaunch); with --filters tyr_denoise, tyr_temporal, tyr_svgf, tyr_taa and tyr_allocate_samples on a 16 x 8 frame
(FilterLaunch), taking turns per repeat.  Prints one JSON line per entry; run it in turns on two builds (TYRANT_HIP_LIBRARY
names the other one) to compare them, as profiles/query_host_path_ab.txt and profiles/filter_host_path_ab.txt record.

    python tools/query_host_path.py [--filters] [--calls 2000] [--repeats 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime in the process, see tests/conftest.py)

import numpy as np  # noqa: E402

from tyrant_amd import binding, scenes  # noqa: E402

N = 256
W, H = 16, 8


def query_entries(g, L, h, plane):
    g.build_upload(scenes.cornell_box().triangles)
    o, d, t, prim = plane(N, 3, -40, 40), plane(N, 3, -1, 1), plane(N, 1), plane(N, 1)
    return {"tyr_query_closest": lambda: L.tyr_query_closest(g.h, N, o, d, None, 0, t, prim, None, None, h)}


def filter_entries(g, L, h, plane):
    n = W * H
    accum, alb, nrm, z, m, pdz, color = plane(n, 4, 1, 4), plane(n, 3), plane(n, 3), plane(n, 1, 10, 13), plane(n, 2, -1.5, 1.5), plane(n, 1, 10, 13), plane(n, 4)
    out, aux, err, spp = plane(n, 4), plane(n, 1), plane(n, 1), plane(n, 1)
    din, tin = binding.DenoiseIn(accum, alb, nrm, z), binding.TemporalIn(accum, alb, nrm, z, m, pdz)
    sin, ain = binding.SvgfIn(accum, alb, nrm, z, m, pdz), binding.TaaIn(color, z, m, pdz)
    prm = binding.AllocateParams(4 * n, 1, 8)
    return {
        "tyr_denoise": lambda: L.tyr_denoise(g.h, C.byref(din), None, out, h),
        "tyr_temporal": lambda: L.tyr_temporal(g.h, C.byref(tin), None, out, aux, h),
        "tyr_svgf": lambda: L.tyr_svgf(g.h, C.byref(sin), None, out, aux, h),
        "tyr_taa": lambda: L.tyr_taa(g.h, C.byref(ain), None, out, h),
        "tyr_allocate_samples": lambda: L.tyr_allocate_samples(g.h, err, C.byref(prm), spp, None, h),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", action="store_true")
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    g = binding.Renderer(W, H, 1024) if args.filters else binding.Renderer(64, 64, 4096)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    keep = []  # (the tensors behind the addresses)

    def plane(n, k, lo=0.0, hi=1.0):
        """the address of n x k seeded float32 values on the device"""
        keep.append(torch.from_numpy(rng.uniform(lo, hi, (n, k)).astype(np.float32)).to(dev))
        return keep[-1].data_ptr()

    stream = torch.cuda.Stream(dev)
    entries = (filter_entries if args.filters else query_entries)(g, g.L, stream.cuda_stream, plane)
    walls = {k: [] for k in entries}
    for rep in range(args.repeats + 1):  # one warm-up
        for name, call in entries.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                rc = call()
                if rc:
                    raise binding.TyrError(rc, name)
            stream.synchronize()
            if rep:
                walls[name].append((time.perf_counter() - t0) * 1e3)
    assert g.query_error() == 0
    g.close()
    for name, w in walls.items():
        print(json.dumps({"library": os.path.relpath(binding.LIB_PATH, ROOT), "entry": name, "calls": args.calls, "n": W * H if args.filters else N,
                          "wall_ms": [round(x, 3) for x in w], "us_per_call_median": round(float(np.median(w)) * 1e3 / args.calls, 3)}))


if __name__ == "__main__":
    main()
