"""Host time per query call: the wall time of CALLS back-to-back tyr_query_closest calls of n = 256 rays on one stream, ending in
one synchronise, on the Cornell box's 36 triangles -- the kernel is negligible, what is timed is the entry's host path (device scope, stream
entry, ticket clear, launch, `done` record).  Prints one JSON line; run it in turns on two builds (TYRANT_HIP_LIBRARY names the
other one) to compare them, as profiles/query_host_path_ab.txt records.

    python tools/query_host_path.py [--calls 2000] [--repeats 5]
"""
from __future__ import annotations

import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    g = binding.Renderer(64, 64, 4096)
    g.build_upload(scenes.cornell_box().triangles)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    o = torch.from_numpy(rng.uniform(-40, 40, (N, 3)).astype(np.float32)).to(dev)
    d = torch.from_numpy(rng.normal(size=(N, 3)).astype(np.float32)).to(dev)
    t, prim = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    h, L = stream.cuda_stream, g.L
    args_c = (g.h, N, o.data_ptr(), d.data_ptr(), None, 0, t.data_ptr(), prim.data_ptr(), None, None, h)
    walls = []
    for rep in range(args.repeats + 1):  # one warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            rc = L.tyr_query_closest(*args_c)
            if rc:
                raise binding.TyrError(rc, "tyr_query_closest")
        stream.synchronize()
        if rep:
            walls.append((time.perf_counter() - t0) * 1e3)
    assert g.query_error() == 0
    g.close()
    print(json.dumps({"library": os.path.relpath(binding.LIB_PATH, ROOT), "calls": args.calls, "n": N, "wall_ms": [round(w, 3) for w in walls],
                      "us_per_call_median": round(float(np.median(walls)) * 1e3 / args.calls, 3)}))


if __name__ == "__main__":
    main()
