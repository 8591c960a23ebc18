#!/usr/bin/env python3
"""tests/fuzz_primary_overlap.py [n] [seed] -- tests/fuzz_parity.py's random cases (scenes, frame sizes, pixel shards up to eight
ranks, queue sizes whose top-ups wrap the start position anywhere, moved cameras, launch-shape knobs; every one compared with the
oracle as that script does) with the knobs of the top-up in two parts drawn on top, from a generator of this
script's own: primary_overlap, overlap_trace_blocks 3..5, window_inset 0..8 and overlap_min_new = 0, without which queues of this
size never split.  Half of the cases are steered to where the split can run -- a pinhole camera, merged traversal launches --
the others stay as drawn.  Prints one line per case, with the top-ups it launched in two parts and the rays its second part had
to trace itself, then the failures and how many cases split and strayed.  tests/test_primary_overlap.py runs a seeded slice."""
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_parity  # noqa: E402
from tyrant_amd import binding  # noqa: E402


def draw_case(rng, own, case=0):
    """fuzz_parity's case `case` of `rng`, unchanged in what it draws there, with the split's knobs from `own`"""
    c = fuzz_parity.draw_case(rng, case)
    c["knobs"].update(primary_overlap=int(own.choice([1, 1, 1, 0])), overlap_trace_blocks=int(own.integers(3, 6)), overlap_min_new=0, window_inset=int(own.choice([0, 0, 0, 2, 5, 8])))
    if own.random() < 0.5:
        c["cam"] = dataclasses.replace(c["cam"], lensRadius=0.0)
        c["knobs"]["merge_trace"] = 1
    return c


def run_case(c):
    """fuzz_parity.run_case, and what the ctx's window record says when the case closes it: (ok, why, line, splits, strays)"""
    seen = {}
    close = binding.Renderer.close

    def closing(self):
        try:
            seen.update(self.primary_window())
        finally:
            close(self)

    binding.Renderer.close = closing
    try:
        ok, why, line = fuzz_parity.run_case(c)
    finally:
        binding.Renderer.close = close
    splits, strays = seen.get("splits", 0), seen.get("strays", 0)
    if c["knobs"]["primary_overlap"] == 0 and splits:
        ok, why = False, why + " split with primary_overlap 0"
    if c["knobs"]["window_inset"] == 0 and strays:
        ok, why = False, why + f" {strays} rays outside the un-inset window entered the tree"
    if not ok and "FAIL" not in line:
        line += " -> FAIL" + why
    return ok, why, f"{line} [splits {splits} strays {strays}]", splits, strays


def main(argv):
    n_cases = int(argv[1]) if len(argv) > 1 else 12
    seed = int(argv[2]) if len(argv) > 2 else 1
    rng, own = np.random.default_rng(seed), np.random.default_rng([seed, 28])
    bad = split = strayed = 0
    for case in range(n_cases):
        ok, _, line, splits, strays = run_case(draw_case(rng, own, case))
        bad += not ok
        split += splits > 0
        strayed += strays > 0
        print(line, flush=True)
    print(f"cases that split: {split}, of them with strays: {strayed}")
    print("failures:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
