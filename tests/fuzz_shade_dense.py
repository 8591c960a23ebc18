#!/usr/bin/env python3
"""tests/fuzz_shade_dense.py [n] [seed] -- tests/fuzz_parity.py's random cases (scenes with and without materials, emissive
triangles and palettes, frame sizes, pixel shards, queue sizes, cameras, suns, launch-shape knobs; every one compared with the
oracle as that script does: iteration and ray counts identical, the last iteration's queues bit for bit, radiance within 1e-5)
with shade_dense (a shade tile's atmosphere requests and shadow tests on dense lanes) drawn on top, from a
generator of this script's own, so that a seed names the same cases as there.  Two cases in three run the dense path; of those,
half are steered to where all of it runs -- fold_spheres, resolve_shadows and retire_sky on, merged traversal launches -- the
others stay as drawn.  A scene with a light list runs the lane path whatever the key says (hip/shade.hip: no dense kernel for it)
and is not counted.  Prints one line per case, then the failures and how many cases ran the dense path."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_parity  # noqa: E402


def draw_case(rng, own, case=0):
    """fuzz_parity's case `case` of `rng`, unchanged in what it draws there, with shade_dense from `own`"""
    c = fuzz_parity.draw_case(rng, case)
    c["knobs"]["shade_dense"] = int(own.choice([1, 1, 0]))
    if c["knobs"]["shade_dense"] and own.random() < 0.5:
        c["knobs"].update(fold_spheres=1, resolve_shadows=1, retire_sky=1, merge_trace=1)
    return c


def main(argv):
    n_cases = int(argv[1]) if len(argv) > 1 else 12
    seed = int(argv[2]) if len(argv) > 2 else 1
    rng, own = np.random.default_rng(seed), np.random.default_rng([seed, 32])
    bad = dense = 0
    for case in range(n_cases):
        c = draw_case(rng, own, case)
        ok, _, line = fuzz_parity.run_case(c)
        bad += not ok
        dense += c["knobs"]["shade_dense"] and not c["sc"].light_list
        print(line, flush=True)
    print(f"cases on the dense path: {dense} of {n_cases}")
    print("failures:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
