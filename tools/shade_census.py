#!/usr/bin/env python3
"""tools/shade_census.py [c2|c3] -- diagnostic build only (make tagged TAG=census EXTRA_HIPFLAGS=-DTYR_SHADE_CENSUS, loaded through
TYRANT_HIP_LIBRARY): what the three wave-wide sections of a k_shade tile are asked for, per iteration of one render at 1080p, 8 spp
-- the lanes that request the atmosphere for themselves (sun samples, misses) or for their ghost, the shadow rays that await the
sphere and root-box test, and the waves that hold at least one of each: the passes the lane path runs, against the passes the
requests fill when they are gathered across the tile's four waves (TYR_TUNE_SHADE_DENSE).  The counted launch is chosen by
TYR_CENSUS_ITER (the iteration since tyr_create), so every iteration is counted on a ctx of its own."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tyrant_amd import binding, scenes  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
sc = {"c2": lambda: scenes.cornell_soup(10000), "c3": lambda: scenes.mesh_scene(706)}[wl]()
nodes, prims = binding.bvh_build(sc.triangles)
W, H, SPP = 1920, 1080, 8
print(f"{wl}, {W}x{H}, {SPP} spp, queue = all primaries; per iteration of one render (tile = 256 slots = 4 waves)")
print("it   tiles  wave-tiles  valid lanes   sun req  miss req ghost req shadow cand | waves with >= 1: own atmo   ghost  shadow | dense passes: atmo shadow | passes saved  of wave-tiles")
tot_saved = tot_waves = 0
for it in range(8):
    os.environ["TYR_CENSUS_ITER"] = str(it)
    r = binding.Renderer(W, H, W * H * SPP, flags=binding.TYR_FLAG_TRIANGLE_MATERIALS if sc.triangle_materials else 0)
    r.load_scene(sc, nodes, prims)
    r.render(SPP)
    d = r.counters()["debug"]
    r.close()
    valid, sun, miss, ghost, shadow, w_own, w_ghost, w_shadow, w_valid, tiles, p_atmo, p_shadow = (int(v) for v in d[:12])
    if tiles == 0:
        continue
    saved = (w_own + w_ghost - p_atmo) + (w_shadow - p_shadow)
    tot_saved += saved
    tot_waves += w_valid
    print(f"{it + 1:2d} {tiles:7d} {w_valid:11d} {valid:12d} {sun:9d} {miss:9d} {ghost:9d} {shadow:11d} | {w_own:24d} {w_ghost:7d} {w_shadow:7d} | {p_atmo:18d} {p_shadow:6d} | {saved:12d} {saved / max(w_valid, 1):12.3f}")
    print(f"     per valid lane: sun {sun / valid:.3f} miss {miss / valid:.3f} ghost {ghost / valid:.3f} shadow {shadow / valid:.3f}; waves that run the section: own atmo {w_own / w_valid:.3f} ghost {w_ghost / w_valid:.3f} shadow {w_shadow / w_valid:.3f}")
print(f"ceiling: {tot_saved} section passes saved over {tot_waves} wave-tiles = {tot_saved / max(tot_waves, 1):.3f} per wave-tile (a wave-tile runs up to three: own atmosphere, ghost, shadow test)")
