"""tools/render_gap_probe.py [steps=200] [profile=1] [mask=10] [queue=N] [knob=value ...] -- where a bench-style step's time goes
outside the kernels, without a profiler: `steps` times set_frame + reset_accum + render (1080p, 8 spp, the C3 mesh), the host
clock around each of the three calls, and -- profile=1, every stage bracketed for it -- the stages' summed time from timings()
in a second pass, so that `ms per step - kernel ms per step` is the time per step in which no stage of ours ran.
mask: the stages the first pass times (bench.py's timed region keeps TYR_K_EXTEND | TYR_K_CONNECT = 10).
The second pass runs with primary_overlap=0: with a top-up in two parts TYR_K_PRIMARY (window part's start to rest part's end) runs
beside TYR_K_EXTEND and the stages' sum would count that time twice."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402

from tyrant_amd import binding, scenes  # noqa: E402

knobs = {k: int(v) for k, v in (a.split("=") for a in sys.argv[1:])}
steps = knobs.pop("steps", 200)
queue = knobs.pop("queue", 1920 * 1080 * 8)
profile = knobs.pop("profile", 1)
mask = knobs.pop("mask", 10)
sc = scenes.mesh_scene(706)
nodes, prims = binding.bvh_build(sc.triangles)
g = binding.Renderer(1920, 1080, queue, flags=1 | (2 if profile else 0))
g.load_scene(sc, nodes, prims)
g.set_tuning(**knobs)


def run(n):
    per = {"set_frame": [], "reset_accum": [], "render": []}
    t_begin = time.perf_counter()
    for _ in range(n):
        t0 = time.perf_counter()
        g.set_frame(1)
        t1 = time.perf_counter()
        g.reset_accum()
        t2 = time.perf_counter()
        g.render(8)
        t3 = time.perf_counter()
        per["set_frame"].append(t1 - t0)
        per["reset_accum"].append(t2 - t1)
        per["render"].append(t3 - t2)
    return (time.perf_counter() - t_begin) / n, per


for _ in range(3):  # code objects loaded, persistent grids sized
    run(1)
if profile:
    g.set_tuning(profile_mask=mask)
g.timings(reset=True)
ms_step, per = run(steps)
tm = g.timings(reset=True)
print(f"{steps} steps, profile={profile} mask={mask}: {ms_step * 1e3:.4f} ms per step; device_error {g.counters()['device_error']}")
for name, v in per.items():
    v = sorted(v)
    print(f"  host clock around {name:12s} median {statistics.median(v) * 1e6:9.1f} us   min {v[0] * 1e6:9.1f}   90 % {v[int(0.9 * (len(v) - 1))] * 1e6:9.1f}")
if profile:
    timed = {k: (v["ms"] / steps, v["launches"] / steps) for k, v in tm.items() if v["launches"]}
    print("  stages timed in this pass (ms per step, launches per step):", {k: (round(a, 4), b) for k, (a, b) in timed.items()})
    # second pass: every stage bracketed, for the kernels' own time per step (the brackets themselves stretch the step, not the stages)
    g.set_tuning(profile_mask=31, primary_overlap=0)  # (stages that follow one another: their sum is the kernels' time)
    g.timings(reset=True)
    ms_all, _ = run(steps)
    tm = g.timings(reset=True)
    busy = sum(v["ms"] for v in tm.values()) / steps
    print(f"  all stages bracketed, primary_overlap=0: {ms_all * 1e3:.4f} ms per step, stages' sum {busy:.4f} ms per step:", {k: round(v["ms"] / steps, 4) for k, v in tm.items() if v["launches"]})
    print(f"  first pass's step - stages' sum = {ms_step * 1e3 - busy:.4f} ms per step with no stage running (boundaries inside the render + between renders + the 33 MB clear)")
