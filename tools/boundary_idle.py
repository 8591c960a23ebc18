#!/usr/bin/env python3
"""tools/boundary_idle.py <kernel_trace.csv> [renders=3] -- idle time per kind of kernel boundary in the last `renders` renders of a
`rocprofv3 --kernel-trace` run of tools/stream_probe.py (or bench.py): per render span / busy / idle, the gap (us) behind each kind of
kernel, one column per render, and the idle between the last kernel of a render and the first kernel of the next (whatever runs
in between -- the accumulation buffer's clear, counter updates -- is listed with it)."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
n_renders = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r.get("Grid_Size_X", 0) or 0)) for r in rows)
RENDER = ("k_primary", "k_pad_holes", "k_trace_flat", "k_shade", "k_scan_words", "k_extend_spheres", "k_connect_spheres")


def short(n):
    return n.replace("void ", "").replace("tyr::", "").split("(")[0][:30]


starts = [i for i, k in enumerate(ks) if "k_primary" in k[2] and k[3] > 256][-n_renders:]  # the launch that generates a render's camera rays
renders = []
for i0 in starts:
    i1 = i0
    while i1 + 1 < len(ks) and any(r in ks[i1 + 1][2] for r in RENDER) and not ("k_primary" in ks[i1 + 1][2] and ks[i1 + 1][3] > 256):
        i1 += 1
    renders.append((i0, i1))
gaps = {}
for r, (i0, i1) in enumerate(renders):
    seq = ks[i0 : i1 + 1]
    busy = sum(e - s for s, e, _, _ in seq)
    span = seq[-1][1] - seq[0][0]
    print(f"render {r}: {len(seq)} kernels, span {span / 1e6:.4f} ms, busy {busy / 1e6:.4f} ms, idle {(span - busy) / 1e3:.1f} us")
    for a, b in zip(seq, seq[1:]):
        gaps.setdefault(short(a[2]) + " -> " + short(b[2]), [[] for _ in renders])[r].append((b[0] - a[1]) / 1e3)
print("gap behind each kind of boundary, us (per render: n x mean [min .. max]):")
for k, per in gaps.items():
    print(f"  {k:58s}" + "  ".join(f"{len(v)} x {sum(v) / len(v):5.1f} [{min(v):5.1f} .. {max(v):5.1f}]" if v else "        -        " for v in per))
print("between renders (end of a render's last kernel -> start of the next render's k_primary), us:")
for (_, i1), (j0, _) in zip(renders, renders[1:]):
    between = ks[i1 + 1 : j0]
    inside = sum(e - s for s, e, _, _ in between)
    print(f"  {(ks[j0][0] - ks[i1][1]) / 1e3:7.1f} us, of which kernels in between {inside / 1e3:6.1f} us: " + ", ".join(f"{short(n)} {(e - s) / 1e3:.1f}" for s, e, n, _ in between))
