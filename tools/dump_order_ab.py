"""A/B of ray dumps traced in bin order ("dump_order", lucille_amd/csrc/lh_order.h) against the dumps as given, in ONE process: the same accelerator, the
same rays, set_param("dump_order", 0 / 1) alternating launch by launch.  python tools/dump_order_ab.py [sizes] [pairs] [ntri] [key] [mode]
sizes: comma list of ray counts (default 1000000,4000000,16000000,100000000: the table behind "dump_order_min" in profiles/dump_order.md); pairs:
alternating pairs per size (default 6); ntri: triangles of the soup (default 1000000); key: "dump_order_bits" (default 0: the library's); mode: closest
(default) or any.
Per size: min / median / max ms of either side and the gain of the medians; "on wins" where the slowest ordered launch beats the
fastest given one.  A library given through LH_LIBRARY that has no ordered dumps (the parent's) is timed as given alone: run the tool once with
it and once without for the pairs of profiles/dump_order.md."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import lucille_amd as la
from lucille_amd import binding
from oracle import pyoracle as po
sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1000000,4000000,16000000,100000000").split(",")]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 6
ntri = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
P, idx, org, dr = po.soup(ntri, max(sizes))
acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
has_order = hasattr(binding.lib(), "lh_accel_order_statistics")
if has_order:
    acc.set_param("dump_order_min", 1)
    if len(sys.argv) > 4 and int(sys.argv[4]) > 0:
        acc.set_param("dump_order_bits", int(sys.argv[4]))
mode = la.MODE_ANY if len(sys.argv) > 5 and sys.argv[5] == "any" else la.MODE_CLOSEST
od = torch.from_numpy(org).cuda(); dd = torch.from_numpy(dr).cuda()
print("%s, %d triangles, %d alternating pairs per size, %s hit" % (binding.library_path(), ntri, reps, "any" if mode == la.MODE_ANY else "closest"), flush=True)
for n in sizes:
    o, d = od[:n], dd[:n]
    sides = (0, 1) if has_order else (0,)
    ms = {s: [] for s in sides}; outs = {}
    for s in sides:          # warm-up: allocations, the workspace
        if has_order:
            acc.set_param("dump_order", s)
        outs[s] = acc.intersect_device(o, d, mode=mode)
    torch.cuda.synchronize()
    for _ in range(reps):
        for s in sides:
            if has_order:
                acc.set_param("dump_order", s)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); acc.intersect_device(o, d, out=outs[s], mode=mode); e1.record(); torch.cuda.synchronize(); ms[s].append(e0.elapsed_time(e1))
    line = "%11d rays: given %.3f / %.3f / %.3f ms" % (n, min(ms[0]), statistics.median(ms[0]), max(ms[0]))
    if has_order:
        same = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b) for a, b in zip(outs[0], outs[1]))
        line += "   ordered %.3f / %.3f / %.3f ms   %+.1f %%%s   records equal: %s" % (
            min(ms[1]), statistics.median(ms[1]), max(ms[1]), 100.0 * (statistics.median(ms[0]) / statistics.median(ms[1]) - 1.0),
            "   on wins" if max(ms[1]) < min(ms[0]) else "", same)
    print(line, flush=True)
