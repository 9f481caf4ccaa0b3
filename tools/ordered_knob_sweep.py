"""Sweep of the regroup threshold ("min_active") and the triangle pass's batch ("tri_batch") on an ORDERED ray dump (lucille_amd/csrc/lh_order.h), in ONE
process: the same accelerator, the same rays, the settings alternating launch by launch through set_param, event times, every setting's records compared
bit for bit with the first's.  python tools/ordered_knob_sweep.py [nrays] [rounds] [mode] [min_actives] [tri_batches] [ntri]
nrays: rays of the dump (default 100000000: the headline's); rounds: launches per setting (default 7; a round runs every setting once, in turn); mode:
closest (default) or any; min_actives / tri_batches: comma lists (default 24,32,40,48,56 and 8,12,16,20,24: the grid behind LH_ORDERED_* in
profiles/ordered_walk.md); ntri: triangles of the soup (default 1000000).
The base pair (24, 8: LH_DUMP_MIN_ACTIVE / LH_DUMP_TRI_BATCH, the pair an ordered dump runs with when the caller has set no knob) is always part of the
grid.  Per setting: min / median / max ms; "wins": its median is below the base pair's by more than the base pair's own spread (max - min).  A caller's
knob holds for every dump of the accelerator, ordered ones included (lh_query.hip lh_launch), which is what makes the sweep possible without a rebuild."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import lucille_amd as la
from lucille_amd import binding, scenes
nr = int(sys.argv[1]) if len(sys.argv) > 1 else 100000000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
mode = la.MODE_ANY if len(sys.argv) > 3 and sys.argv[3] == "any" else la.MODE_CLOSEST
mas = [int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else "24,32,40,48,56").split(",")]
tbs = [int(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "8,12,16,20,24").split(",")]
ntri = int(sys.argv[6]) if len(sys.argv) > 6 else 1000000
BASE = (24, 8)
grid = [BASE] + [(m, t) for m in mas for t in tbs if (m, t) != BASE]
P, idx, st = scenes.soup_triangles(ntri, 0.005)
ho, hd, _ = scenes.soup_rays(nr, st)
o = torch.from_numpy(ho).cuda(); d = torch.from_numpy(hd).cuda()
del ho, hd
acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
acc.set_param("dump_order_min", 1); acc.set_param("dump_order", 1)
print("%s, %d triangles, %d rays, %s hit, %d rounds over %d settings" % (binding.library_path(), ntri, nr, "any" if mode == la.MODE_ANY else "closest", rounds, len(grid)), flush=True)


def bits(out):
    return [x.view(torch.int64) if x.dtype == torch.float64 else x for x in out]


def launch(pair, out=None):
    acc.set_param("min_active", pair[0]); acc.set_param("tri_batch", pair[1])
    return acc.intersect_device(o, d, out=out, mode=mode)


ref = tuple(x.clone() for x in launch(BASE))          # warm-up: the workspace; and the records every setting must repeat
out = launch(BASE)
torch.cuda.synchronize()
assert acc.order_statistics(clear=True)["dumps"] == 2
ms = {p: [] for p in grid}; equal = {p: True for p in grid}
for r in range(rounds):
    for p in grid:
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); launch(p, out); e1.record(); torch.cuda.synchronize()
        ms[p].append(e0.elapsed_time(e1))
        equal[p] = equal[p] and all(torch.equal(a, b) for a, b in zip(bits(out), bits(ref)))
base_med, base_spread = statistics.median(ms[BASE]), max(ms[BASE]) - min(ms[BASE])
print("base (%d, %d): %.3f / %.3f / %.3f ms, spread %.3f ms" % (BASE + (min(ms[BASE]), base_med, max(ms[BASE]), base_spread)))
for p in grid:
    med = statistics.median(ms[p])
    print("min_active %2d tri_batch %2d: %8.3f / %8.3f / %8.3f ms   %+6.2f %%   records equal: %s%s" % (
        p[0], p[1], min(ms[p]), med, max(ms[p]), 100.0 * (base_med / med - 1.0), equal[p], "   wins" if base_med - med > base_spread else ""), flush=True)
best = min(grid, key=lambda p: statistics.median(ms[p]))
print("best median: (%d, %d) %.3f ms against the base's %.3f ms" % (best + (statistics.median(ms[best]), base_med)))
