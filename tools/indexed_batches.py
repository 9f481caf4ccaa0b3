"""Indexed ray batches on the device: S-soup-1M, 20 M device-resident fp64 rays, closest hit and any hit, the configurations
ALTERNATING within each repeat, device time by events around each call:
  (a) the plain lh_accel_intersect_device_ex call on all rays;
  (b) lh_accel_intersect_device_indexed with the identity list (no list, no count);
  (c) the indexed call on a seeded random half of the rays, ids ascending, the count on the device;
  (d) the same half the way a caller does it without the entry point: torch.index_select of the rays, the plain call on the
      gathered rays, index_copy_ of the records into the full arrays;
  (e) lh_accel_compact_device alone over the records of (a), in GB/s of records read (4 bytes a record for the prim array, 16 for
      rec16 -- the line fetched -- and 1 for the any-hit bytes; each is read twice, the figure counts it once).
Mrays/s are of the LISTED rays.  (d) is the yardstick for (c), (a) for (b).  Records of (b), (c), (d) are checked against (a)'s.
    python tools/indexed_batches.py [nrays] [repeats]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lucille_amd as la  # noqa: E402
from lucille_amd import scenes  # noqa: E402

nr = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
P, idx, st = scenes.soup_triangles(1000000, 0.005)
o64, d64, _ = scenes.soup_rays(nr, st)
org = torch.from_numpy(np.ascontiguousarray(o64, np.float64)).cuda(); dr = torch.from_numpy(np.ascontiguousarray(d64, np.float64)).cuda()
acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()

rng = np.random.default_rng(20)
half = np.sort(rng.permutation(nr)[:nr // 2]).astype(np.int64)
half_l = torch.from_numpy(half).cuda()                       # torch's gather / scatter want int64
half_i = half_l.to(torch.int32)
half_n = torch.tensor([half.size], dtype=torch.int32, device="cuda")


def outputs(mode):
    if mode == la.MODE_ANY:
        return (torch.zeros(nr, dtype=torch.uint8, device="cuda"),)
    return (torch.zeros(nr, dtype=torch.int32, device="cuda"),) + tuple(torch.zeros(nr, dtype=torch.float64, device="cuda") for _ in range(3))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def run(cfg, mode, out):
    if cfg == "a":
        return timed(lambda: acc.intersect_device(org, dr, out=out, mode=mode)), nr
    if cfg == "b":
        return timed(lambda: acc.intersect_device_indexed(org, dr, out=out, mode=mode)), nr
    if cfg == "c":
        return timed(lambda: acc.intersect_device_indexed(org, dr, out=out, mode=mode, index=half_i, count=half_n)), half.size

    def today():
        o = org.index_select(0, half_l); d = dr.index_select(0, half_l)
        r = acc.intersect_device(o, d, mode=mode)
        for full, part in zip(out, r):
            full.index_copy_(0, half_l, part)
    return timed(today), half.size


res, ok = {}, {}
for mode, mname in ((la.MODE_CLOSEST, "closest"), (la.MODE_ANY, "any")):
    outs = {c: outputs(mode) for c in "abcd"}
    for c in "abcd":
        run(c, mode, outs[c])                               # warm: allocator, queues
    times = {c: [] for c in "abcd"}
    for r in range(reps):
        for c in "abcd":
            dt, n = run(c, mode, outs[c])
            times[c].append(dt)
    torch.cuda.synchronize()
    ok[mname] = {"b": bool(all(torch.equal(x, y) for x, y in zip(outs["b"], outs["a"]))),
                 "c": bool(all(torch.equal(x[half_l], y[half_l]) for x, y in zip(outs["c"], outs["a"]))),
                 "c untouched": bool(all(int((x != 0).sum()) == int((x[half_l] != 0).sum()) for x in outs["c"])),
                 "d": bool(all(torch.equal(x[half_l], y[half_l]) for x, y in zip(outs["d"], outs["a"])))}
    for c in "abcd":
        n = nr if c in "ab" else half.size
        ts = sorted(times[c])
        res["%s (%s)" % (c, mname)] = {"best_Mrays": round(n / ts[0] / 1e6, 1), "median_Mrays": round(n / ts[len(ts) // 2] / 1e6, 1),
                                       "worst_Mrays": round(n / ts[-1] / 1e6, 1), "ms": [round(x * 1e3, 3) for x in times[c]]}
    # (e) the compaction alone
    recs = {"prim": (outs["a"][0], 4, la.SELECT_HIT)} if mode == la.MODE_CLOSEST else {"occluded": (outs["a"][0], 1, la.SELECT_OCCLUDED)}
    if mode == la.MODE_CLOSEST:
        rec16 = acc.intersect_device(org, dr, records="rec16")[0]
        recs["rec16"] = (rec16, 16, la.SELECT_HIT)
    for name, (r, nbytes, sel) in recs.items():
        pair = la.compact(r, sel)
        ts = sorted(timed(lambda: la.compact(r, sel, out=pair)) for _ in range(reps + 1))
        hit = (r.reshape(nr, -1)[:, 0] != -1) if sel == la.SELECT_HIT else (r != 0)
        exp = torch.nonzero(hit).flatten()
        ok["compact " + name] = bool(int(pair[1].item()) == exp.numel() and torch.equal(pair[0][:exp.numel()].long(), exp))
        res["e (%s)" % name] = {"best_GBs": round(nr * nbytes / ts[0] / 1e9, 1), "median_GBs": round(nr * nbytes / ts[len(ts) // 2] / 1e9, 1),
                                "selected": int(exp.numel()), "ms": [round(x * 1e3, 3) for x in ts]}
    del outs

for k, v in res.items():
    if "best_Mrays" in v:
        print("%-16s best %7.1f  median %7.1f  worst %7.1f Mrays/s of the listed rays   calls (ms) %s" % (
            k, v["best_Mrays"], v["median_Mrays"], v["worst_Mrays"], " ".join("%.2f" % x for x in v["ms"])))
    else:
        print("%-16s best %7.1f  median %7.1f GB/s of records read, %d of %d selected   calls (ms) %s" % (
            k, v["best_GBs"], v["median_GBs"], v["selected"], nr, " ".join("%.3f" % x for x in v["ms"])))
ratio = {}
for m in ("closest", "any"):
    ratio["b / a (%s)" % m] = round(res["b (%s)" % m]["median_Mrays"] / res["a (%s)" % m]["median_Mrays"], 3)
    ratio["c / d (%s)" % m] = round(res["c (%s)" % m]["median_Mrays"] / res["d (%s)" % m]["median_Mrays"], 3)
    ratio["c / a (%s)" % m] = round(res["c (%s)" % m]["median_Mrays"] / res["a (%s)" % m]["median_Mrays"], 3)
print("ratios (medians of %d, same run):" % reps, ratio, " records:", ok)
print(json.dumps({"rays": nr, "repeats": reps, "results": res, "ratios": ratio, "records_ok": ok}))
acc.close()
