"""Per-ray maximum distance (lh_accel_intersect_device_tmax) on the device: S-soup-1M and S-soup-10M, 50 M device-resident fp64 rays,
any hit and closest hit, one process.  Every rate is taken over a window of at least a second of back-to-back calls (device time by
events around the window) after a warm-up; a candidate ALTERNATES with its baseline and each pair is repeated three times, so the
spread of the run is visible next to every ratio.
  (a) cost of the path: the bounded call with every bound +inf  /  lh_accel_intersect_device_ex (the kernels every other launch runs);
      and lh_accel_intersect_device_indexed with the identity list  /  the same baseline: the share of that cost the indexed launch
      brings, which the bounded launch rides on;
  (b) gain: bounds at 1 %, 5 % and 25 % of the scene's diagonal  /  the unbounded call;
  (c) the shadow-pass pattern: closest hit, compact() the hits, bounded any hit on the listed rays (bounds: 5 % of the diagonal)  /
      the same with an unbounded closest-hit second pass on the list that the caller filters with t < tmax.
Bounds are in units of t (multiples of |dir|): a fraction of the diagonal divided by the ray's |dir|.  The answers of every bounded
call are checked against the unbounded records filtered with t < tmax.  With statistics on, one any-hit pass per bound also reports
node visits and triangles through the filter (the pruning itself, on S-soup-1M).
    python tools/tmax_batches.py [nrays] [scenes: 1m,10m] [repeats] [window seconds]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lucille_amd as la  # noqa: E402
from lucille_amd import scenes  # noqa: E402

nr = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
which = (sys.argv[2] if len(sys.argv) > 2 else "1m,10m").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
window = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
NTRI = {"1m": 1_000_000, "10m": 10_000_000}


def window_rate(fn, rays):
    """Mrays/s of fn over >= `window` seconds of back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    k = max(2, int(np.ceil(1.15 * window / max(e0.elapsed_time(e1) * 1e-3, 1e-6))))
    while True:
        e0.record()
        for _ in range(k):
            fn()
        e1.record(); e1.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3
        if dt >= window:
            return rays * k / dt / 1e6
        k = int(np.ceil(k * 1.3 * window / dt))


def pairs(cand, base, rays):
    """[(candidate, baseline) Mrays/s] x reps, alternating; -> dict with the rates, the ratios and their spread"""
    cand(); base()
    c, b = [], []
    for _ in range(reps):
        c.append(window_rate(cand, rays)); b.append(window_rate(base, rays))
    r = [x / y for x, y in zip(c, b)]
    return {"candidate_Mrays": [round(x, 1) for x in c], "baseline_Mrays": [round(x, 1) for x in b], "ratio": [round(x, 4) for x in r],
            "ratio_median": round(float(np.median(r)), 4), "baseline_spread": round((max(b) - min(b)) / float(np.median(b)), 4)}


def outputs(mode):
    if mode == la.MODE_ANY:
        return (torch.zeros(nr, dtype=torch.uint8, device="cuda"),)
    return (torch.zeros(nr, dtype=torch.int32, device="cuda"),) + tuple(torch.zeros(nr, dtype=torch.float64, device="cuda") for _ in range(3))


def check(got, unb, tmax, mode):
    keep = (unb[0] != -1) & (unb[1] < tmax)
    if mode == la.MODE_ANY:
        return bool(torch.equal(got[0] != 0, keep)) and int(got[0].max()) <= 1
    return bool(torch.equal(got[0] != -1, keep) and torch.equal(got[1][keep], unb[1][keep]) and torch.equal(got[0][keep], unb[0][keep])
                and bool((got[1][~keep] == 1e38).all()))


result = {"rays": nr, "repeats": reps, "window_s": window, "scenes": {}}
for sname in which:
    P, idx, st = scenes.soup_triangles(NTRI[sname], 0.005)
    o64, d64, _ = scenes.soup_rays(nr, st)
    diag = float(np.linalg.norm(P.max(0) - P.min(0)))
    dlen = np.linalg.norm(d64, axis=1)
    org = torch.from_numpy(np.ascontiguousarray(o64, np.float64)).cuda(); dr = torch.from_numpy(np.ascontiguousarray(d64, np.float64)).cuda()
    inv_len = torch.from_numpy(1.0 / dlen).cuda()
    del o64, d64
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    inf = torch.full((nr,), float("inf"), dtype=torch.float64, device="cuda")
    bounds = {f: (f * diag) * inv_len for f in (0.01, 0.05, 0.25)}
    unb = acc.intersect_device(org, dr)
    torch.cuda.synchronize()
    res = {"diagonal": diag, "node_bytes": acc.dump_node_bytes(), "hits": int((unb[0] != -1).sum())}
    print("== S-soup-%s: %d triangles, %d rays, %d hits, %d-byte nodes, diagonal %.4f" % (sname.upper(), NTRI[sname], nr, res["hits"], res["node_bytes"], diag), flush=True)
    for mode, mname in ((la.MODE_ANY, "any"), (la.MODE_CLOSEST, "closest")):
        oc, ob = outputs(mode), outputs(mode)
        # (a) the cost of the path
        r = pairs(lambda: acc.intersect_device(org, dr, out=oc, mode=mode, tmax=inf), lambda: acc.intersect_device(org, dr, out=ob, mode=mode), nr)
        r["records_ok"] = bool(all(torch.equal(x, y) for x, y in zip(oc, ob)))
        res["a %s: +inf / unbounded" % mname] = r
        print("(a) %-7s bounds +inf %s  unbounded %s Mrays/s  ratio %s (median %.4f; the baseline's own spread %.4f)  records equal: %s" % (
            mname, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["baseline_spread"], r["records_ok"]), flush=True)
        # ... and of the indexed launch it rides on: the identity list, no bounds
        r = pairs(lambda: acc.intersect_device_indexed(org, dr, out=oc, mode=mode), lambda: acc.intersect_device(org, dr, out=ob, mode=mode), nr)
        r["records_ok"] = bool(all(torch.equal(x, y) for x, y in zip(oc, ob)))
        res["a %s: indexed identity list / unbounded" % mname] = r
        print("(a) %-7s identity list, no bounds %s  unbounded %s Mrays/s  ratio %s (median %.4f)  records equal: %s" % (
            mname, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["records_ok"]), flush=True)
        # (b) the gain
        for f, tm in bounds.items():
            r = pairs(lambda: acc.intersect_device(org, dr, out=oc, mode=mode, tmax=tm), lambda: acc.intersect_device(org, dr, out=ob, mode=mode), nr)
            r["records_ok"] = check(oc, unb, tm, mode)
            r["hits_left"] = int((oc[0] != (0 if mode == la.MODE_ANY else -1)).sum())
            res["b %s: %g of the diagonal / unbounded" % (mname, f)] = r
            print("(b) %-7s bounds %4.0f %% of the diagonal %s  unbounded %s Mrays/s  ratio %s (median %.4f)  hits left %d  records ok: %s" % (
                mname, 100 * f, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["hits_left"], r["records_ok"]), flush=True)
        del oc, ob
    # (c) the shadow-pass pattern
    tm = bounds[0.05]
    first = outputs(la.MODE_CLOSEST); occ = outputs(la.MODE_ANY); second = outputs(la.MODE_CLOSEST)
    lst = la.compact(unb[0], la.SELECT_HIT)

    def cand():
        acc.intersect_device(org, dr, out=first)
        la.compact(first[0], la.SELECT_HIT, out=lst)
        acc.intersect_device(org, dr, out=occ, mode=la.MODE_ANY, index=lst[0], count=lst[1], tmax=tm)

    def base():
        acc.intersect_device(org, dr, out=first)
        la.compact(first[0], la.SELECT_HIT, out=lst)
        acc.intersect_device(org, dr, out=second, index=lst[0], count=lst[1])
        torch.logical_and(second[0] != -1, second[1] < tm, out=shadow)
    shadow = torch.zeros(nr, dtype=torch.bool, device="cuda")
    r = pairs(cand, base, nr)
    hit = unb[0] != -1
    r["records_ok"] = bool(torch.equal((occ[0] != 0)[hit], shadow[hit]))
    res["c shadow pass: bounded any hit / unbounded closest hit + filter"] = r
    print("(c) shadow pass (Mrays/s of the first pass's rays): bounded any hit %s  unbounded closest hit + filter %s  ratio %s (median %.4f)  equal: %s" % (
        r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["records_ok"]), flush=True)
    del first, occ, second, shadow
    # the pruning itself: one counted any-hit pass per bound (statistics make the call synchronous: not timed)
    acc.trace_statistics(True)
    o1 = outputs(la.MODE_ANY)
    for name, tmx in [("+inf", inf)] + [("%g" % f, b) for f, b in bounds.items()]:
        acc.statistics(clear=True)
        acc.intersect_device(org, dr, out=o1, mode=la.MODE_ANY, tmax=tmx)
        s = acc.statistics(clear=True)
        res["visits any, bounds %s" % name] = s
        print("    any hit, bounds %-5s: %.2f node visits, %.2f triangles through the filter per ray, %d hits" % (
            name, s["nodes"] / max(s["rays"], 1), s["tris"] / max(s["rays"], 1), s["hits"]), flush=True)
    acc.trace_statistics(False)
    result["scenes"][sname] = res
    acc.close()
    del org, dr, inv_len, inf, bounds, unb, o1, lst
    torch.cuda.empty_cache()
print(json.dumps(result))
