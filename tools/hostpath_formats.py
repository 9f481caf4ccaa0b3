"""Host batch path by format: S-soup-1M, 20 M rays in pageable host arrays, {f64 -> f64, f32 -> f64, f64 -> rec16, f32 -> rec16}
x {closest, any} through lh_accel_intersect_host (f64 -> f64: the fp64 entry point itself) and lh_accel_intersect_host_ex, the
configurations ALTERNATING within each of 5 repeats (benchlegs/hostpath.py's protocol: caller-owned, already-touched arrays, the
first call warms the ring).  Prints the best, median and spread of the repeats per configuration, the ratios of the new formats
to the fp64 path of the same run, and one JSON line.  Records of every configuration are checked against the fp64 path's (rec16:
its fp64 records rounded to fp32).
    python tools/hostpath_formats.py [nrays] [repeats] [configs]
configs: a comma-separated subset of the six names below (e.g. "f32 rec16 closest"), for a timeline of those alone
(rocprofv3 --kernel-trace --memory-copy-trace --stats -- python tools/hostpath_formats.py 20000000 2 "f32 rec16 closest")."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import lucille_amd as la  # noqa: E402
from lucille_amd import binding, scenes  # noqa: E402

nr = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
P, idx, st = scenes.soup_triangles(1000000, 0.005)
o64, d64, _ = scenes.soup_rays(nr, st)
o64 = np.ascontiguousarray(o64, np.float64); d64 = np.ascontiguousarray(d64, np.float64)
o32 = o64.astype(np.float32); d32 = d64.astype(np.float32)
acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
L = acc.L

hp = np.zeros(nr, np.uint32); ht = np.zeros(nr); hu = np.zeros(nr); hv = np.zeros(nr)
rec = binding._rec16_host(nr); rec[:] = 0
occ = np.zeros(nr, np.uint8)


def run(name):
    rays, fmt_out, mode = name.split()
    o, d = (o32, d32) if rays == "f32" else (o64, d64)
    rf = binding.RAYS_F32 if rays == "f32" else binding.RAYS_F64
    m = la.MODE_ANY if mode == "any" else la.MODE_CLOSEST
    t0 = time.perf_counter()
    if rays == "f64" and fmt_out == "f64":           # the fp64 entry point itself
        if m == la.MODE_ANY:
            rc = L.lh_accel_intersect_host(acc.h, nr, o.ctypes.data, d.ctypes.data, None, None, None, None, occ.ctypes.data, m)
        else:
            rc = L.lh_accel_intersect_host(acc.h, nr, o.ctypes.data, d.ctypes.data, hp.ctypes.data, ht.ctypes.data, hu.ctypes.data,
                                           hv.ctypes.data, None, m)
    elif m == la.MODE_ANY:
        rc = L.lh_accel_intersect_host_ex(acc.h, nr, o.ctypes.data, d.ctypes.data, rf, binding.REC_F64, None, None, None, None,
                                          occ.ctypes.data, m)
    elif fmt_out == "rec16":
        rc = L.lh_accel_intersect_host_ex(acc.h, nr, o.ctypes.data, d.ctypes.data, rf, binding.REC16, rec.ctypes.data, None, None, None,
                                          None, m)
    else:
        rc = L.lh_accel_intersect_host_ex(acc.h, nr, o.ctypes.data, d.ctypes.data, rf, binding.REC_F64, hp.ctypes.data, ht.ctypes.data,
                                          hu.ctypes.data, hv.ctypes.data, None, m)
    dt = time.perf_counter() - t0
    assert rc == 0, L.lh_last_error()
    return dt


CONFIGS = ["f64 f64 closest", "f32 f64 closest", "f64 rec16 closest", "f32 rec16 closest", "f64 f64 any", "f32 f64 any"]
if len(sys.argv) > 3:
    CONFIGS = [c.strip() for c in sys.argv[3].split(",") if c.strip()]
    assert all(len(c.split()) == 3 for c in CONFIGS), CONFIGS
times = {c: [] for c in CONFIGS}
run("f64 f64 closest"); run("f64 f64 any")          # the ring and the copy threads
for r in range(reps):
    for c in CONFIGS:
        times[c].append(run(c))

# correctness of what the last repeats left: rays here are fp64 widenings of nothing -- the fp32 rays are ROUNDED fp64 rays, so
# f32 configurations are checked against the fp64 path on their widened rays, once, outside the timing
ok = {}
run("f64 f64 closest"); ref = (hp.copy(), ht.copy(), hu.copy(), hv.copy())
run("f64 rec16 closest")
ok["f64 rec16"] = bool(np.array_equal(rec[:, 0], ref[0]) and all(np.array_equal(rec[:, k].view(np.float32), ref[k].astype(np.float32)) for k in (1, 2, 3)))
run("f64 f64 any"); ok["f64 any == hits"] = bool(np.array_equal(occ.astype(bool), ref[0] != 0xFFFFFFFF))
ow, dw = o32.astype(np.float64), d32.astype(np.float64)
L.lh_accel_intersect_host(acc.h, nr, ow.ctypes.data, dw.ctypes.data, hp.ctypes.data, ht.ctypes.data, hu.ctypes.data, hv.ctypes.data, None, 0)
refw = (hp.copy(), ht.copy(), hu.copy(), hv.copy())
run("f32 rec16 closest")
ok["f32 rec16"] = bool(np.array_equal(rec[:, 0], refw[0]) and all(np.array_equal(rec[:, k].view(np.float32), refw[k].astype(np.float32)) for k in (1, 2, 3)))
run("f32 f64 closest")
ok["f32 f64"] = bool(all(np.array_equal(a, b) for a, b in zip((hp, ht, hu, hv), refw)))

res = {}
for c in CONFIGS:
    ts = sorted(times[c])
    res[c] = {"best_Mrays": round(nr / ts[0] / 1e6, 1), "median_Mrays": round(nr / ts[len(ts) // 2] / 1e6, 1),
              "worst_Mrays": round(nr / ts[-1] / 1e6, 1), "ms": [round(x * 1e3, 2) for x in times[c]]}
    print("%-18s best %7.1f  median %7.1f  worst %7.1f Mrays/s   calls (ms) %s" % (c, res[c]["best_Mrays"], res[c]["median_Mrays"],
                                                                                 res[c]["worst_Mrays"], " ".join("%.1f" % (x * 1e3) for x in times[c])))
ratio = {}
if "f32 rec16 closest" in res and "f64 f64 closest" in res:
    ratio["f32 rec16 / f64 closest"] = round(res["f32 rec16 closest"]["best_Mrays"] / res["f64 f64 closest"]["best_Mrays"], 3)
if "f32 f64 any" in res and "f64 f64 any" in res:
    ratio["f32 / f64 any"] = round(res["f32 f64 any"]["best_Mrays"] / res["f64 f64 any"]["best_Mrays"], 3)
print("ratios (best of %d, same run):" % reps, ratio, " records:", ok)
print(json.dumps({"rays": nr, "repeats": reps, "results": res, "ratios": ratio, "records_ok": ok}))
acc.close()
