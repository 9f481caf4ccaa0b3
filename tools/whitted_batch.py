"""The refraction chain for a caller's batch of hit records (lh_accel_whitted_device, the defaults: eps 1e-7, eta 1.33, depth 8) on two
inputs, a seeded 1024 x 512 light probe as the accelerator's environment, one process:
  S-soup-1M  -- 1 M soup triangles, `--rays` rays of the synthetic dump and their closest-hit records;
  config 5   -- the AO example scene (tests/golden/ao_c1.npz) tessellated `--tess` times, the primary rays of a `--size`^2 frame.
Every rate is M chain rays/s (the rays of depths 1 .. 8 the chain traces, counted once by the library's statistics) over a window of at
least `--window` seconds of back-to-back calls (device time by events around the window) after a warm-up; the candidate ALTERNATES with
its baseline and each pair is repeated `--repeats` times, so the spread of the run stands next to the ratio.
  candidate: whitted_device -- one bounce kernel and one listed closest-hit launch per depth, lists and counts on the device;
  baseline:  the same chain by hand through public calls -- per depth the alive ids as a torch tensor, lh_accel_state_build_device on
             their gathered records, the bounce as torch operations (one kernel per fp64 operation: nothing contracted), the rays
             scattered to their ids, intersect_device with that id list, environment_device on the rays that left.
The two answers (bounces, end rays, colours) are compared bit for bit.
    python tools/whitted_batch.py [--rays 4000000] [--size 1024] [--tess 8] [--scenes soup,c5] [--repeats 3] [--window 1.0] [--out profiles/whitted_batch.txt]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lucille_amd as la  # noqa: E402
from lucille_amd import scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4_000_000)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--tess", type=int, default=8)
ap.add_argument("--scenes", default="soup,c5")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=1.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []
CUT = -0x80000000          # LH_WHITTED_CUT as int32 bits
NORM_MIN = float(np.float32(1.0e-17))


def say(s):
    print(s, flush=True); lines.append(s)


def window_rate(fn, rays):
    """M rays/s of fn over >= args.window seconds of back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    k = max(2, int(np.ceil(1.15 * args.window / max(e0.elapsed_time(e1) * 1e-3, 1e-6))))
    while True:
        e0.record()
        for _ in range(k):
            fn()
        e1.record(); e1.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3
        if dt >= args.window:
            return rays * k / dt / 1e6
        k = int(np.ceil(k * 1.3 * args.window / dt))


def pairs(cand, base, rays):
    cand(); base()
    c, b = [], []
    for _ in range(args.repeats):
        c.append(window_rate(cand, rays)); b.append(window_rate(base, rays))
    r = [x / y for x, y in zip(c, b)]
    return {"candidate_Mrays": [round(x, 1) for x in c], "baseline_Mrays": [round(x, 1) for x in b], "ratio": [round(x, 4) for x in r],
            "ratio_median": round(float(np.median(r)), 4), "baseline_spread": round((max(b) - min(b)) / float(np.median(b)), 4),
            "candidate_spread": round((max(c) - min(c)) / float(np.median(c)), 4)}


def scene(name):
    """-> (accelerator, org, dr, description)"""
    if name == "soup":
        P, idx, st = scenes.soup_triangles(1_000_000, 0.005)
        o, d, _ = scenes.soup_rays(args.rays, st)
        acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
        return acc, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), "S-soup-1M, %d rays of the dump" % args.rays
    g = np.load(os.path.join(ROOT, "tests", "golden", "ao_c1.npz"))
    acc = la.HipAccel(0); ntri = 0
    for k in range(int(g["ngeoms"])):
        P, I = scenes.tessellate(g["pos%d" % k], g["idx%d" % k], args.tess)
        ntri += I.shape[0] // 3
        acc.add_mesh(P, I); del P, I
    acc.commit(); acc.wait_exact()
    c = g["camera"]
    cam = la.Camera.make(args.size, args.size, c[16], c[:16], int(c[19]))
    org, dr = acc.primary_rays(cam, 0, 0, args.size, args.size, 1)
    return acc, org, dr, "config-5 scene (%d triangles), primary rays of a %d^2 frame" % (ntri, args.size)


def bounce_torch(P, n, I, eps, eta):
    """lh_whitted.h's bounce, one torch kernel per fp64 operation"""
    cos1 = (I[:, 0] * n[:, 0] + I[:, 1] * n[:, 1]) + I[:, 2] * n[:, 2]
    ent = cos1 < 0.0
    c = torch.where(ent, -cos1, cos1)
    e = torch.where(ent, torch.full_like(cos1, 1.0 / eta), torch.full_like(cos1, eta))
    N = torch.where(ent[:, None], n, -n)
    coeff = 1.0 - (e * e) * (1.0 - c * c)
    tir = coeff <= 0.0
    s = (cos1.float() * 2.0).double()
    Rt = I - n * s[:, None]
    q = e * c - torch.sqrt(torch.where(tir, torch.zeros_like(coeff), coeff))
    Rr = q[:, None] * N + e[:, None] * I
    R = torch.where(tir[:, None], Rt, Rr)
    n2 = (R[:, 0] * R[:, 0] + R[:, 1] * R[:, 1]) + R[:, 2] * R[:, 2]
    big = n2 > NORM_MIN
    r = 1.0 / torch.sqrt(torch.where(big, n2, torch.ones_like(n2)))
    R = torch.where(big[:, None], R * r[:, None], R)
    return P + eps * R, R


result = {"repeats": args.repeats, "window_s": args.window, "map": [512, 1024], "scenes": {}}
sky = np.random.default_rng(3).uniform(0.1, 2.0, (512, 1024, 4)).astype(np.float32)
p = la.WhittedParams()
for sname in args.scenes.split(","):
    acc, org, dr, what = scene(sname)
    acc.set_environment((1.0, 0.5, 2.0), sky)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    n = int(org.shape[0]); nhit = int((rec[0] != -1).sum())
    dev = org.device
    out_c = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.float64, device=dev),
             torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev))
    out_h = tuple(torch.empty_like(x) for x in out_c)
    ray_o = torch.empty((n, 3), dtype=torch.float64, device=dev); ray_d = torch.empty_like(ray_o)
    rec_h = tuple(torch.empty_like(x) for x in rec)
    state = torch.empty((n, la.STATE_DOUBLES), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fill(out):
        out[0].fill_(0x5A5A5A5A); out[1].fill_(-1.0); out[2].fill_(-1.0); out[3].fill_(-1.0)

    def candidate():
        acc.whitted_device(org, dr, rec, p, out=out_c)

    def by_hand():
        b, eo, ed, rgb = out_h
        prim0 = rec[0]
        b[:] = torch.where(prim0 != -1, b, torch.full_like(b, -1)); rgb[prim0 == -1] = 0.0
        ids = torch.nonzero(prim0 != -1).squeeze(1).int()
        co, cd, cr = org, dr, rec          # the rays and records the alive ids index
        for d in range(1, p.max_depth + 1):
            k = int(ids.numel())
            if k == 0:
                break
            il = ids.long()
            go, gd = co[il].contiguous(), cd[il].contiguous()
            gr = tuple(x[il].contiguous() for x in cr)
            la.binding._check(acc.L.lh_accel_state_build_device(acc.h, k, C.c_void_p(go.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_void_p(gr[0].data_ptr()),
                                                                C.c_void_p(gr[1].data_ptr()), C.c_void_p(gr[2].data_ptr()), C.c_void_p(gr[3].data_ptr()),
                                                                C.c_void_p(state.data_ptr()), stream), "lh_accel_state_build_device")
            st = state[:k]
            no, nd = bounce_torch(st[:, 0:3], st[:, 6:9], st[:, 20:23], p.eps, p.eta)
            ray_o[il] = no; ray_d[il] = nd; eo[il] = no; ed[il] = nd
            acc.intersect_device(ray_o, ray_d, out=rec_h, index=ids)
            miss = rec_h[0][il] == -1
            gone = il[miss]
            b[gone] = d
            if int(gone.numel()):
                rgb[gone] = acc.environment_device(nd[miss].contiguous())
            if d == p.max_depth:
                b[il[~miss]] = d | CUT; rgb[il[~miss]] = 0.0
            ids = ids[~miss]
            co, cd, cr = ray_o, ray_d, rec_h

    fill(out_c); fill(out_h)
    acc.trace_statistics(True); acc.statistics(clear=True); candidate(); s = acc.statistics(clear=True); acc.trace_statistics(False)
    chain = int(s["rays"])
    by_hand(); torch.cuda.synchronize()
    hit = rec[0] != -1
    equal = bool(torch.equal(out_c[0], out_h[0]) and torch.equal(out_c[3].view(torch.int32), out_h[3].view(torch.int32))
                 and torch.equal(out_c[1][hit].view(torch.int64), out_h[1][hit].view(torch.int64))
                 and torch.equal(out_c[2][hit].view(torch.int64), out_h[2][hit].view(torch.int64)))
    cut = int(((out_c[0] != -1) & (out_c[0] < 0)).sum())
    say("== %s: %d hits of %d rays, %d chain rays (%.2f per hit), %d chains cut at depth %d; light probe 1024 x 512" % (
        what, nhit, n, chain, chain / max(nhit, 1), cut, p.max_depth))
    r = pairs(candidate, by_hand, chain)
    r["answers_equal"] = equal
    say("whitted_device %s  by hand %s M chain rays/s  ratio %s (median %.4f; spread of the baseline %.4f, of the candidate %.4f)  answers equal: %s" % (
        r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["baseline_spread"], r["candidate_spread"], equal))
    say("%.2f node visits per chain ray" % (s["nodes"] / max(chain, 1)))
    result["scenes"][sname] = {"what": what, "rays": n, "hits": nhit, "chain_rays": chain, "cut": cut, **r}
    acc.close(); del org, dr, rec, out_c, out_h, ray_o, ray_d, rec_h, state
    torch.cuda.empty_cache()
say(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
