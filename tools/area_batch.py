"""Area lights for a caller's batch of hit records (lh_accel_area_lights_device) on two scenes, S = 1, 4 and 16 samples of L = 1 and 4 lights, one
process:
  S-soup-1M  -- 1 M soup triangles, `--rays` rays of the synthetic dump and their closest-hit records;
  config 5   -- the AO example scene (tests/golden/ao_c1.npz) tessellated `--tess` times, the primary rays of a `--size`^2 frame.
The lights: quads of two emitter triangles on a shell around the hits' box, a tenth of its diagonal wide; light 0 is plain (no flags), the others
carry AREA_FACING | AREA_INVSQ | AREA_PDF.  Every rate is M shadow rays/s (hits x L x S work items) over a window of at least `--window` seconds of
back-to-back calls (device time by events around the window) after a warm-up; the candidate ALTERNATES with its baseline and each pair is repeated
`--repeats` times, so the spread of the run stands next to every ratio.  The candidate is always the fused stage (area_lights_device, "ao_fused" 1):
  (a) / the materialised stage ("ao_fused" 0: rays and bounds in HBM, one bounded any-hit launch, the same resolve);
  (b) / the same by hand: area_light_rays_device (64 bytes of ray, bound and weight per item), a bounded any-hit intersect_device, the masked
      weighted mean and the scatter as torch operations on the device.
(a)'s two answers are compared bit for bit.  With statistics on, one more fused pass reports the items that went through the fix-up queue.
    python tools/area_batch.py [--rays 1000000] [--size 1024] [--tess 8] [--scenes soup,c5] [--repeats 3] [--window 1.0] [--out profiles/area_batch.txt]"""
import argparse
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
ap.add_argument("--rays", type=int, default=1_000_000)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--tess", type=int, default=8)
ap.add_argument("--scenes", default="soup,c5")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=1.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def window_time(fn):
    """seconds per call of fn over >= args.window seconds of back-to-back calls"""
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
            return dt / k
        k = int(np.ceil(k * 1.3 * args.window / dt))


def pairs(cand, base, rays):
    cand(); base()
    c, b = [], []
    for _ in range(args.repeats):
        c.append(rays / window_time(cand) / 1e6); b.append(rays / window_time(base) / 1e6)
    r = [x / y for x, y in zip(c, b)]
    return {"candidate_Mrays": [round(x, 1) for x in c], "baseline_Mrays": [round(x, 1) for x in b], "ratio": [round(x, 4) for x in r],
            "ratio_median": round(float(np.median(r)), 4), "baseline_spread": round((max(b) - min(b)) / float(np.median(b)), 4)}


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


def emitters(L, lo, hi):
    """L quads on a shell around the hits' box -> (table [2 L, 3, 3], the lights)"""
    rng = np.random.default_rng(17)
    c = 0.5 * (lo + hi); r = float(np.linalg.norm(hi - lo))
    tris, lights = [], []
    for l in range(L):
        v = rng.normal(size=3); v /= np.linalg.norm(v)
        v[1] = abs(v[1]) + 0.3                                         # above the scene rather than below it
        p = c + v / np.linalg.norm(v) * r * rng.uniform(0.6, 1.2)
        a = np.cross(v, rng.normal(size=3)); a *= 0.1 * r / np.linalg.norm(a)
        b = np.cross(v, a); b *= 0.1 * r / np.linalg.norm(b)
        tris += [[p, p + a, p + a + b], [p, p + a + b, p + b]]
        lights.append(la.AreaLight(2 * l, 2, tuple(rng.uniform(0.2, 2.0, 3)), 0 if l == 0 else la.AREA_FACING | la.AREA_INVSQ | la.AREA_PDF))
    return np.array(tris), lights


result = {"repeats": args.repeats, "window_s": args.window, "scenes": {}}
for sname in args.scenes.split(","):
    acc, org, dr, what = scene(sname)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    n = int(org.shape[0]); hit = rec[0] != -1; nhit = int(hit.sum())
    Ph = (org + dr * rec[1][:, None])[hit]
    lo, hi = Ph.min(dim=0).values.cpu().numpy(), Ph.max(dim=0).values.cpu().numpy()
    del Ph
    res = {"what": what, "rays": n, "hits": nhit}
    say("== %s: %d hits of %d rays" % (what, nhit, n))
    for L in (1, 4):
        table, ls = emitters(L, lo, hi)
        acc.set_emitters(table)
        rgb_l = torch.tensor([list(x.rgb) for x in ls], dtype=torch.float64, device="cuda")
        for S in (1, 4, 16):
            items = nhit * L * S
            p = la.AreaParams(1.0e-5, 1.0, S)
            out_f = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda"))
            out_m = (torch.empty_like(out_f[0]), torch.empty_like(out_f[1]))

            def fused():
                acc.area_lights_device(org, dr, rec, ls, p, 1, out=out_f)

            def materialised():
                acc.set_param("ao_fused", 0)
                try:
                    acc.area_lights_device(org, dr, rec, ls, p, 1, out=out_m)
                finally:
                    acc.set_param("ao_fused", 1)

            r = pairs(fused, materialised, items)
            r["answers_equal"] = bool(torch.equal(out_f[0], out_m[0]) and torch.equal(out_f[1].view(torch.int32), out_m[1].view(torch.int32)))
            res["L=%d S=%d a fused / materialised" % (L, S)] = r
            say("L = %d S = %2d (a fused / materialised) fused %s  baseline %s M shadow rays/s  ratio %s (median %.4f; the baseline's own spread %.4f)  answers equal: %s" % (
                L, S, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["baseline_spread"], r["answers_equal"]))
            rays_out = acc.area_light_rays_device(org, dr, rec, ls, p, 1)
            hand_occ = torch.empty(n * L * S, dtype=torch.uint8, device="cuda")

            def by_hand():
                slot, nslots, ro, rd, rt, rw = acc.area_light_rays_device(org, dr, rec, ls, p, 1, out=rays_out)
                k = int(nslots.item()) * L * S
                occ = acc.intersect_device(ro[:k], rd[:k], mode=la.MODE_ANY, tmax=rt[:k], out=(hand_occ[:k],))[0]
                open_ = (rt[:k].view(-1, L, S) > 0) & (occ.view(-1, L, S) == 0)
                w = torch.where(open_, rw[:k].view(-1, L, S), torch.zeros((), dtype=torch.float64, device=org.device)).sum(dim=2)
                val = ((w[:, :, None] * rgb_l[None, :, :]).sum(dim=1) / S).float()
                mask = (open_.any(dim=2).int() << torch.arange(L, dtype=torch.int32, device=org.device)[None, :]).sum(dim=1, dtype=torch.int32)
                h = slot != -1
                om = torch.full((n,), -1, dtype=torch.int32, device=org.device); om[h] = mask[slot[h].long()]
                ov = torch.zeros((n, 3), dtype=torch.float32, device=org.device); ov[h] = val[slot[h].long()]
                return om, ov

            r = pairs(fused, by_hand, items)
            om, ov = by_hand()          # torch's sum need not take the list and sample order: masks equal, colours close
            r["masks_equal"] = bool(torch.equal(om, out_f[0]))
            r["largest_relative_colour_difference"] = float(((ov - out_f[1]).abs() / out_f[1].abs().clamp_min(1e-30)).max())
            res["L=%d S=%d b fused / by hand" % (L, S)] = r
            say("L = %d S = %2d (b fused / by hand) fused %s  baseline %s M shadow rays/s  ratio %s (median %.4f; the baseline's own spread %.4f)  masks equal: %s, colours within %.3g (relative)" % (
                L, S, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["baseline_spread"], r["masks_equal"], r["largest_relative_colour_difference"]))
            acc.trace_statistics(True)
            acc.statistics(clear=True); fused(); s = acc.statistics(clear=True); q = int(acc.L.lh_accel_last_retraced(acc.h))
            acc.trace_statistics(False)
            res["L=%d S=%d queue" % (L, S)] = {"items": s["rays"], "through_the_queue": q, "not_open": s["hits"]}
            say("L = %d S = %2d: %d of %d items went through the fix-up queue; %d not open; %.2f node visits per item" % (
                L, S, q, s["rays"], s["hits"], s["nodes"] / max(s["rays"], 1)))
            del out_f, out_m, rays_out, hand_occ
            torch.cuda.empty_cache()
    result["scenes"][sname] = res
    acc.close(); del org, dr, rec
    torch.cuda.empty_cache()
say(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
