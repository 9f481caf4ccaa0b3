"""The environment-lit gather for a caller's batch of hit records (lh_accel_env_device) on two scenes, N = 16 and 64 gather rays per hit,
a seeded 1024 x 512 light probe as the accelerator's environment, one process:
  S-soup-1M  -- 1 M soup triangles, `--rays` rays of the synthetic dump and their closest-hit records;
  config 5   -- the AO example scene (tests/golden/ao_c1.npz) tessellated `--tess` times, the primary rays of a `--size`^2 frame.
Every rate is M gather rays/s over a window of at least `--window` seconds of back-to-back calls (device time by events around the
window) after a warm-up; the candidate ALTERNATES with its baseline and each pair is repeated `--repeats` times, so the spread of the run
stands next to every ratio.  The candidate is always the fused stage (env_device, "ao_fused" 1):
  (a) / the materialised stage ("ao_fused" 0: gather rays in HBM, one any-hit launch, the same resolve reading the directions);
  (b) / the same by hand: ao_rays_device (48 bytes of ray per gather ray; eps is AO's 1e-6 here and there), any-hit intersect_device,
      environment_device on every direction, the masked sum and the scatter as torch operations on the device;
  (c) / the fused AO stage on the same hits (ao_device): the price of the byte per ray plus the colour resolve -- the figure that matters.
(a)'s two answers are compared bit for bit.  With statistics on, one more fused pass reports the gather rays that went through the
fix-up queue.
    python tools/env_batch.py [--rays 4000000] [--size 1024] [--tess 8] [--scenes soup,c5] [--repeats 3] [--window 1.0] [--out profiles/env_batch.txt]"""
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
ap.add_argument("--rays", type=int, default=4_000_000)
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


result = {"repeats": args.repeats, "window_s": args.window, "map": [512, 1024], "scenes": {}}
sky = np.random.default_rng(3).uniform(0.1, 2.0, (512, 1024, 4)).astype(np.float32)
for sname in args.scenes.split(","):
    acc, org, dr, what = scene(sname)
    acc.set_environment((1.0, 0.5, 2.0), sky)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    n = int(org.shape[0]); hit = rec[0] != -1; nhit = int(hit.sum())
    p = la.EnvParams(1.0e-6, 1.0)          # AO's offset: the by-hand rays and the AO stage of (c) start where the gather's do
    res = {"what": what, "rays": n, "hits": nhit}
    say("== %s: %d hits of %d rays; light probe 1024 x 512" % (what, nhit, n))
    for NS in (16, 64):
        N = int(NS ** 0.5) ** 2; ng = nhit * N
        out_f = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda"))
        out_m = (torch.empty_like(out_f[0]), torch.empty_like(out_f[1])); out_a = (torch.empty_like(out_f[0]), torch.empty(n, dtype=torch.float32, device="cuda"))
        rays_out = acc.ao_rays_device(org, dr, rec, NS)
        hand_occ = torch.empty(n * N, dtype=torch.uint8, device="cuda"); hand_rgb = torch.empty((n * N, 3), dtype=torch.float32, device="cuda")

        def fused():
            acc.env_device(org, dr, rec, NS, p, out=out_f)

        def materialised():
            acc.set_param("ao_fused", 0)
            try:
                acc.env_device(org, dr, rec, NS, p, out=out_m)
            finally:
                acc.set_param("ao_fused", 1)

        def by_hand():
            slot, nslots, ao_o, ao_d = acc.ao_rays_device(org, dr, rec, NS, out=rays_out)
            k = int(nslots.item()) * N
            occ = acc.intersect_device(ao_o[:k], ao_d[:k], mode=la.MODE_ANY, out=(hand_occ[:k],))[0]
            rgb = acc.environment_device(ao_d[:k], out=hand_rgb[:k])
            blocked = occ.view(-1, N) != 0
            s = torch.where(blocked[:, :, None], torch.zeros((), dtype=torch.float64, device=org.device), rgb.view(-1, N, 3).double()).sum(dim=1)
            val = ((p.scale * s) / N).float(); cnt = blocked.sum(dim=1, dtype=torch.int32)
            h = slot != -1
            oc = torch.full((n,), -1, dtype=torch.int32, device=org.device); oc[h] = cnt[slot[h].long()]
            ov = torch.zeros((n, 3), dtype=torch.float32, device=org.device); ov[h] = val[slot[h].long()]
            return oc, ov

        def ao_stage():
            acc.ao_device(org, dr, rec, NS, out=out_a)

        for tag, base in (("a fused / materialised", materialised), ("b fused / by hand", by_hand), ("c fused gather / fused AO", ao_stage)):
            r = pairs(fused, base, ng)
            if base is materialised:
                r["answers_equal"] = bool(torch.equal(out_f[0], out_m[0]) and torch.equal(out_f[1].view(torch.int32), out_m[1].view(torch.int32)))
            if base is by_hand:          # torch's sum need not take the r order: counts equal, colours close
                oc, ov = by_hand()
                r["counts_equal"] = bool(torch.equal(oc, out_f[0])); r["largest_colour_difference"] = float((ov - out_f[1]).abs().max())
            res["N=%d %s" % (N, tag)] = r
            say("N = %2d (%s) fused %s  baseline %s M gather rays/s  ratio %s (median %.4f; the baseline's own spread %.4f)%s" % (
                N, tag, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["baseline_spread"],
                "  answers equal: %s" % r["answers_equal"] if "answers_equal" in r else ""))
        acc.trace_statistics(True)
        acc.statistics(clear=True); fused(); s = acc.statistics(clear=True); q = int(acc.L.lh_accel_last_retraced(acc.h))
        acc.trace_statistics(False)
        res["N=%d queue" % N] = {"gather_rays": s["rays"], "through_the_queue": q, "occluded": s["hits"]}
        say("N = %2d: %d of %d gather rays went through the fix-up queue; %d occluded; %.2f node visits per gather ray" % (
            N, q, s["rays"], s["hits"], s["nodes"] / max(s["rays"], 1)))
        del out_f, out_m, out_a, rays_out, hand_occ, hand_rgb
        torch.cuda.empty_cache()
    result["scenes"][sname] = res
    acc.close(); del org, dr, rec
    torch.cuda.empty_cache()
say(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
