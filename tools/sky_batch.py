"""The sun-and-sky gather for a caller's batch of hit records (lh_accel_env_device while a sky is set) on two scenes, N = 16 and 64 gather
rays per hit, one process:
  S-soup-1M  -- 1 M soup triangles, `--rays` rays of the synthetic dump and their closest-hit records;
  config 5   -- the AO example scene (tests/golden/ao_c1.npz) tessellated `--tess` times, the primary rays of a `--size`^2 frame.
The sky is the reference's default site (tests/golden/sky_reference.npz holds its basis floats and sun colour); the map it is measured
against is tools/env_batch.py's seeded 1024 x 512 light probe.  Every rate is M gather rays/s (hits x N: the sun's rays are not counted)
over a window of at least `--window` seconds of back-to-back calls (device time by events around the window) after a warm-up; the
candidate ALTERNATES with its baseline and each pair is repeated `--repeats` times, so the spread of the run stands next to every ratio.
All stages fused ("ao_fused" 1):
  (a) the sky gather without the sun / the map gather on the same hits: the analytic sky against four texel gathers per open ray;
  (b) the sky gather with the sun / the map gather: plus one launch and 1 / N more rays;
  (c) the sky gather with the sun / the same by hand: ao_rays_device (48 bytes of ray per gather ray), any-hit intersect_device on them
      and on one sun ray per hit, sky_device on every direction, the masked sum, the sun's term and the scatter as torch operations.
(c)'s counts are compared exactly, its colours by their largest difference (torch's sum need not take the r order).
    python tools/sky_batch.py [--rays 4000000] [--size 1024] [--tess 8] [--scenes soup,c5] [--repeats 3] [--window 1.0] [--out profiles/sky_batch.txt]"""
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


gold = np.load(os.path.join(ROOT, "tests", "golden", "sky_reference.npz"))
site = gold["site0"]
result = {"repeats": args.repeats, "window_s": args.window, "map": [512, 1024], "site": [float(x) for x in site], "scenes": {}}
probe = np.random.default_rng(3).uniform(0.1, 2.0, (512, 1024, 4)).astype(np.float32)
for sname in args.scenes.split(","):
    acc, org, dr, what = scene(sname)
    acc.set_environment((1.0, 0.5, 2.0), probe)
    skies = {f: la.Sky.from_site(site[0], site[1], site[2], int(site[3]), site[4], site[5], basis_rgb=gold["basis_rgb"], basis_y=gold["basis_y"],
                                 sun_rgb=gold["sun_rgb0"], flags=f) for f in (0, la.SKY_SUN)}
    sun_dir = torch.tensor(list(skies[0].sun_dir), dtype=torch.float64, device="cuda")
    sun_rgb = torch.tensor(list(skies[0].sun_rgb), dtype=torch.float32, device="cuda").double()
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    n = int(org.shape[0]); nhit = int((rec[0] != -1).sum())
    p = la.EnvParams(1.0e-6, 0.3183098861837907)          # AO's offset: the by-hand rays start where the gather's do
    res = {"what": what, "rays": n, "hits": nhit}
    say("== %s: %d hits of %d rays; sky of the default site, light probe 1024 x 512" % (what, nhit, n))
    for NS in (16, 64):
        N = int(NS ** 0.5) ** 2; ng = nhit * N
        out_s = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda"))
        out_m = (torch.empty_like(out_s[0]), torch.empty_like(out_s[1]))
        rays_out = acc.ao_rays_device(org, dr, rec, NS)
        hand_occ = torch.empty(n * N, dtype=torch.uint8, device="cuda"); hand_rgb = torch.empty((n * N, 3), dtype=torch.float32, device="cuda")
        hand_sun = torch.empty(n, dtype=torch.uint8, device="cuda")

        def sky_gather(flags):
            def f():
                acc.set_sky(skies[flags])
                acc.env_device(org, dr, rec, NS, p, out=out_s)
            return f

        def map_gather():
            acc.reset_sky()
            acc.env_device(org, dr, rec, NS, p, out=out_m)

        def by_hand():
            acc.set_sky(skies[la.SKY_SUN])
            slot, nslots, ao_o, ao_d = acc.ao_rays_device(org, dr, rec, NS, out=rays_out)
            m = int(nslots.item()); k = m * N
            occ = acc.intersect_device(ao_o[:k], ao_d[:k], mode=la.MODE_ANY, out=(hand_occ[:k],))[0]
            so = ao_o[:k].view(m, N, 3)[:, 0, :].contiguous()
            socc = acc.intersect_device(so, sun_dir.expand(m, 3).contiguous(), mode=la.MODE_ANY, out=(hand_sun[:m],))[0]
            rgb = acc.sky_device(ao_d[:k], out=hand_rgb[:k])
            blocked = occ.view(-1, N) != 0
            s = torch.where(blocked[:, :, None], torch.zeros((), dtype=torch.float64, device=org.device), rgb.view(-1, N, 3).double()).sum(dim=1)
            s = torch.where((socc != 0)[:, None], s, s + sun_rgb[None, :])
            val = ((p.scale * s) / N).float(); cnt = blocked.sum(dim=1, dtype=torch.int32)
            h = slot != -1
            oc = torch.full((n,), -1, dtype=torch.int32, device=org.device); oc[h] = cnt[slot[h].long()]
            ov = torch.zeros((n, 3), dtype=torch.float32, device=org.device); ov[h] = val[slot[h].long()]
            return oc, ov

        for tag, cand, base in (("a sky / map", sky_gather(0), map_gather), ("b sky + sun / map", sky_gather(la.SKY_SUN), map_gather),
                                ("c sky + sun / by hand", sky_gather(la.SKY_SUN), by_hand)):
            r = pairs(cand, base, ng)
            if base is by_hand:
                cand(); oc, ov = by_hand()
                r["counts_equal"] = bool(torch.equal(oc, out_s[0]))
                r["largest_relative_colour_difference"] = float(((ov - out_s[1]).abs().max() / out_s[1].abs().max()).item())
            res["N=%d %s" % (N, tag)] = r
            say("N = %2d (%s) candidate %s  baseline %s M gather rays/s  ratio %s (median %.4f; the baseline's own spread %.4f)%s" % (
                N, tag, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["baseline_spread"],
                "  counts equal: %s, largest relative colour difference %.3g" % (r["counts_equal"], r["largest_relative_colour_difference"]) if "counts_equal" in r else ""))
        del out_s, out_m, rays_out, hand_occ, hand_rgb, hand_sun
        torch.cuda.empty_cache()
    result["scenes"][sname] = res
    acc.close(); del org, dr, rec
    torch.cuda.empty_cache()
say(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
