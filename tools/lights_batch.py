"""Direct light for a caller's batch of hit records (lh_accel_lights_device) on two scenes, L = 1, 4 and 16 lights, one process:
  S-soup-1M  -- 1 M soup triangles, `--rays` rays of the synthetic dump and their closest-hit records;
  config 5   -- the AO example scene (tests/golden/ao_c1.npz) tessellated `--tess` times, the primary rays of a `--size`^2 frame.
The lights: light 0 is directional (the reference's sun, no flags); the others alternate point lights around the scene's box, plain and with the
inverse square.  Every rate is M shadow rays/s (hits x L work items) over a window of at least `--window` seconds of back-to-back calls (device time
by events around the window) after a warm-up; the candidate ALTERNATES with its baseline and each pair is repeated `--repeats` times, so the
spread of the run stands next to every ratio.  The candidate is always the fused stage (lights_device, "ao_fused" 1):
  (a) / the materialised stage ("ao_fused" 0: rays and bounds in HBM, one bounded any-hit launch, the same resolve);
  (a') the same pair with LIGHT_COSINE on every light: the fused stage never walks the items the cosine culls, the materialised one launches them
       under a dead bound;
  (b) / the same by hand: light_rays_device (56 bytes of ray and bound per item), a bounded any-hit intersect_device, the masked weighted sum and
      the scatter as torch operations on the device (lights without the cosine: the weight is 1 or 1 / |dir|^2, made from the ray arrays);
  (c) L = 1, directional: the milliseconds of one call against what the sky gather's sun launch costs in the same run -- env_device under a
      sky with LH_SKY_SUN minus the same call without it (N = 16 gather rays; the difference is the sun's ray kernel and its any-hit launch).
(a)'s two answers are compared bit for bit.  With statistics on, one more fused pass reports the items that went through the fix-up queue.
    python tools/lights_batch.py [--rays 4000000] [--size 1024] [--tess 8] [--scenes soup,c5] [--repeats 3] [--window 1.0] [--out profiles/lights_batch.txt]"""
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
SUN_DIR = (0.3, 0.9, 0.316227766)


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


def light_list(L, lo, hi, cosine):
    """light 0: the sun; then point lights on a shell around the hits' box, every second one with the inverse square"""
    rng = np.random.default_rng(17)
    c = 0.5 * (lo + hi); r = float(np.linalg.norm(hi - lo))
    out = [la.Light(SUN_DIR, (1.0, 0.9, 0.8), la.LIGHT_COSINE if cosine else 0)]
    for l in range(1, L):
        v = rng.normal(size=3); v = c + v / np.linalg.norm(v) * r * rng.uniform(0.6, 1.5)
        f = la.LIGHT_POINT | (la.LIGHT_INVSQ if l % 2 == 0 else 0) | (la.LIGHT_COSINE if cosine else 0)
        out.append(la.Light(tuple(v), tuple(rng.uniform(0.2, 2.0, 3)), f))
    return out


result = {"repeats": args.repeats, "window_s": args.window, "scenes": {}}
for sname in args.scenes.split(","):
    acc, org, dr, what = scene(sname)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    n = int(org.shape[0]); hit = rec[0] != -1; nhit = int(hit.sum())
    Ph = (org + dr * rec[1][:, None])[hit]
    lo, hi = Ph.min(dim=0).values.cpu().numpy(), Ph.max(dim=0).values.cpu().numpy()
    del Ph
    p = la.LightsParams(1.0e-5)
    res = {"what": what, "rays": n, "hits": nhit}
    say("== %s: %d hits of %d rays" % (what, nhit, n))
    for L in (1, 4, 16):
        items = nhit * L
        out_f = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda"))
        out_m = (torch.empty_like(out_f[0]), torch.empty_like(out_f[1]))
        for cosine in (0, 1):
            ls = light_list(L, lo, hi, cosine)

            def fused():
                acc.lights_device(org, dr, rec, ls, p, out=out_f)

            def materialised():
                acc.set_param("ao_fused", 0)
                try:
                    acc.lights_device(org, dr, rec, ls, p, out=out_m)
                finally:
                    acc.set_param("ao_fused", 1)

            tag = "a' fused / materialised, cosine" if cosine else "a fused / materialised"
            r = pairs(fused, materialised, items)
            r["answers_equal"] = bool(torch.equal(out_f[0], out_m[0]) and torch.equal(out_f[1].view(torch.int32), out_m[1].view(torch.int32)))
            res["L=%d %s" % (L, tag)] = r
            say("L = %2d (%s) fused %s  baseline %s M shadow rays/s  ratio %s (median %.4f; the baseline's own spread %.4f)  answers equal: %s" % (
                L, tag, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["baseline_spread"], r["answers_equal"]))
        ls = light_list(L, lo, hi, 0)
        rays_out = acc.light_rays_device(org, dr, rec, ls, p)
        hand_occ = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        rgb_l = torch.tensor([list(x.rgb) for x in ls], dtype=torch.float64, device="cuda")
        invsq = torch.tensor([bool(x.flags & la.LIGHT_INVSQ) for x in ls], device="cuda")

        def fused():
            acc.lights_device(org, dr, rec, ls, p, out=out_f)

        def by_hand():
            slot, nslots, ro, rd, rt = acc.light_rays_device(org, dr, rec, ls, p, out=rays_out)
            k = int(nslots.item()) * L
            occ = acc.intersect_device(ro[:k], rd[:k], mode=la.MODE_ANY, tmax=rt[:k], out=(hand_occ[:k],))[0]
            bit = (rt[:k].view(-1, L) > 0) & (occ.view(-1, L) == 0)
            d = rd[:k].view(-1, L, 3)
            w = torch.where(invsq[None, :], 1.0 / (d * d).sum(dim=2), torch.ones((), dtype=torch.float64, device=org.device))
            val = (torch.where(bit, w, torch.zeros((), dtype=torch.float64, device=org.device))[:, :, None] * rgb_l[None, :, :]).sum(dim=1).float()
            mask = (bit.int() << torch.arange(L, dtype=torch.int32, device=org.device)[None, :]).sum(dim=1, dtype=torch.int32)
            h = slot != -1
            om = torch.full((n,), -1, dtype=torch.int32, device=org.device); om[h] = mask[slot[h].long()]
            ov = torch.zeros((n, 3), dtype=torch.float32, device=org.device); ov[h] = val[slot[h].long()]
            return om, ov

        r = pairs(fused, by_hand, items)
        om, ov = by_hand()          # torch's sum need not take the list order: masks equal, colours close
        r["masks_equal"] = bool(torch.equal(om, out_f[0])); r["largest_colour_difference"] = float((ov - out_f[1]).abs().max())
        res["L=%d b fused / by hand" % L] = r
        say("L = %2d (b fused / by hand) fused %s  baseline %s M shadow rays/s  ratio %s (median %.4f; the baseline's own spread %.4f)  masks equal: %s, colours within %.3g" % (
            L, r["candidate_Mrays"], r["baseline_Mrays"], r["ratio"], r["ratio_median"], r["baseline_spread"], r["masks_equal"], r["largest_colour_difference"]))
        acc.trace_statistics(True)
        acc.statistics(clear=True); fused(); s = acc.statistics(clear=True); q = int(acc.L.lh_accel_last_retraced(acc.h))
        acc.trace_statistics(False)
        res["L=%d queue" % L] = {"items": s["rays"], "through_the_queue": q, "bit_clear": s["hits"]}
        say("L = %2d: %d of %d items went through the fix-up queue; %d with their bit clear; %.2f node visits per item" % (
            L, q, s["rays"], s["hits"], s["nodes"] / max(s["rays"], 1)))
        del out_f, out_m, rays_out, hand_occ
        torch.cuda.empty_cache()
    # (c) one directional light against the sky gather's own sun launch
    sun = [la.Light(SUN_DIR, (1.0, 0.9, 0.8), 0)]
    out_l = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda"))
    out_e = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda"))
    sky = la.Sky.from_site(35.39, 139.44, 9.0, 20, 10.5, 2.0, basis_rgb=np.ones((3, 3)), basis_y=np.ones(3), sun_rgb=(1.0, 0.9, 0.8), flags=0)
    sky.sun_dir[:] = SUN_DIR
    ep = la.EnvParams(1.0e-5, 0.3183098861837907)

    def one_light():
        acc.lights_device(org, dr, rec, sun, p, out=out_l)

    def gather():
        acc.env_device(org, dr, rec, 16, ep, out=out_e)

    t_light, t_sun, t_nosun = [], [], []
    one_light()
    for _ in range(args.repeats):
        t_light.append(window_time(one_light) * 1e3)
        sky.flags = la.SKY_SUN; acc.set_sky(sky); gather(); t_sun.append(window_time(gather) * 1e3)
        sky.flags = 0; acc.set_sky(sky); gather(); t_nosun.append(window_time(gather) * 1e3)
    acc.reset_sky()
    diff = [a - b for a, b in zip(t_sun, t_nosun)]
    res["c one directional light"] = {"lights_device_ms": [round(x, 3) for x in t_light], "sky_gather_with_sun_ms": [round(x, 3) for x in t_sun],
                                      "sky_gather_without_sun_ms": [round(x, 3) for x in t_nosun], "sun_launch_ms": [round(x, 3) for x in diff]}
    say("(c) one directional light: lights_device %s ms a call (compaction, stage, resolve, its one round trip); the sky gather (N = 16) %s ms with the sun, %s without: the sun's launch %s ms" % (
        [round(x, 3) for x in t_light], [round(x, 3) for x in t_sun], [round(x, 3) for x in t_nosun], [round(x, 3) for x in diff]))
    result["scenes"][sname] = res
    acc.close(); del org, dr, rec, out_l, out_e
    torch.cuda.empty_cache()
say(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
