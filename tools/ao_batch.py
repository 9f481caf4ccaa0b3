"""The AO stage for a caller's batch of hit records, on the primary hit records of the BASELINE config-2 frame
(tests/golden/rib/ambient_occlusion.rib, size^2, its own 3 x 3 pixel samples, 64 AO samples), the three ALTERNATING within each repeat
of one process, device time by events around each:
  (a) HipAccel.ao_device, fused (lh_accel_ao_device);
  (b) the same AO by hand: ao_rays_device (N x 48 bytes of rays per hit to HBM), intersect_device in any-hit mode, a torch reduction
      and scatter;
  (c) render_ao_tile of the same frame under LH_STAGE_TIMING=1: the `compact + ao + resolve` stages it prints are the yardstick of
      (a), which runs the same traversal kernel behind a per-ray key load and in front of a scatter.
(a)'s counts are checked against (b)'s.  Compare (a) with (c) allowing (c)'s own spread over the repeats plus 5 %; (a) must beat (b).
    python tools/ao_batch.py [--size 1024] [--repeats 5] [--out profiles/ao_batch.txt]"""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lucille_amd as la  # noqa: E402
from lucille_amd import rib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--gather", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()

sc = rib.RibScene(os.path.join(ROOT, "tests", "golden", "rib", "ambient_occlusion.rib"))
acc = la.HipAccel(0); sc.add_to(acc); acc.commit(); acc.wait_exact()
ps = int(sc.info.pixel_samples[0]); W = H = args.size; NS = args.gather; N = int(NS ** 0.5) ** 2
cam = la.Camera.make(W, H, sc.camera.flength, list(sc.camera.cam2world), sc.camera.rh)
org, dr = acc.primary_rays(cam, 0, 0, W, H, ps)
rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
n = int(org.shape[0])
STAGES = re.compile(r"AO batch stages \(ms\): primary ([\d.]+) closest ([\d.]+) compact ([\d.]+) ao ([\d.]+) resolve ([\d.]+)")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1), r


def by_hand():
    slot, nslots, ao_o, ao_d = acc.ao_rays_device(org, dr, rec, NS)
    k = int(nslots.item())                                           # the any-hit call wants its ray count on the host
    occ = acc.intersect_device(ao_o[:k * N], ao_d[:k * N], mode=la.MODE_ANY)[0]
    per = occ.view(k, N).ne(0).sum(dim=1, dtype=torch.int32)
    hit = slot != -1
    cnt = torch.full((n,), -1, dtype=torch.int32, device=org.device)
    cnt[hit] = per[slot[hit].long()]
    rad = torch.where(hit, ((N - cnt.double()) / N).float(), torch.zeros((), device=org.device))
    return cnt, rad


def tile_stages():
    """render_ao_tile with the stage timer on -> (compact, ao, resolve) ms, from the line the library prints to stderr"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["LH_STAGE_TIMING"] = "1"
        try:
            acc.render_ao_tile(cam, 0, 0, W, H, ps, NS)
        finally:
            del os.environ["LH_STAGE_TIMING"]
            os.dup2(saved, 2); os.close(saved)
        tmp.seek(0); text = tmp.read().decode(errors="replace")
    m = STAGES.search(text)
    if not m:
        raise SystemExit("no stage line in the library's output:\n" + text)
    return tuple(float(m.group(k)) for k in (3, 4, 5))


ca, _ = acc.ao_device(org, dr, rec, NS); cb, _ = by_hand(); tile_stages()          # warm: buffers, queues, allocator
ok = bool(torch.equal(ca, cb))
ta, tb, tc = [], [], []
for _ in range(args.repeats):
    ta.append(timed(lambda: acc.ao_device(org, dr, rec, NS))[0])
    tb.append(timed(by_hand)[0])
    tc.append(tile_stages())
tcs = [sum(x) for x in tc]
hits = int((ca != -1).sum())
res = {"frame": "%dx%d, %d x %d pixel samples, %d AO samples" % (W, H, ps, ps, NS), "rays": n, "hits": hits, "ao_rays": hits * N,
       "repeats": args.repeats, "a_ao_device_ms": [round(x, 3) for x in ta], "b_by_hand_ms": [round(x, 3) for x in tb],
       "c_tile_compact_ao_resolve_ms": [round(x, 3) for x in tcs], "c_stages_ms": [[round(y, 3) for y in x] for x in tc],
       "median_ms": {"a": round(float(np.median(ta)), 3), "b": round(float(np.median(tb)), 3), "c": round(float(np.median(tcs)), 3)},
       "c_spread_ms": round(max(tcs) - min(tcs), 3), "a_over_c": round(float(np.median(ta) / np.median(tcs)), 3),
       "a_over_b": round(float(np.median(ta) / np.median(tb)), 3), "counts_a_equal_b": ok}
lines = ["ao_batch.py: %s; %d rays, %d hits, %d AO rays; %d repeats, (a) (b) (c) alternating" % (res["frame"], n, hits, hits * N, args.repeats),
         "(a) ao_device, fused            ms: %s   median %.3f" % (" ".join("%.3f" % x for x in ta), res["median_ms"]["a"]),
         "(b) by hand                     ms: %s   median %.3f" % (" ".join("%.3f" % x for x in tb), res["median_ms"]["b"]),
         "(c) tile compact + ao + resolve ms: %s   median %.3f   spread %.3f" % (" ".join("%.3f" % x for x in tcs), res["median_ms"]["c"], res["c_spread_ms"]),
         "a / c %.3f   a / b %.3f   counts of (a) == (b): %s" % (res["a_over_c"], res["a_over_b"], ok), json.dumps(res)]
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
acc.close(); sc.close()
