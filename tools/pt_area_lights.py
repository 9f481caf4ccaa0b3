"""The path tracer with area lights at every path vertex (lh_render_pt_tile_lights) on the config-4 frame: tests/golden/ao_ps.npz (1 986 triangles,
vertex normals), kd 0.8, white environment, `--size`^2 pixels x `--spp` samples in ONE pass, at most `--vertices` path vertices, one emitter quad of
two triangles above the scene.  Every time is milliseconds per frame over a window of at least `--window` seconds of back-to-back frames (wall clock
around the window: a lit pass synchronises once per stage and bounce, its host time is part of what it costs) after a warm-up; the candidate ALTERNATES
with its baseline and each pair is repeated `--repeats` times, so the spread of the run stands next to every difference.
  (a) lh_render_pt_tile_lights with no lights and no sink / lh_render_pt_tile2, and with one delta light / lh_render_pt_tile_lit with it, one process:
      the same launches, frames compared bit for bit;
  (b) one delta light / no lights: the yardstick tools/pt_lights.py measured, in this run;
  (c) narea = 1 with S = 1, 4, 16 and narea = 4 with S = 4 / no lights: what the area lights cost a frame and a bounce (the bounces the pass ran:
      max_depth_reached), and the shadow rays/s that is (hits x narea x S work items over the difference);
  (d) with --parent LIB (the parent commit's liblucille_hip.so): lh_render_pt_tile2, and lh_render_pt_tile_lit with one light, of this build / of that
      one, in ALTERNATING PROCESSES, one window each, before this process opens the device.
    python tools/pt_area_lights.py [--size 1024] [--spp 16] [--vertices 8] [--repeats 3] [--window 1.0] [--parent LIB] [--out profiles/pt_area_lights.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--vertices", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=1.0)
ap.add_argument("--parent", default=None)
ap.add_argument("--child", choices=("tile2", "lit1"), default=None,
                help="one window of lh_render_pt_tile2, or of lh_render_pt_tile_lit with one light, with the library LH_LIBRARY names; prints its ms per frame")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def child_ms(lib, entry):
    env = dict(os.environ)
    if lib:
        env["LH_LIBRARY"] = os.path.abspath(lib)
    else:
        env.pop("LH_LIBRARY", None)
    out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", entry, "--size", str(args.size), "--spp", str(args.spp),
                                   "--vertices", str(args.vertices), "--window", str(args.window)], env=env, timeout=300)
    return float(json.loads(out.decode().strip().splitlines()[-1])["ms"])


# (d) first: this process has not opened the device yet
parent = {}
if args.parent and not args.child:
    for entry in ("tile2", "lit1"):
        cand, base = [], []
        for _ in range(args.repeats):
            cand.append(child_ms(None, entry)); base.append(child_ms(args.parent, entry))
        parent[entry] = {"this_build_ms": [round(x, 3) for x in cand], "parent_ms": [round(x, 3) for x in base],
                         "median_difference_ms": round(float(np.median(cand) - np.median(base)), 3), "parent_spread_ms": round(max(base) - min(base), 3),
                         "this_build_spread_ms": round(max(cand) - min(cand), 3)}

import torch  # noqa: E402

import lucille_amd as la  # noqa: E402


def window_ms(fn):
    """milliseconds per call of fn over >= args.window seconds of back-to-back calls, by the wall clock"""
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    k = max(2, int(np.ceil(1.15 * args.window / max(time.perf_counter() - t0, 1e-6))))
    while True:
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= args.window:
            return dt / k * 1e3
        k = int(np.ceil(k * 1.3 * args.window / dt))


g = np.load(os.path.join(ROOT, "tests", "golden", "ao_ps.npz"))
acc = la.HipAccel(0)
for k in range(int(g["ngeoms"])):
    acc.add_mesh(g["pos%d" % k], g["idx%d" % k])
    if ("nrm%d" % k) in g.files:
        acc.set_normals(k, g["nrm%d" % k], int(g["two_side%d" % k]))
acc.commit(); acc.wait_exact()
acc.set_material(la.ALL_MESHES, la.Material.make(kd=(0.8, 0.8, 0.8)))
acc.set_environment((1.0, 1.0, 1.0), None)
c = g["camera"]
N = args.size
cam = la.Camera.make(N, N, c[16], c[:16], int(c[19]))
out = torch.zeros((N, N, 3), dtype=torch.float32, device="cuda")
stats = {}
DELTA = [la.Light((-0.5, 0.6, 1.0), (1.5, 1.0, 0.5), la.LIGHT_COSINE)]


def unlit():
    out.zero_()
    stats["tile2"] = acc.render_pt_tile2(cam, 0, 0, N, N, 0, args.spp, args.spp, max_vertices=args.vertices, seed=7, out=out)[1]


def lit1():
    out.zero_()
    stats["lit1"] = acc.render_pt_tile_lit(cam, 0, 0, N, N, 0, args.spp, args.spp, max_vertices=args.vertices, lights=DELTA, seed=7, out=out)[1]


if args.child:
    fn = unlit if args.child == "tile2" else lit1
    fn(); fn()
    print(json.dumps({"ms": window_ms(fn), "library": la.library_path()}), flush=True)
    acc.close()
    sys.exit(0)

# the emitter quad above the sphere, its normals pointing down; four lights share it in the narea = 4 run
acc.set_emitters(np.array([[[1.7, -3.0, 6.5], [1.7, -1.0, 6.5], [3.7, -1.0, 6.5]], [[1.7, -3.0, 6.5], [3.7, -1.0, 6.5], [3.7, -3.0, 6.5]]]))
AREA = [la.AreaLight(0, 2, rgb, la.AREA_COSINE | la.AREA_FACING) for rgb in ((3.0, 2.5, 2.0), (0.5, 1.0, 2.0), (2.0, 0.5, 1.0), (1.0, 1.0, 1.0))]


def lights_fn(name, delta=(), narea=0, S=1):
    def fn():
        out.zero_()
        stats[name] = acc.render_pt_tile_lights(cam, 0, 0, N, N, 0, args.spp, args.spp, max_vertices=args.vertices, lights=delta, area=AREA[:narea],
                                                area_params=la.AreaParams(1e-5, 1.0, S), seed=7, out=out)[1]
    return fn


def pairs(cand, base):
    cand(); base()
    a, b = [], []
    for _ in range(args.repeats):
        a.append(window_ms(cand)); b.append(window_ms(base))
    return a, b


def r3(xs):
    return [round(x, 3) for x in xs]


result = {"size": N, "spp": args.spp, "max_vertices": args.vertices, "repeats": args.repeats, "window_s": args.window}
say("== config-4 frame: ao_ps (1 986 triangles), %d^2 x %d spp in one pass (%d paths), <= %d vertices, kd 0.8, white environment, one emitter quad" % (
    N, args.spp, N * N * args.spp, args.vertices))
# (a)
none = lights_fn("none")
for name, cand, base in (("no lights / tile2", none, unlit), ("one delta light / tile_lit", lights_fn("delta1", DELTA), lit1)):
    base(); ref = out.clone(); cand(); equal = bool(torch.equal(out.view(torch.int32), ref.view(torch.int32)))
    a, b = pairs(cand, base)
    result["a " + name] = {"lights_entry_ms": r3(a), "baseline_ms": r3(b), "median_ratio": round(float(np.median(a) / np.median(b)), 4),
                           "baseline_spread_ms": round(max(b) - min(b), 3), "frames_equal": equal}
    say("(a) lh_render_pt_tile_lights, %s: %s ms / %s ms a frame: median ratio %.4f (the baseline's own spread %.3f ms); frames equal bit for bit: %s" % (
        name, r3(a), r3(b), float(np.median(a) / np.median(b)), max(b) - min(b), equal))
bounces = int(stats["tile2"]["max_depth_reached"])
sink = la.PtSink(int(stats["tile2"]["rays"]), args.vertices, fields=("prim",))
acc.render_pt_tile_lit(cam, 0, 0, N, N, 0, args.spp, args.spp, max_vertices=args.vertices, sink=sink, seed=7)
hits = int((sink.prim[:sink.total()] != -1).sum().item())
del sink
torch.cuda.empty_cache()
# (b), (c)
for name, cand, items in (("b one delta light", lit1, 1), ("c narea 1, S 1", lights_fn("a1s1", (), 1, 1), 1), ("c narea 1, S 4", lights_fn("a1s4", (), 1, 4), 4),
                          ("c narea 1, S 16", lights_fn("a1s16", (), 1, 16), 16), ("c narea 4, S 4", lights_fn("a4s4", (), 4, 4), 16)):
    a, b = pairs(cand, none)
    d = float(np.median(a) - np.median(b))
    result[name + " / no lights"] = {"lit_ms": r3(a), "unlit_ms": r3(b), "lights_cost_ms": round(d, 3), "per_bounce_ms": round(d / bounces, 3), "hits": hits,
                                     "items_per_hit": items, "M_shadow_rays_per_s": round(hits * items / d / 1e3, 1), "unlit_spread_ms": round(max(b) - min(b), 3)}
    say("(%s) %s ms / no lights %s ms a frame (spread %.3f ms): the lights cost %.3f ms a frame = %.3f ms a bounce (%d bounces); %d hits x %d items: "
        "%.1f M shadow rays/s" % (name, r3(a), r3(b), max(b) - min(b), d, d / bounces, bounces, hits, items, hits * items / d / 1e3))
# (d)
for entry, what in (("tile2", "lh_render_pt_tile2"), ("lit1", "lh_render_pt_tile_lit with one light")):
    if entry in parent:
        p = parent[entry]
        result["d %s, this build / the parent's" % entry] = p
        say("(d) %s, alternating processes: this build %s ms, the parent commit's %s ms a frame: medians differ by %+.3f ms; the parent's own spread %.3f ms, "
            "this build's %.3f ms" % (what, p["this_build_ms"], p["parent_ms"], p["median_difference_ms"], p["parent_spread_ms"], p["this_build_spread_ms"]))
acc.close()
say(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
