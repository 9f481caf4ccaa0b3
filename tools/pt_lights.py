"""The path tracer with a light list (lh_render_pt_tile_lit) on the config-4 frame: tests/golden/ao_ps.npz (1 986 triangles, vertex normals), kd 0.8,
white environment, `--size`^2 pixels x `--spp` samples in ONE pass, at most `--vertices` path vertices.  Every time is milliseconds per frame over a
window of at least `--window` seconds of back-to-back frames (wall clock around the window: a lit pass synchronises once per bounce, its host time is part
of what it costs) after a warm-up; the candidate ALTERNATES with its baseline and each pair is repeated `--repeats` times, so the spread of the run stands
next to every ratio.
  (a) lh_render_pt_tile_lit with nlights = 0 and no sink / lh_render_pt_tile2, one process: the same launches, frames compared bit for bit;
  (b) nlights = 1 and 4 / nlights = 0: what the lights cost a frame and a bounce (the bounces the pass ran: max_depth_reached), and the shadow rays/s
      that is (hits x nlights work items over the difference); light 0 is directional, the others point lights above the scene, all with the cosine;
  (c) with --parent LIB (the parent commit's liblucille_hip.so): lh_render_pt_tile2 of this build / of that one, in ALTERNATING PROCESSES, one window
      each, before this process opens the device.
    python tools/pt_lights.py [--size 1024] [--spp 16] [--vertices 8] [--repeats 3] [--window 1.0] [--parent LIB] [--out profiles/pt_lights.txt]"""
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
ap.add_argument("--child", action="store_true", help="one window of lh_render_pt_tile2 with the library LH_LIBRARY names; prints its ms per frame")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def child_ms(lib):
    env = dict(os.environ)
    if lib:
        env["LH_LIBRARY"] = os.path.abspath(lib)
    else:
        env.pop("LH_LIBRARY", None)
    out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", "--size", str(args.size), "--spp", str(args.spp),
                                   "--vertices", str(args.vertices), "--window", str(args.window)], env=env, timeout=300)
    return float(json.loads(out.decode().strip().splitlines()[-1])["ms"])


# (c) first: this process has not opened the device yet
parent = None
if args.parent and not args.child:
    cand, base = [], []
    for _ in range(args.repeats):
        cand.append(child_ms(None)); base.append(child_ms(args.parent))
    parent = {"this_build_ms": [round(x, 3) for x in cand], "parent_ms": [round(x, 3) for x in base],
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


def unlit():
    out.zero_()
    stats["tile2"] = acc.render_pt_tile2(cam, 0, 0, N, N, 0, args.spp, args.spp, max_vertices=args.vertices, seed=7, out=out)[1]


if args.child:
    unlit(); unlit()
    print(json.dumps({"ms": window_ms(unlit), "library": la.library_path()}), flush=True)
    acc.close()
    sys.exit(0)

LIGHTS = [la.Light((-0.5, 0.6, 1.0), (1.5, 1.0, 0.5), la.LIGHT_COSINE), la.Light((5.5, -5.0, 4.0), (40.0, 30.0, 20.0), la.LIGHT_POINT | la.LIGHT_COSINE | la.LIGHT_INVSQ),
          la.Light((-3.0, 2.0, 5.0), (30.0, 30.0, 40.0), la.LIGHT_POINT | la.LIGHT_COSINE | la.LIGHT_INVSQ), la.Light((2.0, 4.0, 3.0), (5.0, 4.0, 3.0), la.LIGHT_POINT | la.LIGHT_COSINE)]


def lit_fn(L):
    def fn():
        out.zero_()
        stats[L] = acc.render_pt_tile_lit(cam, 0, 0, N, N, 0, args.spp, args.spp, max_vertices=args.vertices, lights=LIGHTS[:L], seed=7, out=out)[1]
    return fn


def pairs(cand, base):
    cand(); base()
    a, b = [], []
    for _ in range(args.repeats):
        a.append(window_ms(cand)); b.append(window_ms(base))
    return a, b


result = {"size": N, "spp": args.spp, "max_vertices": args.vertices, "repeats": args.repeats, "window_s": args.window}
say("== config-4 frame: ao_ps (1 986 triangles), %d^2 x %d spp in one pass (%d paths), <= %d vertices, kd 0.8, white environment" % (N, args.spp, N * N * args.spp, args.vertices))
# (a)
lit0 = lit_fn(0)
unlit(); ref = out.clone(); lit0(); equal = bool(torch.equal(out.view(torch.int32), ref.view(torch.int32)))
a, b = pairs(lit0, unlit)
result["a nlights 0 / tile2"] = {"lit_entry_ms": [round(x, 3) for x in a], "tile2_ms": [round(x, 3) for x in b], "median_ratio": round(float(np.median(a) / np.median(b)), 4),
                                 "tile2_spread_ms": round(max(b) - min(b), 3), "frames_equal": equal, "rays": stats["tile2"]["rays"]}
say("(a) nlights 0 through lh_render_pt_tile_lit %s ms / lh_render_pt_tile2 %s ms a frame: median ratio %.4f (tile2's own spread %.3f ms); frames equal bit for bit: %s; %d rays, %d bounces" % (
    [round(x, 3) for x in a], [round(x, 3) for x in b], float(np.median(a) / np.median(b)), max(b) - min(b), equal, stats["tile2"]["rays"], stats["tile2"]["max_depth_reached"]))
# (b)
bounces = int(stats["tile2"]["max_depth_reached"])
sink = la.PtSink(int(stats["tile2"]["rays"]), args.vertices, fields=("prim",))
acc.render_pt_tile_lit(cam, 0, 0, N, N, 0, args.spp, args.spp, max_vertices=args.vertices, sink=sink, seed=7)
hits = int((sink.prim[:sink.total()] != -1).sum().item())
del sink
torch.cuda.empty_cache()
for L in (1, 4):
    a, b = pairs(lit_fn(L), lit0)
    d = float(np.median(a) - np.median(b))
    result["b nlights %d / 0" % L] = {"lit_ms": [round(x, 3) for x in a], "unlit_ms": [round(x, 3) for x in b], "lights_cost_ms": round(d, 3),
                                      "per_bounce_ms": round(d / bounces, 3), "per_light_per_bounce_ms": round(d / bounces / L, 3), "hits": hits,
                                      "M_shadow_rays_per_s": round(hits * L / d / 1e3, 1), "unlit_spread_ms": round(max(b) - min(b), 3)}
    say("(b) nlights %d %s ms / nlights 0 %s ms a frame (spread %.3f ms): the lights cost %.3f ms a frame = %.3f ms a bounce (%d bounces) = %.3f ms a light and bounce; "
        "%d hits x %d lights: %.1f M shadow rays/s" % (L, [round(x, 3) for x in a], [round(x, 3) for x in b], max(b) - min(b), d, d / bounces, bounces, d / bounces / L,
                                                      hits, L, hits * L / d / 1e3))
# (c)
if parent:
    result["c tile2, this build / the parent's"] = parent
    say("(c) lh_render_pt_tile2, alternating processes: this build %s ms, the parent commit's %s ms a frame: medians differ by %+.3f ms; the parent's own spread %.3f ms, "
        "this build's %.3f ms" % (parent["this_build_ms"], parent["parent_ms"], parent["median_difference_ms"], parent["parent_spread_ms"], parent["this_build_spread_ms"]))
acc.close()
say(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
