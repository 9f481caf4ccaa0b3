"""What material textures cost an AO frame (lh_accel_set_texture; the textured resolve of lh_render.hip), on two frames, one GPU:
  c2  BASELINE config 2 -- the example RIB (tests/golden/rib/ambient_occlusion.rib, its own PixelSamples), `--size`^2, 64 AO samples;
  c5  the config-5 scene -- tests/golden/ao_c1.npz tessellated `--tess` times -- at `--size`^2, one sample per pixel, 64 AO samples.
Every mesh gets planar per-vertex texture coordinates (four periods across the scene), so the fetches of a frame are spread over the
texture.  A frame is ONE tile, its image left in HBM; a time is ms per frame over a window of at least `--window` seconds of
back-to-back frames (host clock: every tile call ends synchronised) after a warm-up.
  (a) / (b)   one accelerator, windows ALTERNATING between (a) no texture and (b) a `--texture`^2 texture on every mesh, `--repeats`
              pairs: (b) - (a) is what the multiply costs, reported beside
  copy        the time of a plain device copy of the frame's sample records (prim, u, v: 20 bytes per camera sample) in the same run --
              the resolve's extra reads are of that order if the fetch is gather-bound as designed;
  (a) vs parent   with `--parent-lib FILE` (a liblucille_hip.so built from the parent commit): (a) in child processes ALTERNATING between
              that library and this tree's (LH_LIBRARY), `--repeats` pairs; the parent's own spread stands next to the difference.
    python tools/tex_frames.py [--scenes c2,c5] [--size 1024] [--tess 8] [--texture 1024] [--repeats 3] [--window 1.0]
                               [--parent-lib build/liblucille_hip_parent.so] [--out profiles/tex_frames.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lucille_amd as la  # noqa: E402
from lucille_amd import rib, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", default="c2,c5")
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--tess", type=int, default=8)
ap.add_argument("--texture", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=1.0)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help="(internal) one window of (a) on this scene, the time as JSON")
args = ap.parse_args()
NS = 64
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def planar_st(P, lo, hi):
    """four periods of s along x and of t along the larger of y / z, a little of the third axis in each"""
    q = (P - lo) / np.maximum(hi - lo, 1e-30)
    return np.ascontiguousarray(np.stack([4.0 * q[:, 0] + 0.37 * q[:, 1], 4.0 * q[:, 2] + 0.61 * q[:, 1]], -1))


def scene(name):
    """-> (accelerator with texture coordinates on every mesh, camera, pixel samples, description)"""
    acc = la.HipAccel(0)
    if name == "c2":
        sc = rib.RibScene(os.path.join(ROOT, "tests", "golden", "rib", "ambient_occlusion.rib"))
        sc.add_to(acc)
        ms = [m["positions"][:, :3] for m in sc.meshes()]
        cam = la.Camera.make(args.size, args.size, sc.camera.flength, list(sc.camera.cam2world), sc.camera.rh)
        ps = int(sc.info.pixel_samples[0])
        sc.close()
    else:
        g = np.load(os.path.join(ROOT, "tests", "golden", "ao_c1.npz"))
        ms = []
        for k in range(int(g["ngeoms"])):
            P, I = scenes.tessellate(g["pos%d" % k], g["idx%d" % k], args.tess)
            acc.add_mesh(P, I); ms.append(P); del I
        c = g["camera"]
        cam = la.Camera.make(args.size, args.size, c[16], c[:16], int(c[19])); ps = 1
    lo = np.min([m.min(0) for m in ms], axis=0); hi = np.max([m.max(0) for m in ms], axis=0)
    for k, P in enumerate(ms):
        acc.set_attribute(k, la.ATTR_TEXCOORD, planar_st(P, lo, hi))
    ntri = acc.commit()["ntriangles"]; acc.wait_exact()
    what = "%s: %d triangles in %d meshes, %d x %d, %d x %d pixel samples, %d AO samples" % (name, ntri, len(ms), args.size, args.size, ps, ps, NS)
    return acc, cam, ps, what


def window_ms(fn):
    """ms per call of fn (synchronous) over >= args.window seconds of back-to-back calls"""
    t0 = time.perf_counter(); fn(); one = time.perf_counter() - t0
    k = max(2, int(np.ceil(1.15 * args.window / max(one, 1e-6))))
    while True:
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        dt = time.perf_counter() - t0
        if dt >= args.window:
            return dt / k * 1e3
        k = int(np.ceil(k * 1.3 * args.window / dt))


def spread(x):
    return (max(x) - min(x)) / float(np.median(x))


if args.child:
    acc, cam, ps, _ = scene(args.child)
    out = torch.empty((args.size, args.size, 3), dtype=torch.float32, device="cuda")
    frame = lambda: acc.render_ao_tile(cam, 0, 0, args.size, args.size, ps, NS, seed=1, out=out)      # noqa: E731
    frame(); frame()
    print(json.dumps({"ms": window_ms(frame), "checksum": float(out.double().sum().item())}), flush=True)
    acc.close()
    sys.exit(0)

result = {"repeats": args.repeats, "window_s": args.window, "texture": args.texture, "scenes": {}}
tex = np.random.default_rng(1).uniform(0.1, 1.0, (args.texture, args.texture, 4)).astype(np.float32)
for name in args.scenes.split(","):
    acc, cam, ps, what = scene(name)
    say("== " + what)
    out = torch.empty((args.size, args.size, 3), dtype=torch.float32, device="cuda")
    stats = {}

    def frame():
        stats.update(acc.render_ao_tile(cam, 0, 0, args.size, args.size, ps, NS, seed=1, out=out)[1])

    frame(); plain = out.clone(); st_plain = dict(stats)
    acc.set_texture(la.ALL_MESHES, tex); frame(); textured = out.clone(); st_tex = dict(stats)
    grey = bool((plain[..., 0] == plain[..., 1]).all()); coloured = bool((textured[..., 0] != textured[..., 1]).any())
    a_ms, b_ms = [], []
    for _ in range(args.repeats):
        acc.set_texture(la.ALL_MESHES, None); frame(); a_ms.append(window_ms(frame))
        acc.set_texture(la.ALL_MESHES, tex); frame(); b_ms.append(window_ms(frame))
    acc.set_texture(la.ALL_MESHES, None); frame()
    same_after = bool(torch.equal(out, plain))
    # a plain copy of the frame's sample records: prim (4) + u (8) + v (8) bytes per camera sample
    S = args.size * args.size * ps * ps
    src = (torch.zeros(S, dtype=torch.int32, device="cuda"), torch.zeros(S, dtype=torch.float64, device="cuda"), torch.zeros(S, dtype=torch.float64, device="cuda"))
    dst = tuple(torch.empty_like(x) for x in src)

    def copy():
        for d, s in zip(dst, src):
            d.copy_(s)
        torch.cuda.synchronize()

    copy(); c_ms = [window_ms(copy) for _ in range(args.repeats)]
    diff = [b - a for a, b in zip(a_ms, b_ms)]
    res = {"what": what, "samples": S, "stats_equal": st_plain == st_tex, "untextured_is_grey": grey, "textured_is_coloured": coloured,
           "untextured_again_bit_equal": same_after, "a_untextured_ms": [round(x, 3) for x in a_ms], "b_textured_ms": [round(x, 3) for x in b_ms],
           "b_minus_a_ms": [round(x, 3) for x in diff], "a_spread": round(spread(a_ms), 4), "record_copy_ms": [round(x, 4) for x in c_ms],
           "b_minus_a_over_copy": round(float(np.median(diff)) / float(np.median(c_ms)), 2)}
    say("(a) untextured %s ms  (b) textured %s ms  (b) - (a) %s ms (median %.3f; (a)'s own spread %.4f)" % (
        res["a_untextured_ms"], res["b_textured_ms"], res["b_minus_a_ms"], float(np.median(diff)), res["a_spread"]))
    say("a plain copy of the %d sample records (20 bytes each): %s ms; (b) - (a) is %.2f of it; statistics equal: %s; untextured again bit-equal: %s" % (
        S, res["record_copy_ms"], res["b_minus_a_over_copy"], res["stats_equal"], res["untextured_again_bit_equal"]))
    acc.close(); del out, plain, textured, src, dst
    torch.cuda.empty_cache()
    if args.parent_lib:
        libs = {"parent": os.path.abspath(args.parent_lib), "this": os.path.join(ROOT, "lucille_amd", "csrc", "liblucille_hip.so")}
        ms = {"parent": [], "this": []}; sums = set()
        for _ in range(args.repeats):
            for tag in ("parent", "this"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--size", str(args.size), "--tess", str(args.tess), "--window", str(args.window)]
                p = subprocess.run(cmd, env=dict(os.environ, LH_LIBRARY=libs[tag]), capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    raise SystemExit("child (%s) failed: %s" % (tag, p.stderr[-2000:]))
                r = json.loads(p.stdout.strip().splitlines()[-1]); ms[tag].append(r["ms"]); sums.add(r["checksum"])
        d = float(np.median(ms["this"])) - float(np.median(ms["parent"]))
        res["vs_parent"] = {"parent_ms": [round(x, 3) for x in ms["parent"]], "this_ms": [round(x, 3) for x in ms["this"]], "median_difference_ms": round(d, 3),
                            "parent_spread_ms": round(max(ms["parent"]) - min(ms["parent"]), 3), "frames_equal": len(sums) == 1}
        say("(a) against the parent's build, alternating processes: parent %s ms, this tree %s ms; medians differ by %.3f ms, the parent's own windows by %.3f ms; frames equal: %s" % (
            res["vs_parent"]["parent_ms"], res["vs_parent"]["this_ms"], d, res["vs_parent"]["parent_spread_ms"], res["vs_parent"]["frames_equal"]))
    result["scenes"][name] = res
say(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
