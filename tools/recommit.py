"""Re-commit in place against destroy + create + add + set + commit, on S-soup-1M and on the BASELINE config-5 scene (the AO example scene
tessellated 8 times: 21.1 M triangles).  Every mesh carries a colour per vertex.  Per scene, in ONE child process, three cases:
  (a) every vertex jittered: lh_accel_update_mesh_device per mesh + lh_accel_recommit;
  (b) a new colour array per mesh and nothing else: lh_accel_set_attribute_device per mesh + lh_accel_recommit (no tree is built);
  (c) the positions handed over again unchanged: update + re-commit (flatten, compare, the trees stand);
each against the same geometry and attributes through the only way there was before: lh_accel_destroy, lh_accel_create, lh_accel_add_mesh_device
and lh_accel_set_attribute_device per mesh, lh_accel_commit.  The candidate and the baseline alternate in windows of `--window` seconds (1) in one
process, `--windows` (3) each; per window the mean wall time of an operation is printed with the window's median and slowest operation (a window
that one operation dominates is marked: a stall), then the baseline's own spread (max - min over its windows) beside the difference, for the
means and for the medians, the slowest re-commit of every window split into its staging calls and the lh_accel_recommit call, and the LH_BUILD_TIMING phase lines of one operation of each kind once.  A ray batch is traced after the last
(a) on both accelerators: the records must be equal.
Every GPU step is a fresh child under its own `timeout`; a failing child stops the run.
    python tools/recommit.py [--out FILE] [--scenes soup1m,config5] [--window S] [--windows N]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"soup1m": 240, "config5": 540}          # seconds a child may take


def child(scene, window, windows):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import lucille_amd as la
    from lucille_amd import scenes
    if scene == "soup1m":
        P, idx, st = scenes.soup_triangles(1000000, 0.005)
        meshes = [(P, idx)]
        org, dr, _ = scenes.soup_rays(200000, st)
    else:
        g = np.load(os.path.join(ROOT, "tests", "golden", "ao_c1.npz"))
        meshes = [scenes.tessellate(g["pos%d" % k], g["idx%d" % k], 8) for k in range(int(g["ngeoms"]))]
        allp = np.concatenate([m[0][::997] for m in meshes]); lo, hi = allp.min(0), allp.max(0)
        rng = np.random.default_rng(4)
        org = rng.uniform(lo - 1, hi + 1, (200000, 3)); dr = rng.uniform(lo, hi, (200000, 3)) - org
    ntri = sum(m[1].shape[0] // 3 for m in meshes)
    ext = float(max(np.ptp(m[0], axis=0).max() for m in meshes))
    dI = [torch.from_numpy(I.view(np.int32)).cuda() for _, I in meshes]
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    base = [torch.from_numpy(P).cuda() for P, _ in meshes]
    # two jittered placements (every vertex moves by up to 1e-4 of the scene's extent) and two colour arrays: the operations alternate between them
    pos = [[b + (torch.rand(b.shape, generator=gen, device="cuda", dtype=torch.float64) - 0.5) * (2e-4 * ext) for b in base] for _ in range(2)]
    col = [[torch.rand(b.shape, generator=gen, device="cuda", dtype=torch.float64) for b in base] for _ in range(2)]
    torch.cuda.synchronize()
    print("scene %s: %d meshes, %d triangles, %s" % (scene, len(meshes), ntri, torch.cuda.get_device_name(0)), flush=True)

    def fresh(p, c, updatable):
        a = la.HipAccel(0)
        if updatable:
            a.set_param("updatable", 1)
        for k in range(len(base)):
            a.add_mesh_device(p[k], dI[k]); a.set_attribute_device(k, la.ATTR_COLOR, c[k])
        a.commit()
        return a

    state = {"acc": fresh(pos[0], col[0], True), "ref": fresh(pos[0], col[0], False), "n": 0, "k": 0, "slow": (0.0, 0.0, 0.0, 0.0)}

    def recommit(t0):
        """the re-commit behind the staging calls that began at t0; remembers the slowest operation: (wall, staging, re-commit call, the library's own seconds), ms"""
        t1 = time.perf_counter()
        r = state["acc"].recommit()
        t2 = time.perf_counter()
        op = (1e3 * (t2 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * r["recommit_seconds"])
        if op[0] > state["slow"][0]:
            state["slow"] = op
        return r

    def cand_a():
        t0 = time.perf_counter()
        state["k"] += 1; p = pos[state["k"] & 1]
        for k in range(len(base)):
            state["acc"].update_mesh_device(k, p[k])
        return recommit(t0)

    def cand_b():
        t0 = time.perf_counter()
        state["k"] += 1; c = col[state["k"] & 1]
        for k in range(len(base)):
            state["acc"].set_attribute_device(k, la.ATTR_COLOR, c[k])
        return recommit(t0)

    def cand_c():
        t0 = time.perf_counter()
        for k in range(len(base)):
            state["acc"].update_mesh_device(k, state["placed"][k])
        return recommit(t0)

    def baseline():
        state["n"] += 1
        state["ref"].close()
        state["ref"] = fresh(pos[state["n"] & 1], col[state["n"] & 1], False)

    def run_window(f):
        """(mean ms per operation, operations, median ms, slowest ms) of one window"""
        ops, t0 = [], time.perf_counter()
        while True:
            ta = time.perf_counter(); f(); tb_ = time.perf_counter()
            ops.append(1e3 * (tb_ - ta))
            if tb_ - t0 >= window:
                ops.sort()
                return 1e3 * (tb_ - t0) / len(ops), len(ops), ops[len(ops) // 2], ops[-1]

    def show(w):
        # "!": one operation is more than half of the window's time -- a stall; the mean of such a window says little, its median is the ordinary operation
        return "  ".join("%.2f (%d; median %.2f, slowest %.2f%s)" % (m, n, med, mx, " !" if mx > 0.5 * m * n and n > 1 or mx > 3.0 * med else "") for m, n, med, mx in w)

    quiet = os.environ.pop("LH_BUILD_TIMING", None)
    for name, cand, want in (("(a) every vertex jittered", cand_a, (1, 1, 1)), ("(b) colours only", cand_b, (0, 0, 1)), ("(c) positions unchanged", cand_c, (1, 0, 1))):
        if cand is cand_c:                                 # the placement the accelerator holds now, handed over again and again
            state["placed"] = pos[0]
            for k in range(len(base)):
                state["acc"].update_mesh_device(k, pos[0][k])
            state["acc"].recommit()
        r = cand(); baseline()                             # warm: allocator pools
        r = cand()
        assert (r["flattened"], r["rebuilt_trees"], r["regathered"]) == want, (name, r)
        tc, tb, slow = [], [], []
        for _ in range(windows):
            state["slow"] = (0.0, 0.0, 0.0, 0.0)
            tc.append(run_window(cand)); tb.append(run_window(baseline))
            slow.append(state["slow"])
        os.environ["LH_BUILD_TIMING"] = "1"
        sys.stderr.flush(); print("--- %s: phase lines of one re-commit" % name, flush=True)
        cand(); sys.stderr.flush()
        print("--- %s: phase lines of one destroy + create + add + set + commit" % name, flush=True)
        baseline(); sys.stderr.flush()
        os.environ.pop("LH_BUILD_TIMING", None)
        mc = sum(w[0] for w in tc) / len(tc); mb = sum(w[0] for w in tb) / len(tb)
        spread = max(w[0] for w in tb) - min(w[0] for w in tb)
        dc = sorted(w[2] for w in tc)[len(tc) // 2]; db = sorted(w[2] for w in tb)[len(tb) // 2]
        dspread = max(w[2] for w in tb) - min(w[2] for w in tb)
        print("%s, mean ms per operation in windows of %.1f s (operations per window; the window's median and slowest operation; ! = a stall):" % (name, window))
        print("    re-commit in place:                    %s" % show(tc))
        print("    destroy, create, add, set, commit:     %s" % show(tb))
        print("    slowest re-commit of each window, ms:  %s" % "  ".join("%.2f = staging %.2f + call %.2f (the library's own %.2f)" % x for x in slow))
        verdict = "faster" if mc < mb - spread else ("SLOWER by more than the baseline's spread" if mc > mb + spread else "within the baseline's spread")
        print("    window means %.2f / %.2f ms, ratio %.2f; the baseline's own spread %.2f ms: the re-commit is %s" % (mc, mb, mb / mc, spread, verdict))
        dverdict = "faster" if dc < db - dspread else ("SLOWER by more than the baseline's spread" if dc > db + dspread else "within the baseline's spread")
        print("    window medians %.2f / %.2f ms, ratio %.2f; the spread of the baseline's medians %.2f ms: the ordinary re-commit is %s" % (dc, db, db / dc, dspread, dverdict), flush=True)
        if cand is cand_a:
            # both accelerators at the same placement: the same records
            state["ref"].close(); state["ref"] = fresh(pos[state["k"] & 1], col[0], False)
            ra = state["acc"].intersect_host(org, dr); rb = state["ref"].intersect_host(org, dr)
            same = all(np.array_equal(x, y) for x, y in zip(ra, rb))
            print("--- records of %d rays equal after the re-commits: %s (%d hits)" % (org.shape[0], same, int((ra[0] != la.MISS).sum())), flush=True)
            assert same
    if quiet is not None:
        os.environ["LH_BUILD_TIMING"] = quiet
    state["acc"].close(); state["ref"].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--scenes", default="soup1m,config5"); ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--windows", type=int, default=3); ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.window, a.windows)
    text = []
    for scene in a.scenes.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[scene]), sys.executable, os.path.abspath(__file__), "--child", scene, "--window", str(a.window), "--windows", str(a.windows)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        out = r.stdout.decode()
        print(out, end="", flush=True); text.append(out)
        if r.returncode != 0:
            msg = "child for %s ended with status %d: stopping\n" % (scene, r.returncode)
            print(msg, end=""); text.append(msg)
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(text))
    return 0 if r.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
