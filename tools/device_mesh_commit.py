"""Commit from host arrays against commit from device tensors, on S-soup-1M and on the BASELINE config-5 scene (the AO example
scene tessellated 8 times: 21.1 M triangles).  Per scene, in ONE child process:
  (host)   lh_accel_add_mesh per mesh + lh_accel_commit(LH_BUILD_ON_DEVICE) + lh_accel_wait_exact: the host flatten, the
           tri64 upload, then the device builders;
  (device) lh_accel_add_mesh_device per mesh from tensors already on the device + lh_accel_commit: the flatten kernel, then the
           same builders.
Each is run `repeats` times, alternating; wall times of every run and the LH_BUILD_TIMING phase lines of the last pair are
printed, and a ray batch is traced on both accelerators (the records must be equal).  What (device) does NOT include is what a
caller whose vertices are produced on the GPU no longer pays: it would have had to copy them to the host first.
With --attributes every mesh also gets per-vertex normals and colours (seeded; lh_accel_set_normals / _set_attribute from host
arrays, lh_accel_set_normals_device / _set_attribute_device from tensors): each run then commits four ways -- host arrays and
device tensors, without and with the attributes -- so the cost of the attribute gather is read against the commit without
attributes of the same run, beside the host-array build with the same attributes.
Every GPU step is a fresh child under its own `timeout`; a failing child stops the run.
    python tools/device_mesh_commit.py [--out FILE] [--repeats N] [--scenes soup1m,config5] [--attributes]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"soup1m": 240, "config5": 540}          # seconds a child may take


def child(scene, repeats, attributes=False):
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
    dmeshes = [(torch.from_numpy(P).cuda(), torch.from_numpy(I.view(np.int32)).cuda()) for P, I in meshes]
    attrs = dattrs = None
    if attributes:
        rng = np.random.default_rng(12)
        attrs = []
        for P, _ in meshes:
            N = rng.normal(size=P.shape); N /= np.linalg.norm(N, axis=1, keepdims=True)
            attrs.append((N, rng.uniform(0, 1, P.shape)))
        dattrs = [(torch.from_numpy(N).cuda(), torch.from_numpy(Cl).cuda()) for N, Cl in attrs]
    torch.cuda.synchronize()
    print("scene %s: %d meshes, %d triangles, %s" % (scene, len(meshes), ntri, torch.cuda.get_device_name(0)), flush=True)

    def host(with_attrs=False):
        t0 = time.perf_counter()
        a = la.HipAccel(0)
        for k, (P, I) in enumerate(meshes):
            a.add_mesh(P, I)
            if with_attrs:
                a.set_normals(k, attrs[k][0]); a.set_attribute(k, la.ATTR_COLOR, attrs[k][1])
        a.commit(on_device=True); a.wait_exact()
        return a, time.perf_counter() - t0

    def device(with_attrs=False):
        t0 = time.perf_counter()
        a = la.HipAccel(0)
        for k, (P, I) in enumerate(dmeshes):
            a.add_mesh_device(P, I)
            if with_attrs:
                a.set_normals_device(k, dattrs[k][0]); a.set_attribute_device(k, la.ATTR_COLOR, dattrs[k][1])
        a.commit()
        return a, time.perf_counter() - t0

    quiet = os.environ.pop("LH_BUILD_TIMING", None)
    th, td, tha, tda = [], [], [], []
    for r in range(repeats):
        last = r == repeats - 1
        if last:
            os.environ["LH_BUILD_TIMING"] = "1"
            sys.stderr.flush(); print("--- phase lines, host arrays (run %d)" % r, flush=True)
        ah, s = host(); th.append(s)
        if last:
            sys.stderr.flush(); print("--- phase lines, device tensors (run %d)" % r, flush=True)
        ad, s = device(); td.append(s)
        if last:
            sys.stderr.flush()
            os.environ.pop("LH_BUILD_TIMING", None)
            ra = ah.intersect_host(org, dr); rb = ad.intersect_host(org, dr)
            same = all(np.array_equal(x, y) for x, y in zip(ra, rb))
            ih, idv = ah.info(), ad.info()
            print("--- records of %d rays equal: %s (%d hits); nodes %d / %d, triangles in tree %d / %d"
                  % (org.shape[0], same, int((ra[0] != la.MISS).sum()), ih["nnodes_traversal"], idv["nnodes_traversal"], ih["ntriangles_in_tree"], idv["ntriangles_in_tree"]), flush=True)
            assert same
        ah.close(); ad.close()
        if attributes:
            if last:
                os.environ["LH_BUILD_TIMING"] = "1"
                sys.stderr.flush(); print("--- phase lines, host arrays with normals and colours (run %d)" % r, flush=True)
            ah, s = host(True); tha.append(s)
            if last:
                sys.stderr.flush(); print("--- phase lines, device tensors with normals and colours (run %d)" % r, flush=True)
            ad, s = device(True); tda.append(s)
            if last:
                sys.stderr.flush()
                os.environ.pop("LH_BUILD_TIMING", None)
                n = min(org.shape[0], 20000)
                ra = ah.intersect_host(org[:n], dr[:n]); rb = ad.intersect_host(org[:n], dr[:n])
                sa = ah.state_build(org[:n], dr[:n], *ra); sb = ad.state_build(org[:n], dr[:n], *rb)
                same = all(np.array_equal(x, y) for x, y in zip(ra, rb)) and sa.tobytes() == sb.tobytes()
                print("--- hit records and state records of %d rays equal: %s" % (n, same), flush=True)
                assert same
            ah.close(); ad.close()
    if quiet is not None:
        os.environ["LH_BUILD_TIMING"] = quiet
    fmt = lambda v: " ".join("%.1f" % (1e3 * x) for x in v)          # noqa: E731
    print("commit wall, host arrays   (add_mesh + commit on device + wait_exact), ms per run: %s" % fmt(th))
    print("commit wall, device tensors (add_mesh_device + commit),                ms per run: %s" % fmt(td))
    print("last run: host arrays %.1f ms, device tensors %.1f ms, ratio %.2f" % (1e3 * th[-1], 1e3 * td[-1], th[-1] / td[-1]), flush=True)
    if attributes:
        print("commit wall, host arrays with normals and colours,    ms per run: %s" % fmt(tha))
        print("commit wall, device tensors with normals and colours, ms per run: %s" % fmt(tda))
        print("last run: device tensors %.1f ms without, %.1f ms with the attributes (+%.1f ms, x%.3f); host arrays with them %.1f ms"
              % (1e3 * td[-1], 1e3 * tda[-1], 1e3 * (tda[-1] - td[-1]), tda[-1] / td[-1], 1e3 * tha[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--scenes", default="soup1m,config5")
    ap.add_argument("--child"); ap.add_argument("--attributes", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats, a.attributes)
    text = []
    for scene in a.scenes.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[scene]), sys.executable, os.path.abspath(__file__), "--child", scene, "--repeats", str(a.repeats)] + (["--attributes"] if a.attributes else [])
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
