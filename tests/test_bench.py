"""bench.py's plain run (the headline alone) and --dump-outputs: the sample of hit records it writes is the records of those
rays, on the GPU at N = 1 and through the decoding of rank 0's gathered slabs at N > 1 (host tensors, no GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import lucille_amd as la
from benchlegs.common import record_views
from lucille_amd import shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wire,mode", [(16, la.MODE_CLOSEST), (28, la.MODE_CLOSEST), (1, la.MODE_ANY)])
def test_gathered_records_decode_every_rank_and_chunk(wire, mode):
    import torch
    world, n_total, nchunks = 3, 100_003, 4
    per = shard.chunk_capacity(n_total, world, nchunks)
    slices = [shard.ray_slice(n_total, r, world) for r in range(world)]
    gathered = [torch.zeros((world, per * wire), dtype=torch.uint8) for _ in range(nchunks)]
    for r, (b0, b1) in enumerate(slices):           # record of ray g: prim g, t g / 2, u g / 4, v -g; occluded g % 2
        for c in range(nchunks):
            lo, hi = c * per, min(b1 - b0, (c + 1) * per)
            if hi <= lo:
                continue
            g = torch.arange(b0 + lo, b0 + hi)
            if wire == 16:
                rec = gathered[c][r].view(torch.int32).view(per, 4)
                rec[:hi - lo, 0] = g.int()
                for k, f in ((1, 0.5), (2, 0.25), (3, -1.0)):
                    rec[:hi - lo, k].view(torch.float32)[:] = g.float() * f
            elif wire == 28:
                row = torch.zeros(per * 28, dtype=torch.uint8)
                p, t, u, v = record_views(torch, row, per)
                p[:hi - lo] = g.int(); t[:hi - lo] = g.double() * 0.5; u[:hi - lo] = g.double() * 0.25; v[:hi - lo] = -g.double()
                gathered[c][r] = row
            else:
                gathered[c][r][:hi - lo] = (g % 2).to(torch.uint8)
    ix = torch.from_numpy(np.unique(np.random.default_rng(7).integers(0, n_total, 5000)))
    starts = torch.tensor([b0 for b0, _ in slices])
    out = bench.gathered_records(torch, la, mode, ix, gathered, starts, per, wire)
    if mode == la.MODE_CLOSEST:
        assert torch.equal(out[0].long(), ix)
        for k, f in ((1, 0.5), (2, 0.25), (3, -1.0)):
            assert torch.equal(out[k].double(), ix.double() * f)
    else:
        assert torch.equal(out[0].long(), ix % 2)


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_steps_records(tmp_path):
    import torch
    from lucille_amd import scenes
    nrays, ntris, he = 2_000_000, 100_000, 0.01
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rays", str(nrays),
           "--tris", str(ntris), "--half-extent", str(he), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l][-1])
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "Mrays/s" and j["higher_is_better"] is True
    assert abs(j["value"] - nrays / j["ms_per_step"] / 1e3) <= 0.01 * j["value"]
    for leg in ("roofline", "validation", "cpu_baseline", "roofline_hbm", "ao_render", "pt_render", "config2", "host_path"):
        assert leg not in j, leg
    d = {f[:-4]: np.load(str(tmp_path / "out" / f)) for f in os.listdir(str(tmp_path / "out"))}
    assert sorted(d) == ["prim", "ray_index", "t", "u", "v"]
    assert all(a.dtype in (np.float32, np.float64) for a in d.values()) and sum(a.nbytes for a in d.values()) <= 64 << 20
    ix = d["ray_index"].astype(np.int64)          # the fixed sample of the dump's rays: the same in every run
    assert np.array_equal(ix, np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, nrays, bench.DUMP_RAYS)))
    # the same scene and rays, traced here: the dumped records are those of the dump's rays
    P, idx, st = scenes.soup_triangles(ntris, he)
    org, dr, _ = scenes.soup_rays(nrays, st)
    acc = la.HipAccel(0)
    acc.add_mesh(P, idx)
    acc.commit()
    exp = acc.intersect_device(torch.from_numpy(org).cuda(), torch.from_numpy(dr).cuda())
    torch.cuda.synchronize()
    acc.close()
    assert np.array_equal(d["prim"], exp[0].cpu().numpy()[ix].astype(np.float64))
    for k, name in ((1, "t"), (2, "u"), (3, "v")):
        assert np.array_equal(d[name], exp[k].cpu().numpy()[ix])
