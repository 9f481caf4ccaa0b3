"""The fused gather stages' kernels, one launch of every instantiation (lucille_amd/csrc/lh_kernels.hip: k_trace_persist_stage<KIND, COUNT, WALK>,
k_coop_walk_stage<KIND>, picked by launch_stage<KIND> from the kind's row).  A wrong cell of that dispatch -- counted for uncounted, checked pushes for the
default walk, one kind's row for another's -- is what this file is for: the kinds' own files launch the checked walk and the counting kernels for some
kinds only.

The cells: every kind (AO, dirt, environment, lights, area lights) x the default walk and "stack_cap" 8 (checked pushes) x trace statistics off and on
(the counted instantiations) x the default visit budget and "ao_budget" 4 (rays leave the persistent kernel for the cooperative stage kernel).

The batch: the first 257 rays of the lights tests' soup with their closest-hit records (hits and misses), a list of their ids with one id twice and two
ids beyond the batch, and a device-resident count that cuts the list's tail.

Per cell: the kind's *_device answer with "ao_fused" 1 equals, bit for bit, the same call with "ao_fused" 0 -- the materialised path launches ray dumps
only, kernels whose device code the stage kernels' change does not touch (profiles/stage_kernels.md) -- and both equal the oracle expectation of the
kind's own test file.  With statistics on, `rays` is slots x N.  With the small budget, statistics on and a kind other than AO,
lh_accel_last_retraced is above 0: rays went through the queue.

What the binding does not show.  (a) lh_accel_last_retraced is set by a batch entry point only under trace statistics and not for the AO kind
(lh_tile.hip ao_batch_device): in the other small-budget cells the same rays meet the same budget, but the queue's traffic is not observed.  (b) Whether
a batch entry point's stage ENDED fused is not reported.  It cannot have fallen back here: the one fallback is the fix-up queue's overflow flag, set by
the push that finds LH_AO_QCAP = 2^22 entries (lh_device.h), a ray is pushed at most once, and every cell holds fewer rays than that (asserted); and
the plan is fused for "ao_fused" 1, fewer than 2^31 rays and no replayed uniforms (lh_gather.h)."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests import test_gpu_area as ta
from tests import test_gpu_dirt as td
from tests import test_gpu_envgather as te
from tests.test_gpu_ao_batch import NO_HIT, POISON32, POISONF, ao_rays, dev, host
from tests.test_gpu_ao_batch import expected as ao_expected
from tests.test_gpu_lights import EPS, FIVE, ls  # noqa: F401  (ls: the soup's fixture)
from tests.test_gpu_lights import expected as lights_expected
from tests.test_gpu_lights import mk as mk_lights

pytestmark = pytest.mark.gpu

B = 257
NS = 16                      # gather_nsamples of the sampled kinds: N = 16
AREA = "three"               # test_gpu_area.py's set: three lights, four samples each
N_OF = {"ao": NS, "dirt": NS, "env": NS, "light": len(FIVE), "area": len(ta.SETS[AREA][0]) * ta.SETS[AREA][1]}
QCAP = 1 << 22               # LH_AO_QCAP


@pytest.fixture(scope="module")
def stage(ls):  # noqa: F811
    """the batch, its list, an accelerator per (stack_cap, ao_budget) on the soup, and the kinds' expectations -- made once, never changed"""
    import torch
    org, dr = ls["org"][:B].contiguous(), ls["dr"][:B].contiguous()
    rec = tuple(x[:B].contiguous() for x in ls["rec"])
    hit = ls["prim"][:B] != po.MISS
    assert 0 < int(hit.sum()) < B
    lst = np.random.default_rng(17).permutation(B).astype(np.uint32)
    lst[7] = lst[3]; lst[11] = B + 2; lst[100] = B + 40          # an id twice, two ids beyond the batch
    count = B - 9                                                # the device-resident count cuts the list
    ent = lst[:count]; ent = ent[ent < B]
    listed = np.zeros(B, bool); listed[ent] = True
    assert listed.sum() < B and (listed & hit).any() and (listed & ~hit).any() and (~listed & hit).any()
    accs = {}
    for cap in (0, 8):
        for budget in (0, 4):
            a = la.HipAccel(0); a.add_mesh(ls["P"], ls["idx"]); a.commit(); a.wait_exact()
            a.set_emitters(ta.TABLE); a.set_environment(te.RGB, te.sky())
            if cap:
                a.set_param("stack_cap", cap)
            if budget:
                a.set_param("ao_budget", budget)
            accs[(cap, budget)] = a
    s = {"accs": accs, "org": org, "dr": dr, "rec": rec, "hit": hit, "listed": listed, "slots": int(hit[ent].sum()),
         "index": dev(lst), "count": torch.tensor([count], dtype=torch.int32, device="cuda"), "exp": {}, "ls": ls,
         "area_ls": dict(ls, exp={})}
    yield s
    for a in accs.values():
        a.close()


def expectation(s, kind):
    """-> (word uint32 [B], value float32 [B(, 3)], skip uint32 [B]: the bits of `word` outside the contract) of every ray of the batch, by the oracle
    and the restatements of the kind's own test file; (dirt: with its parameters)"""
    if kind in s["exp"]:
        return s["exp"][kind]
    ls_, acc = s["ls"], s["accs"][(0, 0)]
    skip = np.zeros(B, np.uint32)
    if kind == "ao":
        slot, nslots, aorg, adir = ao_rays(acc, s["org"], s["dr"], s["rec"], NS, seed=3)
        occ = ls_["oracle"].intersect(aorg, adir, nthreads=8)[0] != po.MISS
        e = ao_expected(slot, occ, NS) + (skip, None)
    elif kind in ("dirt", "env"):
        if "gather" not in s["exp"]:
            slot, nslots, go, gd = td.gather_rays(acc, s["org"], s["dr"], s["rec"], NS, EPS, seed=3)
            s["exp"]["gather"] = (slot, gd) + td.oracle_t(ls_["oracle"], go, gd)
        slot, gd, t, h = s["exp"]["gather"]
        if kind == "dirt":
            near, far = float(np.percentile(t[h], 25)), float(np.percentile(t[h], 75))
            e = td.scatter(slot, *td.values(t, h, NS, near, far)) + (skip, la.DirtParams(near, far, EPS))
        else:
            e = te.scatter(slot, *te.values(h, te.colours(acc, gd), NS, 1.0)) + (skip, None)
    else:
        k = int(np.searchsorted(ls_["ids"], B))          # the batch's hits are the soup's first k slots
        if kind == "light":
            _, out, mask, val, _ = lights_expected(ls_, "five")
            bits = (out[:k].astype(np.uint32) << np.arange(out.shape[1], dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
        else:
            x = ta.expected(s["area_ls"], AREA)
            assert not x["outside"].any()
            mask, val, bits = x["mask"], x["val"], np.zeros(k, np.uint32)
        ids = ls_["ids"][:k]
        m = np.full(B, NO_HIT, np.uint32); m[ids] = mask[:k]
        v = np.zeros((B, 3), np.float32); v[ids] = val[:k]
        skip[ids] = bits
        e = (m, v, skip, None)
    for a in e[:3]:
        a.setflags(write=False)
    s["exp"][kind] = e
    return e


def call(s, kind, acc, fused):
    """the kind's *_device over the list, into poisoned outputs, with "ao_fused" set for the call -> (word uint32 [B], value float32) on the host"""
    import torch
    word = torch.full((B,), POISON32, dtype=torch.int32, device="cuda")
    value = torch.full((B,) if kind in ("ao", "dirt") else (B, 3), POISONF, dtype=torch.float32, device="cuda")
    o, d, rec = s["org"], s["dr"], s["rec"]
    kw = {"index": s["index"], "count": s["count"], "out": (word, value)}
    acc.set_param("ao_fused", fused)
    try:
        if kind == "ao":
            acc.ao_device(o, d, rec, NS, 3, **kw)
        elif kind == "dirt":
            acc.dirt_device(o, d, rec, NS, expectation(s, "dirt")[3], 3, **kw)
        elif kind == "env":
            acc.env_device(o, d, rec, NS, la.EnvParams(EPS, 1.0), 3, **kw)
        elif kind == "light":
            acc.lights_device(o, d, rec, mk_lights(FIVE), la.LightsParams(EPS), **kw)
        else:
            lights, S = ta.SETS[AREA]
            acc.area_lights_device(o, d, rec, ta.mk(lights), ta.prm(S), ta.SEED, **kw)
    finally:
        acc.set_param("ao_fused", 1)
    return host(word, np.uint32).copy(), host(value).copy()


@pytest.mark.parametrize("budget", [0, 4])
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("cap", [0, 8])
@pytest.mark.parametrize("kind", ["ao", "dirt", "env", "light", "area"])
def test_every_instantiation_answers_as_the_materialised_stage(stage, kind, cap, stats, budget):
    s = stage
    acc = s["accs"][(cap, budget)]
    eword, evalue, skip, _ = expectation(s, kind)
    rays = s["slots"] * N_OF[kind]
    assert 0 < rays < QCAP                       # no queue overflow is possible: the fused call ends fused (see above)
    st, queued = None, None
    acc.trace_statistics(stats)
    try:
        if stats:
            acc.statistics(clear=True)
        wf, vf = call(s, kind, acc, 1)
        if stats:
            st = acc.statistics(clear=True)
            queued = int(acc.L.lh_accel_last_retraced(acc.h))
        wm, vm = call(s, kind, acc, 0)
    finally:
        acc.trace_statistics(False)
    on = s["listed"]
    print("%s cap %d stats %d budget %d: %d rays; fused != materialised at %d words, %d values; fused != oracle at %d words; statistics %s; queued %s"
          % (kind, cap, stats, budget, rays, int((wf != wm).sum()), int((vf.view(np.uint32) != vm.view(np.uint32)).sum()),
             int((((wf ^ eword) & ~skip)[on] != 0).sum()), st, queued))
    # 1. the fused stage against the materialised one: every word of both outputs, the poison of the slots that are not listed included
    assert np.array_equal(wf, wm) and td.same_bits(vf, vm)
    assert (wf[~on] == POISON32).all() and (vf[~on] == np.float32(POISONF)).all()
    # 2. both against the oracle (a light's bit outside the contract, and the value of its hit, left out as in test_gpu_lights.py)
    assert np.array_equal(wf[on] & ~skip[on], eword[on] & ~skip[on])
    whole = on & (skip == 0)
    assert td.same_bits(vf[whole], evalue[whole])
    assert (wf[on & ~s["hit"]] == NO_HIT).all()
    # 3. the counted instantiations count the work items; the small budget sends rays through the queue
    if stats:
        assert st["rays"] == rays, st
        assert st["nodes"] > 0, st          # counted by the persistent kernel alone: every ray that starts a walk there visits the root (an item kind's
                                            # `rays` is made on the host, and would not show a counting kernel that did not run)
        if budget and kind != "ao":
            assert 0 < queued <= rays, queued
