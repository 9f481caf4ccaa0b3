"""Generate tests/golden/whitted_bounce.npz and tests/golden/whitted_chain.npz by running the COMPILED REFERENCE (oracle/_ref/
liblucille_ref.so, built from the reference tree by oracle/Makefile) through ctypes.  The fixtures are data; no reference source is stored.

  whitted_bounce.npz: the cases of tests/test_whitted_rule.py (by seed) and what the reference's ri_refract returned for each: the
      direction and the total-reflection flag.
  whitted_chain.npz:  the chain loop of tests/whitted_chain.py over po.soup(300, 2000, 0.2, 5) with the reference's own intersect, state
      and ri_refract (eps 1e-7, eta 1.33, depth 8: the constants of whitted.c): bounces of every ray, the end rays of the eye hits.

    python tests/golden/make_whitted_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from tests import test_whitted_rule as tr  # noqa: E402
from tests import whitted_chain as wc  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    lib = C.CDLL(tr.REFLIB)
    I, N, eta, P, eps = tr.cases()
    R, tir = tr.reference_refract(lib, I, N, eta)
    path = os.path.join(OUT, "whitted_bounce.npz")
    np.savez_compressed(path, I=I, n=N, eta=eta, R=R, tir=tir)
    print("wrote %s: %d cases, %d total reflections, %d bytes" % (path, I.shape[0], int(tir.sum()), os.path.getsize(path)))

    Pm, idx, org, dr = po.soup(300, 2000, 0.2, 5)
    ref = po.RefLib(); ref.add_mesh(Pm, idx); ref.build()
    prim0, st0 = ref.state_batch(org, dr)
    bounces, eo, ed, info = wc.run_chain(ref.state_batch, prim0, st0, refract=lambda i, n, e: tr.reference_refract(lib, i, n, np.broadcast_to(e, (i.shape[0],))))
    hits = np.nonzero(prim0 != po.MISS)[0].astype(np.uint32)
    path = os.path.join(OUT, "whitted_chain.npz")
    np.savez_compressed(path, bounces=bounces, hits=hits, end_org=eo[hits], end_dir=ed[hits], tir=np.int64(info["tir"]), rays=np.array(info["rays"], np.int64))
    print("wrote %s: %s, %d bytes" % (path, info, os.path.getsize(path)))


if __name__ == "__main__":
    main()
