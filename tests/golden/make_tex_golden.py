"""Generate tests/golden/tex_fetch.npz by running the COMPILED REFERENCE's ri_texture_fetch (oracle/_ref/liblucille_ref.so, built
from the reference tree by oracle/Makefile) on hand-filled ri_texture_t records, through ctypes.  The fixture is data: the texels and
(s, t) pairs of tests/test_tex_rule.py's cases (by seed) and the four doubles the reference returned for each; no reference source
is stored.

    python tests/golden/make_tex_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_tex_rule as tr  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    lib = C.CDLL(tr.REFLIB)
    cs = tr.cases()
    z = {"ntex": np.int32(len(cs))}
    for k, (tex, st) in enumerate(cs):
        z["tex%d" % k] = tex; z["st%d" % k] = st; z["out%d" % k] = tr.reference_fetch(lib, tex, st)
    path = os.path.join(OUT, "tex_fetch.npz")
    np.savez_compressed(path, **z)
    print("wrote %s: %d textures, %d fetches, %d bytes" % (path, len(cs), sum(c[1].shape[0] for c in cs), os.path.getsize(path)))


if __name__ == "__main__":
    main()
