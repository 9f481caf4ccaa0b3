"""Generate tests/golden/area_sample.npz by running the COMPILED REFERENCE (oracle/_ref/liblucille_ref.so, built from the reference tree by
oracle/Makefile) through ctypes.  The fixture is data; no reference source is stored.

Four emitters -- one triangle, a quad of two, a mesh of twenty, three triangles of which the middle one has no area -- each built as an ri_geom_t with
the reference's own constructors (ri_geom_new, ri_geom_add_positions, ri_geom_add_indices) and attached to an ri_light_t (ri_light_new,
ri_light_attach_geom).  Per emitter k:

  tris{k}   the triangles, float64 [ntris, 3, 3]
  seed{k}   the seed handed to seedMT
  uni{k}    the three randomMT() numbers every call consumed, float64 [N, 3]: the same stream drawn again after seeding once more
  pos{k}    what ri_light_sample_pos_and_normal wrote into pos, float64 [N, 3]
  nrm{k}    ... and into normal

    python tests/golden/make_area_golden.py
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
REFLIB = os.path.join(ROOT, "oracle", "_ref", "liblucille_ref.so")
NCALLS = 300


def emitters():
    rng = np.random.default_rng(20240)
    one = np.array([[[-0.31, 2.13, -0.27], [0.44, 2.21, -0.19], [0.07, 2.05, 0.52]]])
    quad = np.array([[[0.1, 0.45, 0.1], [0.35, 0.47, 0.12], [0.33, 0.44, 0.37]], [[0.1, 0.45, 0.1], [0.33, 0.44, 0.37], [0.08, 0.42, 0.35]]])
    c = np.array([1.7, 1.3, -1.9])
    mesh = c + 0.3 * rng.standard_normal((20, 3, 3))
    flat = np.array([[[0.0, 3.0, 0.0], [1.0, 3.1, 0.0], [0.0, 3.2, 1.0]],
                     [[0.5, 3.0, 0.5], [0.5, 3.0, 0.5], [0.9, 3.3, 0.1]],          # two equal vertices: no area, the normalise guard's else branch
                     [[1.0, 3.0, 1.0], [2.0, 3.3, 1.0], [1.0, 3.1, 2.0]]])
    return [one, quad, mesh, flat]


def main():
    lib = C.CDLL(REFLIB)
    lib.lref_init()
    lib.RiBegin.argtypes = [C.c_char_p]; lib.RiBegin(None)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    lib.ri_geom_new.restype = vp
    lib.ri_geom_add_positions.argtypes = [vp, C.c_uint, vp]; lib.ri_geom_add_positions.restype = None
    lib.ri_geom_add_indices.argtypes = [vp, C.c_uint, vp]; lib.ri_geom_add_indices.restype = None
    lib.ri_light_new.restype = vp
    lib.ri_light_attach_geom.argtypes = [vp, vp]; lib.ri_light_attach_geom.restype = None
    lib.ri_light_sample_pos_and_normal.argtypes = [dp, dp, vp]; lib.ri_light_sample_pos_and_normal.restype = None
    lib.seedMT.argtypes = [C.c_uint]; lib.seedMT.restype = None
    lib.randomMT.restype = C.c_double
    out = {}
    for k, tris in enumerate(emitters()):
        nt = tris.shape[0]
        P = np.zeros((3 * nt, 4)); P[:, :3] = tris.reshape(-1, 3)          # ri_vector_t: four doubles
        I = np.arange(3 * nt, dtype=np.uint32)
        g = lib.ri_geom_new()
        lib.ri_geom_add_positions(g, 3 * nt, P.ctypes.data)
        lib.ri_geom_add_indices(g, 3 * nt, I.ctypes.data)
        light = lib.ri_light_new()
        lib.ri_light_attach_geom(light, g)
        seed = 4357 + 11 * k
        pos = np.zeros((NCALLS, 4)); nrm = np.zeros((NCALLS, 4))
        lib.seedMT(seed)
        for i in range(NCALLS):
            lib.ri_light_sample_pos_and_normal(pos[i].ctypes.data_as(dp), nrm[i].ctypes.data_as(dp), light)
        lib.seedMT(seed)
        uni = np.array([[lib.randomMT() for _ in range(3)] for _ in range(NCALLS)])
        out.update({"tris%d" % k: tris, "seed%d" % k: np.array(seed, np.uint32), "uni%d" % k: uni, "pos%d" % k: pos[:, :3].copy(), "nrm%d" % k: nrm[:, :3].copy()})
    path = os.path.join(OUT, "area_sample.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d emitters, %d calls each, %d bytes" % (path, k + 1, NCALLS, os.path.getsize(path)))


if __name__ == "__main__":
    main()
