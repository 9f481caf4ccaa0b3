"""Generate tests/golden/sky_reference.npz by running the COMPILED REFERENCE (oracle/_ref/liblucille_ref.so, built from the reference
tree by oracle/Makefile) through ctypes.  The fixture is data; no reference source is stored.

Four skies (latitude, longitude, standard meridian, day, time of day, turbidity; the first is the reference's default site).  Per sky:

  site           the six numbers above (float64)
  sky            what ri_sunsky_init left in the struct, in the order of lh_sky_t's first 20 floats: sun_theta, sun_phi, perez_x[5],
                 perez_y[5], perez_Y[5], zenith_x, zenith_y, zenith_Y
  sun_dir        the struct's sun_dir[3] (float32, the reference's own axes: the light's direction swaps y and z)
  basis_rgb/_y   the twelve basis floats: S0 / S1 / S2Amplitudes through spectrum_to_xyz and xyz_to_rgb (the CIE system of sunsky.c)
  sun_rgb        ri_sunsky_get_sunlight_rgb AFTER the struct's `turbidity` was set to the site's: ri_sunsky_init never stores it, the
                 reference reads whatever the allocation held
  dirs           2 000 seeded float32 unit directions over the whole sphere, then the specials: the zenith, the sun's own direction,
                 v[1] = 0, -0.0, 0.0005, 0.000999, 0.001 (two azimuths each) and five directions below the horizon
  rgb            ri_sunsky_get_sky_rgb of each

    python tests/golden/make_sky_golden.py
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
REFLIB = os.path.join(ROOT, "oracle", "_ref", "liblucille_ref.so")

SITES = [(35.39, 139.44, 9.0, 20, 10.5, 2.0), (35.39, 139.44, 9.0, 180, 16.5, 5.0), (60.0, 10.0, 1.0, 355, 12.0, 3.0), (0.0, 0.0, 0.0, 80, 6.5, 8.0)]
NDIRS = 2000


class Sunsky(C.Structure):          # ri_sunsky_t
    _fields_ = [("sun_theta", C.c_float), ("sun_phi", C.c_float), ("sun_dir", C.c_float * 3), ("turbidity", C.c_float), ("V", C.c_float),
                ("sun_spectrum", C.c_void_p), ("sun_rgb", C.c_float * 3), ("perez_x", C.c_float * 5), ("perez_y", C.c_float * 5),
                ("perez_Y", C.c_float * 5), ("zenith_x", C.c_float), ("zenith_y", C.c_float), ("zenith_Y", C.c_float)]


class ColourSystem(C.Structure):    # struct colourSystem
    _fields_ = [("name", C.c_char_p)] + [(n, C.c_float) for n in ("xRed", "yRed", "xGreen", "yGreen", "xBlue", "yBlue", "xWhite", "yWhite", "gamma")]


def cie_system():
    """the CIE primaries and the equal-energy white point, the colour system sunsky.c converts with"""
    return ColourSystem(b"CIE", 0.7355, 0.2645, 0.2658, 0.7243, 0.1669, 0.0085, 0.33333333, 0.33333333, 0.0)


def directions(k, sun_world):
    rng = np.random.default_rng(1000 + k)
    d = rng.standard_normal((NDIRS, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    sp = [(0.0, 1.0, 0.0), tuple(sun_world)]
    for y in (0.0, -0.0, 0.0005, 0.000999, 0.001):
        for az in (0.3, 4.0):
            h = np.sqrt(1.0 - y * y)
            sp.append((h * np.cos(az), y, h * np.sin(az)))
    sp += [(0.0, -1.0, 0.0), (0.6, -0.8, 0.0), (0.0, -1e-6, 1.0), (-0.7071, -0.001, 0.7071), (0.5, -0.5, -0.7071)]
    return np.concatenate([d, np.array(sp, np.float32)])


def main():
    lib = C.CDLL(REFLIB)
    lib.ri_sunsky_new.restype = C.POINTER(Sunsky)
    lib.ri_sunsky_init.argtypes = [C.POINTER(Sunsky), C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_int]
    lib.ri_sunsky_init.restype = None
    fp = C.POINTER(C.c_float)
    lib.ri_sunsky_get_sky_rgb.argtypes = [fp, C.POINTER(Sunsky), fp]; lib.ri_sunsky_get_sky_rgb.restype = None
    lib.ri_sunsky_get_sunlight_rgb.argtypes = [fp, C.POINTER(Sunsky)]; lib.ri_sunsky_get_sunlight_rgb.restype = None
    lib.spectrum_to_xyz.argtypes = [fp, fp, fp, fp]; lib.spectrum_to_xyz.restype = None
    lib.xyz_to_rgb.argtypes = [C.POINTER(ColourSystem), C.c_float, C.c_float, C.c_float, fp, fp, fp]; lib.xyz_to_rgb.restype = None
    cs = cie_system()
    basis_rgb = np.zeros((3, 3), np.float32); basis_y = np.zeros(3, np.float32)
    for j, name in enumerate(("S0Amplitudes", "S1Amplitudes", "S2Amplitudes")):
        amp = (C.c_float * 41).in_dll(lib, name)
        x, y, z, r, g, b = (C.c_float() for _ in range(6))
        lib.spectrum_to_xyz(amp, C.byref(x), C.byref(y), C.byref(z))
        lib.xyz_to_rgb(C.byref(cs), x, y, z, C.byref(r), C.byref(g), C.byref(b))
        basis_rgb[j] = (r.value, g.value, b.value); basis_y[j] = y.value
    out = {"basis_rgb": basis_rgb, "basis_y": basis_y}
    for k, site in enumerate(SITES):
        s = lib.ri_sunsky_new()
        lib.ri_sunsky_init(s, site[0], site[1], site[2], site[3], site[4], site[5], 0)
        c = s.contents
        sky = np.array([c.sun_theta, c.sun_phi] + list(c.perez_x) + list(c.perez_y) + list(c.perez_Y) + [c.zenith_x, c.zenith_y, c.zenith_Y], np.float32)
        sun_dir = np.array(list(c.sun_dir), np.float32)
        c.turbidity = site[5]
        sun_rgb = np.zeros(3, np.float32)
        lib.ri_sunsky_get_sunlight_rgb(sun_rgb.ctypes.data_as(fp), s)
        d = directions(k, (sun_dir[0], sun_dir[2], sun_dir[1]))
        rgb = np.zeros_like(d)
        for i in range(d.shape[0]):
            lib.ri_sunsky_get_sky_rgb(rgb[i].ctypes.data_as(fp), s, d[i].ctypes.data_as(fp))
        out.update({"site%d" % k: np.array(site, np.float64), "sky%d" % k: sky, "sun_dir%d" % k: sun_dir, "sun_rgb%d" % k: sun_rgb,
                    "dirs%d" % k: d, "rgb%d" % k: rgb})
    path = os.path.join(OUT, "sky_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d skies, %d directions each, %d bytes" % (path, len(SITES), d.shape[0], os.path.getsize(path)))


if __name__ == "__main__":
    main()
