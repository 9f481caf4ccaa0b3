"""The built-in gather sampler (lh_ao_ray_builtin, lucille_amd/csrc/lh_ao.h), restated in numpy from the header's comment, one IEEE operation per
line: the counter, the two 24-bit uniforms, the stratified (z0, z1), cos(theta) and sin(theta) in float32 (numpy's float32 division and square root
are correctly rounded, as the device's are), and the one inexact step -- sinpi / cospi of 2 z1 -- in fp64 from the exact argument.

    local(seed, key, gather_nsamples)      every ray of the keys: the uniforms, (z0, z1), ct, st, the fp64 sinpi / cospi, and the local vector twice --
                                           "ref": the fp64 products (cospi ct, sinpi ct, st), what a device with any sincospif is measured against;
                                           "f32": the float32 vector of a sincospif that rounds the fp64 value once (the host program of
                                           tests/test_ao_sampler_rule.py), bit for bit
    world(h, d)                            the fp64 world direction of local vectors d through 12-double hit records h, in the header's order
    frame_key(px, py, sub, full_width, spp) the key of a frame's sample
    find_edge_keys(seed, gather_nsamples)  the first keys below 2^25 at which the generator sits on one of its four edges

tests/test_ao_sampler_rule.py holds the header, compiled for the host, to this module; tests/test_gpu_ao_sampler.py holds the device to it."""
import functools

import numpy as np

KEY_BITS = 34
KEY_MASK = (1 << KEY_BITS) - 1
GOLD = 0x9E3779B97F4A7C15
U64 = np.uint64
F32 = np.float32
EDGES = ("z0_one", "z1_one", "phi_zero", "r0_zero")
SEARCH_KEYS = 1 << 25


def grid(gather_nsamples):
    """(ntheta, nphi, N): the reference's (int)sqrt(gather_nsamples) strata a side"""
    n = int(np.sqrt(float(gather_nsamples)))
    return n, n, n * n


def mix32(x):
    x = np.asarray(x, U64)
    x = x ^ (x >> U64(33)); x = x * U64(0xff51afd7ed558ccd); x = x ^ (x >> U64(33)); x = x * U64(0xc4ceb9fe1a85ec53); x = x ^ (x >> U64(33))
    return ((x >> U64(16)) & U64(0xFFFFFFFF)).astype(np.uint32)


def counters(seed, key, r, N):
    """k of ray r of key: (seed * GOLD) ^ (((key & mask) * N + r) * 2), everything modulo 2^64; key and r broadcast"""
    with np.errstate(over="ignore"):
        s = (np.array([int(seed) & (2 ** 64 - 1)], U64) * U64(GOLD))[0]
        c = ((np.asarray(key, U64) & U64(KEY_MASK)) * U64(N) + np.asarray(r, U64)) * U64(2)
        return s ^ c


def uniform24(word):
    """the top 24 bits of a 32-bit word times 2^-24, in float32: exact, below 1"""
    return (word >> np.uint32(8)).astype(F32) * F32(5.9604645e-8)


def sincospi(x):
    """(sinpi(x), cospi(x)) in fp64 for x in [0, 2] given exactly: x is reduced modulo 2, n = the nearest multiple of 1/2, f = x - n / 2 in [-1/4, 1/4]
    (both exact), then sin(pi f), cos(pi f) turned by n quarter turns -- so the multiples of 1/2 give exact 0 and +-1"""
    x = np.asarray(x, np.float64)
    x = np.where(x >= 2.0, x - 2.0, x)
    n = np.rint(x * 2.0)
    f = x - n * 0.5
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    q = n.astype(np.int64) & 3
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def local(seed, key, gather_nsamples):
    """every ray of the keys (uint64 [n]) -> dict of [n, N] arrays: k, r0, r1, z0, z1, ct, st (float32), sphi, cphi (fp64), and the local vector [n, N, 3]
    as "ref" (fp64: cphi ct, sphi ct, st) and "f32" (float32: the fp64 sphi, cphi rounded once, then the float32 products)"""
    ntheta, nphi, N = grid(gather_nsamples)
    key = np.atleast_1d(np.asarray(key, U64))
    r = np.arange(N, dtype=np.int64)
    i, j = r % ntheta, r // ntheta
    with np.errstate(over="ignore"):
        k = counters(seed, key[:, None], r[None, :].astype(U64), N)
        r0 = uniform24(mix32(k)); r1 = uniform24(mix32(k + U64(1)))
    z0 = (i.astype(F32)[None, :] + r0) / F32(ntheta)
    z1 = (j.astype(F32)[None, :] + r1) / F32(nphi)
    ct = np.sqrt(z0)
    st = np.sqrt(np.maximum(F32(1.0) - z0, F32(0.0)))
    sphi, cphi = sincospi(F32(2.0) * z1)
    assert r0.dtype == z0.dtype == ct.dtype == st.dtype == F32
    ref = np.stack([cphi * ct.astype(np.float64), sphi * ct.astype(np.float64), st.astype(np.float64)], axis=-1)
    f32 = np.stack([cphi.astype(F32) * ct, sphi.astype(F32) * ct, st], axis=-1)
    return dict(k=k, r0=r0, r1=r1, z0=z0, z1=z1, ct=ct, st=st, sphi=sphi, cphi=cphi, ref=ref, f32=f32, i=i, j=j)


def world(h, d):
    """h [n, 12] hit records (origin, tangent, binormal, Ns), d [n, N, 3] local vectors -> fp64 directions [n, N, 3]: (d0 h[3+k] + d1 h[6+k]) + d2 h[9+k]"""
    h = np.asarray(h, np.float64)[:, None, :]; d = np.asarray(d, np.float64)
    return np.stack([(d[..., 0] * h[..., 3 + k] + d[..., 1] * h[..., 6 + k]) + d[..., 2] * h[..., 9 + k] for k in range(3)], axis=-1)


def frame_key(px, py, sub, full_width, spp):
    """the absolute sample position: pixel (px, py) of a frame full_width wide, sub-sample sub = sy * ps + sx of spp = ps * ps"""
    return (np.asarray(py, U64) * U64(full_width) + np.asarray(px, U64)) * U64(spp) + np.asarray(sub, U64)


def region_keys(x0, w, lines, ps, full_width):
    """the keys of a region's samples in sample order -- line, pixel, sy, sx; lines: the frame line of every line of the region (a tile: y0 .. y0 + h - 1)"""
    spp = ps * ps
    lines = np.asarray(lines, np.int64)
    py = np.repeat(lines, w * spp)
    px = np.tile(np.repeat(x0 + np.arange(w, dtype=np.int64), spp), lines.size)
    sub = np.tile(np.arange(spp, dtype=np.int64), lines.size * w)
    return frame_key(px, py, sub, full_width, spp)


@functools.lru_cache(maxsize=None)
def find_edge_keys(seed, gather_nsamples, limit=SEARCH_KEYS, chunk=1 << 18):
    """-> {edge: (key, r) or None}: for every edge the lowest key below `limit`, and its lowest ray, at which
         z0_one    z0 == 1: the last stratum's (i + r0) / ntheta rounded up (st == 0, the ray lies in the tangent plane);
         z1_one    z1 == 1: the same in phi (phi = 2 pi);
         phi_zero  r1 == 0 in the stratum j = 0 (phi = 0: every component is exact);
         r0_zero   r0 == 0 in the stratum i = 0 (ct == 0: the ray is Ns).
    Only the rays of the stratum in question are drawn, and of their two words the one the edge reads; the search walks the keys in chunks, in order."""
    ntheta, nphi, N = grid(gather_nsamples)
    r_all = np.arange(N, dtype=np.int64)
    i_all, j_all = r_all % ntheta, r_all // ntheta
    want = {"z0_one": (r_all[i_all == ntheta - 1], 0), "z1_one": (r_all[j_all == nphi - 1], 1), "phi_zero": (r_all[j_all == 0], 1),
            "r0_zero": (r_all[i_all == 0], 0)}
    out = {}
    for edge in EDGES:
        rs, word = want[edge]
        out[edge] = None
        for base in range(0, limit, chunk):
            key = np.arange(base, min(base + chunk, limit), dtype=U64)
            with np.errstate(over="ignore"):
                k = counters(seed, key[:, None], rs[None, :].astype(U64), N) + U64(word)
            x = uniform24(mix32(k))
            if edge == "z0_one":
                hit = (i_all[rs].astype(F32)[None, :] + x) / F32(ntheta) == F32(1.0)
            elif edge == "z1_one":
                hit = (j_all[rs].astype(F32)[None, :] + x) / F32(nphi) == F32(1.0)
            else:
                hit = x == F32(0.0)
            if hit.any():
                a, b = np.nonzero(hit)
                out[edge] = (int(key[a[0]]), int(rs[b[0]]))
                break
    return out
