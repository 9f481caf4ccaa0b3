"""Rays for the tests of the bin order of ray dumps (lucille_amd/csrc/lh_order.h): tests/test_order_key.py (the key, the run table and the
destinations against numpy) and tests/test_gpu_dump_order.py (records of an ordered dump == records of the dump as given)."""
import numpy as np


def edge_rays(n, lo, hi, seed, legal_only):
    """n rays around the box lo .. hi whose keys are decided at the edges of the rule: -0.0 / +0.0 and denormal direction components, origins on
    the bounds and on the cell planes, just outside, far outside; and, unless legal_only (rays a walk may be given), NaN and infinite
    coordinates.  Every direction keeps a component of ordinary size."""
    rng = np.random.default_rng(seed)
    lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64); ext = hi - lo
    org = lo + rng.uniform(0.0, 1.0, (n, 3)) * ext
    dr = rng.normal(size=(n, 3)); dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    k = np.arange(n)
    ax = rng.integers(0, 3, n)                # the component a special value goes to
    keep = (ax + 1) % 3                       # ... and one that stays ordinary
    def put(a, sel, values):
        a[k[sel], ax[sel]] = values
    m = k % 16
    put(dr, m == 0, -0.0); put(dr, m == 1, 0.0)
    put(dr, m == 2, 5e-324); put(dr, m == 3, -5e-324); put(dr, m == 4, 2.2e-308); put(dr, m == 5, -1e-310)
    put(org, m == 6, lo[ax[m == 6]]); put(org, m == 7, hi[ax[m == 7]])                                   # on the bounds
    put(org, m == 8, (lo + ext * rng.integers(1, 4, (n, 1)) / 4.0)[k[m == 8], ax[m == 8]])               # on the cell planes of 1 and 2 bits
    put(org, m == 9, np.nextafter(lo, -np.inf)[ax[m == 9]]); put(org, m == 10, np.nextafter(hi, np.inf)[ax[m == 10]])
    put(org, m == 11, (lo - 3.0 * ext)[ax[m == 11]]); put(org, m == 12, (hi + 1e6 * ext)[ax[m == 12]])
    big = 100.0 * ext.max() if legal_only else 1e300
    put(org, m == 13, -big); put(org, m == 14, big)
    if not legal_only:
        s = (k % 64) == 15
        put(org, s, np.nan)
        s = (k % 64) == 31
        put(org, s, np.inf)
        s = (k % 64) == 47
        put(org, s, -np.inf)
        s = (k % 64) == 63
        put(dr, s, np.where(k[s] % 128 < 64, np.nan, -np.nan))
        s = (k % 128) == 79
        put(dr, s, np.inf)
        s = (k % 128) == 111
        put(dr, s, -np.inf)
    dr[k, keep] = np.where(np.abs(dr[k, keep]) < 0.05, 0.5, dr[k, keep])
    return np.ascontiguousarray(org), np.ascontiguousarray(dr)


def one_bin_rays(n, lo, hi, seed):
    """rays of one key at every number of cell bits: origins in the lowest eighth of the box per axis (one cell even at three bits), directions in the all-positive octant"""
    rng = np.random.default_rng(seed)
    lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64)
    org = lo + rng.uniform(0.01, 0.12, (n, 3)) * (hi - lo)
    dr = rng.uniform(0.1, 1.0, (n, 3)); dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    return org, dr
