"""Rays whose direction holds zero components of either sign, aimed at triangles of a scene: the reference takes the order of a box's planes and the
sign of its +-DBL_MAX inverse from the same comparison dir < 0 (bvh.c:473-497), so a -0.0 is a +0.0 to it; lh_ray_setup (lh_filter.h) has to keep
its ng flags and its clamped inverse in the same agreement.  Shared by tests/test_signed_zero_model.py (the host model and the host walk) and
tests/test_gpu_signed_zero.py (the device)."""
import numpy as np

from oracle import pyoracle as po


def scenes():
    """name -> (positions, indices): a soup deep enough for inner nodes, and one triangle (the root is a leaf)"""
    P, idx, _, _ = po.soup(3000, 1, 0.05, 11)
    one = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    return {"soup": (P, idx), "one triangle": (one, np.arange(3, dtype=np.uint32))}


def rays(P, idx, seed=3, per_kind=96):
    """-> (org, dir, minus [n]: the ray has a -0.0 component).  Every ray is aimed at the centroid of a triangle, from inside the scene's box where
    the scene has one: along an axis (two zero components, the four sign pairs), and in an axis plane (one zero component, both signs)"""
    rng = np.random.default_rng(seed)
    T = P[idx].reshape(-1, 3, 3)
    org, dr = [], []
    for axis in range(3):
        for s in (1.0, -1.0):
            for za in (0.0, -0.0):
                for zb in (0.0, -0.0):
                    c = T[rng.integers(0, T.shape[0], per_kind)].mean(axis=1)
                    d = np.empty((per_kind, 3)); d[:, axis] = s; d[:, (axis + 1) % 3] = za; d[:, (axis + 2) % 3] = zb
                    o = c.copy(); o[:, axis] -= s * rng.uniform(0.01, 0.3, per_kind)
                    org.append(o); dr.append(d)
        for z in (0.0, -0.0):
            c = T[rng.integers(0, T.shape[0], per_kind)].mean(axis=1)
            d = rng.standard_normal((per_kind, 3)); d[:, axis] = z
            o = c - d * rng.uniform(0.01, 0.3, (per_kind, 1))
            o[:, axis] = c[:, axis]          # (x - 0 * s is x: the ray stays in the centroid's plane exactly)
            org.append(o); dr.append(d)
    org, dr = np.concatenate(org), np.concatenate(dr)
    return org, dr, ((dr == 0.0) & np.signbit(dr)).any(axis=1)
