"""Per-element Lame parameter fields for the tests (dotmi_mesh::mu / ::lambda are nT arrays, include/dotmi.h).

Every field is a pure function of (scene, kind, seed), so that a subprocess can rebuild it from its name instead of receiving
arrays.  The scene's own YM / PR are the base material.

kinds:
  random         YM log-uniform over [YM / 30, 30 YM] and PR uniform in [0.2, 0.45], independently per element
  stripes        the reference's commented-out set-up (Mesh.cpp:746-764): 8 segments along x by element centroid, the even
                 segments stiffer with PR 0.49.  The contrast is YM x 100, not the reference's x 1000: at x 1000 the
                 oracle's third step on synbar:16x5x5 runs into the iteration cap (10000 iterations, status 2); at x 100
                 every step converges in a handful of iterations
  one-off        one material except the LAST element (YM x 10, PR 0.3)
  one-off-first  one material except element 0 (YM x 10, PR 0.3)
  lam-only       one mu, lambda per element (PR uniform in [0.2, 0.45] at that mu)
"""
from __future__ import annotations

import numpy as np

from dot_amd.scene import lame

KINDS = ("random", "stripes", "one-off", "one-off-first", "lam-only")


def _lame_arrays(YM, PR):
    YM, PR = np.asarray(YM, dtype=np.float64), np.asarray(PR, dtype=np.float64)
    return YM / 2.0 / (1.0 + PR), YM * PR / (1.0 + PR) / (1.0 - 2.0 * PR)


def field(scene, kind: str, seed: int = 0):
    """-> (mu, lam), float64 arrays of shape (nT,)"""
    YM, PR = scene.cfg.YM, scene.cfg.PR
    nT = scene.T.shape[0]
    rng = np.random.default_rng(seed)
    mu0, lam0 = lame(YM, PR)
    if kind == "random":
        ym = YM * np.exp(rng.uniform(np.log(1.0 / 30.0), np.log(30.0), nT))
        pr = rng.uniform(0.2, 0.45, nT)
        return _lame_arrays(ym, pr)
    if kind == "stripes":
        nseg = 8
        X = scene.V_rest[:, 0]
        xmin = X.min()
        seglen = (X.max() - xmin) / nseg
        center = X[scene.T].mean(axis=1)
        seg = np.clip(((center - xmin) / seglen).astype(int), 0, nseg - 1)
        mu_s, lam_s = lame(YM * 100.0, 0.49)
        stiff = seg % 2 == 0
        return np.where(stiff, mu_s, mu0), np.where(stiff, lam_s, lam0)
    if kind in ("one-off", "one-off-first"):
        mu, lam = np.full(nT, mu0), np.full(nT, lam0)
        e = nT - 1 if kind == "one-off" else 0
        mu[e], lam[e] = lame(YM * 10.0, 0.3)
        return mu, lam
    if kind == "lam-only":
        pr = rng.uniform(0.2, 0.45, nT)
        return np.full(nT, mu0), mu0 * 2.0 * pr / (1.0 - 2.0 * pr)
    raise ValueError(f"unknown material field {kind!r}; one of {KINDS}")
