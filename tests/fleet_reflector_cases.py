"""Cases of rfleet_get_reflectors (k_fleet_reflectors): states given with ``set_state`` whose 2 x 2 reflector blocks take every
branch of the marker ellipses' eigen-solve, in two fleets whose members sit on the kernel's edges, and one short real session.

Fleet A: max_landmarks = 128 (ld = 272), reflector counts 0, 1, 63, 64, 65, 128, 0, 2 -- an empty member first and in the middle,
the wave edge, full capacity.  Fleet B: max_landmarks = 5 (n_max = 13, ld = 16), counts 5, 0, 3.

A member's sigma, as handed to set_state, is full and NOT symmetric: every entry outside the reflector blocks is a non-zero random
number (a wrong index or a wrong ld reads one of them), and each block's upper entry differs from its lower one (a read of the
wrong triangle shows).  What the fleet is held to is the lower triangle, mirrored (``mirrored``): what get_state returns."""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

EPS = 2.220446049250313e-16
COUNTS_A, ML_A = (0, 1, 63, 64, 65, 128, 0, 2), 128
COUNTS_B, ML_B = (5, 0, 3), 5
KINDS = ("spd", "a_gt_d", "a_lt_d", "a_eq_d", "c_zero", "c_below", "c_above", "zero", "negative", "pz_zero")
SPD_KINDS = ("spd", "a_gt_d", "a_lt_d", "a_eq_d", "c_zero")          # positive definite: the ellipse they draw is the block itself
UPPER_SHIFT = 0.25            # sigma(id, id+1) as given = sigma(id+1, id) + this: never what the fleet may return
SESSION_SCANS = 20
SESSION_SEEDS = (4100, 4101)


def block_of(kind, rng):
    """-> (a, c, d) of one reflector's block [[a, c], [c, d]]."""
    s = float(rng.uniform(0.5, 2.0))
    if kind == "spd":
        th, l0, l1 = rng.uniform(-math.pi, math.pi), rng.uniform(0.01, 1.0), rng.uniform(0.01, 1.0)
        co, si = math.cos(th), math.sin(th)
        return co * co * l0 + si * si * l1, co * si * (l0 - l1), si * si * l0 + co * co * l1
    if kind == "a_gt_d":
        return 0.04 * s, 0.012 * s, 0.01 * s
    if kind == "a_lt_d":
        return 0.01 * s, -0.02 * s, 0.09 * s
    if kind == "a_eq_d":                                   # p = 0
        return 0.02 * s, 0.005 * s, 0.02 * s
    if kind == "c_zero":
        return 0.03 * s, 0.0, 0.05 * s
    if kind in ("c_below", "c_above"):                     # the negligible-sub-diagonal test, one ulp either side of its threshold
        a, d = 2.0 * s, 1.0 * s
        thr = EPS * (abs(a) + abs(d))
        c = np.nextafter(thr, 0.0) if kind == "c_below" else np.nextafter(thr, np.inf)
        return a, float(c) * (1.0 if rng.uniform() < 0.5 else -1.0), d
    if kind == "zero":
        return 0.0, 0.0, 0.0
    if kind == "negative":                                 # eigenvalues 3 s and -s: one length is sqrt of a negative number
        return 1.0 * s, 2.0 * s, 1.0 * s
    if kind == "pz_zero":                                  # c c underflows: p = 0, z = 0, pz = 0 -- the guard's branch (d1 = d0)
        return 0.0, 1e-200, 0.0
    raise KeyError(kind)


def branch_of(a, c, d):
    """Which way the 2 x 2 solve goes for [[a, c], [c, d]] (ekf_kernels.hip k_ellipses, oracle/ekf_oracle.c oekf_marker_ellipses)."""
    if abs(c) <= EPS * (abs(a) + abs(d)):
        return "negligible"
    p = 0.5 * (a - d)
    z = math.sqrt(abs(p * p + c * c))
    pz = p + z if p >= 0.0 else p - z
    if pz == 0.0:
        return "pz_zero"
    return "p_positive" if p > 0.0 else ("p_zero" if p == 0.0 else "p_negative")


def mirrored(sigma):
    """The symmetric matrix of sigma's lower triangle: what set_state keeps and get_state returns."""
    lo = np.tril(sigma)
    return lo + np.tril(sigma, -1).T


def member(L, seed, shift=0):
    """One member's state: -> NS(L, t, mu, sigma (as given: not symmetric), kinds, blocks [L, 3] = (a, c, d))."""
    rng = np.random.default_rng(seed)
    n = 3 + 2 * L
    mu = rng.uniform(-20.0, 20.0, size=n)
    sigma = rng.uniform(1e-4, 2e-3, size=(n, n)) * rng.choice([-1.0, 1.0], size=(n, n))
    kinds, blocks = [], np.zeros((L, 3))
    for i in range(L):
        kind = KINDS[(i + shift) % len(KINDS)]
        a, c, d = block_of(kind, rng)
        j = 3 + 2 * i
        sigma[j, j], sigma[j + 1, j], sigma[j + 1, j + 1] = a, c, d
        sigma[j, j + 1] = c + UPPER_SHIFT
        kinds.append(kind)
        blocks[i] = a, c, d
    return NS(L=L, t=1.5 + 0.25 * (seed % 7), mu=mu, sigma=sigma, kinds=kinds, blocks=blocks)


def fleet_a():
    return [member(L, 900 + k, shift=3 * k) for k, L in enumerate(COUNTS_A)]


def fleet_b():
    return [member(L, 950 + k, shift=4 * k) for k, L in enumerate(COUNTS_B)]


def expected_landmarks(m):
    """-> (xy [L, 2], cov [L, 2, 2]) of a member as get_state's means and blocks hold them."""
    S = mirrored(m.sigma)
    xy = m.mu[3:].reshape(-1, 2).copy()
    cov = np.stack([S[3 + 2 * i: 5 + 2 * i, 3 + 2 * i: 5 + 2 * i] for i in range(m.L)]) if m.L else np.zeros((0, 2, 2))
    return xy, cov


def same_bits(a, b):
    """Equal as bits, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool((both_nan | (a.view(np.uint64) == b.view(np.uint64))).all())


def ellipse_error(rows, blocks):
    """The largest |R diag R^T - block| over a block's largest entry: rows [K, 5] marker ellipses, blocks [K, 3] = (a, c, d)."""
    from tests.helpers import ellipse_matrices
    M = ellipse_matrices(rows)
    B = np.stack([np.array([[a, c], [c, d]]) for a, c, d in blocks])
    return float((np.abs(M - B).max(axis=(1, 2)) / np.abs(B).max(axis=(1, 2))).max())


def spd_rows(m):
    return np.array([k in SPD_KINDS for k in m.kinds], bool)


def oracle_rows(m):
    """oracle/ekf_oracle.c's marker ellipses of the member's state (its own full, mirrored matrix)."""
    from oracle.binding import OracleEKF
    o = OracleEKF(0, 0.0, (0.0, 0.0, 0.0), 0.0025, 0.0064, 0.0025)
    o.set_state(m.t, m.mu, mirrored(m.sigma))
    rows = o.marker_ellipses()
    o.close()
    return rows if m.L else rows[:0]


def sessions():
    """Two short real sessions (a world of 24 reflectors, about 20 scans): blocks made by augmentation and update."""
    from reflector_ekf_slam_amd import synth
    return [synth.make_session(synth.SessionConfig(f"refl_{seed}", 24, 8, synth.DIFF if k == 0 else synth.OMNI, seed=seed, speed=1.0,
                                                   row_spacing=6.0), max_scans=SESSION_SCANS + 1) for k, seed in enumerate(SESSION_SEEDS)]
