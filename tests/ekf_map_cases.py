"""Cases of the single filter on a pre-loaded map (set_map; reference reflector_ekf_slam.cc:401-425 the match, :279-302 the rows),
shared by tests/test_ekf_map_cpu.py (the cases and the three CPU references against each other, the FP64 floor, the planted
defects) and tests/test_ekf_map_gpu.py (every launch form of the single filter against the longdouble witness with the map
branch, tests/witness/fleet_map_witness.py).

Built with tests/ekf_shape_cases.Builder: a random dense SPD state written with set_state over reflectors on the jittered 2 m
lattice, one non-zero vt, scans 0.1 s apart.  The map's points are free lattice cells (float32-exact, at least 1.6 m from every
reflector and every new point), a map observation lies within 2 mm of its point, the weights are the identity unless stated.  A
case claims three lists per scan, ``expect[k] = (state_pairs, map_pairs, new_ids)``.  Asserted at generation (Builder.scan), no
case excused: both state margins and both map margins (|d1 - 0.05| and d2 - d1 over the weight's scale) of every observation are
>= MARGIN_MIN, and oracle/ekf_numpy.py gives the three lists as claimed.

Map rows are where k_mid is least regular: three pose columns and no landmark block, behind the state pairs in the record, so
that a block step of a wide scan can hold both kinds, and no part in the key of the write-ahead panel (the scan's reflectors).

Four scans, as in the shape sweep (Builder.four_scans): (1) the case's NS state and Mm map pairs; (2) the same reflectors and map
points in another order; (3) another reflector set and other map points, the same counts; (4) part of scan 3's pairs with the
16-row straddler three times and one map point three times (duplicate map rows).

Kinds, (L, NS, Mm):
    mix      a full filter (cap = L): (33, 31, 1), (33, 1, 31), (33, 16, 16); (33, 15, 1) | (33, 16, 1): 32 | 34 rows, the NBR switch;
             (30, 7, 8) and (31, 8, 8): n = 63 | 65; (64, 0, 17): map rows only on a state with landmarks; (127, 24, 8), (127, 0, 32),
             (200, 16, 16).
    pure     n = 3, no reflector, capacity 8: Mm = 1, 16, 17, 32; and one case of two scans that also maps (3 map pairs + 3 new,
             n = 3 -> 9, then those three and two map points).
    growing  cap = L + 8, auto-grow off, scan 1 = NS + Mm + N2 new: (14, 4, 4, N2 = 3), (30, 8, 8, 1), (62, 12, 12, 3): the cross /
             straddle / cross classes of ekf_shape_cases.growing_case with map rows in the same scan.
    wide     L = 128, full, one wide scan, then a scan of 1 state + 1 map: K = 33 = 32 + 1 (the second block step is one map pair
             alone), 40 = 20 + 20 (the first step straddles the state | map boundary of the record), 64 = 0 + 64 (two map-only
             steps on n = 259), 65 = 33 + 32 (staged through HBM, three steps).
    pose     a fix on every scan, the witness in joint form: (33, 7, 7) 31 rows, (33, 7, 8) 33 rows, (64, 15, 15) 63 rows in one
             pass, (64, 1, 30) 65 rows: steps of 30 pairs, the fix on the last.
    weights  (64, 8, 8) twice: rotated anisotropic SPD weights with eigenvalues in [0.25, 4] (map_lip = 2; within 2 mm of the
             point the weighted distance is below 0.006, the next point at least 0.8 away: the weighted margins hold), and the same
             with one weight non-symmetric ([1, 0.5, -0.25, 2]: map_lip < 0, the handle does not speculate).
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from tests import ekf_shape_cases as EC
from tests import fleet_map_cases as MC
from tests.ekf_shape_cases import Builder, _m
from tests.fleet_cases import DIFF, OMNI

# ---- the FP64 noise floor of these cases -------------------------------------------------------------------------------------
# Measured by tests/test_ekf_map_cpu.py::test_fp64_floor (run it with -s) as tests/test_ekf_shapes_cpu.py does for the shape sweep:
# the larger error of oracle/ekf_oracle.c and oracle/ekf_numpy.py against the longdouble witness with the map branch over every
# scan of every case below.  Recorded = measured, rounded up to two digits; the test fails when a re-measurement exceeds it or
# falls below half of it.  The GPU bound is fleet_cases.GPU_FACTOR times these.
FP64_FLOOR_SIGMA = 3.4e-11    # measured 3.380e-11
FP64_FLOOR_MU = 7.2e-16       # measured 7.110e-16
FP64_FLOOR_SIGMA_CASE = "map_grow_L62_S12_M12_N3_diff scan 3 (numpy)"
FP64_FLOOR_MU_CASE = "map_grow_L62_S12_M12_N3_diff scan 3 (numpy)"

witness_of = MC.map_witness_of          # MapWitnessEKF with the case's state and map; a fix goes in jointly
SUITE = NS(name="single_map", floor_sigma=FP64_FLOOR_SIGMA, floor_mu=FP64_FLOOR_MU, witnesses={"witness": witness_of})

MIX_SHAPES = [(33, 31, 1), (33, 1, 31), (33, 16, 16), (33, 15, 1), (33, 16, 1), (30, 7, 8), (31, 8, 8), (64, 0, 17),
              (127, 24, 8), (127, 0, 32), (200, 16, 16)]
PURE_MM = (1, 16, 17, 32)
PURE_CAP = 8
GROWING_SHAPES = [(14, 4, 4, 3), (30, 8, 8, 1), (62, 12, 12, 3)]          # (L, NS, Mm, N2)
WIDE_SHAPES = [(32, 1), (20, 20), (0, 64), (33, 32)]                       # (NS, Mm) on L = 128
WIDE_L = 128
POSE_SHAPES = [(33, 7, 7), (33, 7, 8), (64, 15, 15), (64, 1, 30)]
WEIGHT_SHAPE = (64, 8, 8)
NON_SYMMETRIC = (1.0, 0.5, -0.25, 2.0)


# Seeds: 9600 + the case's number, moved on by 1000 x RESEED[name] where the first draw put an observation nearly equidistant
# (less than MARGIN_MIN apart) from its two nearest map points or reflectors -- Builder.scan asserts every margin of every
# observation, so a case either holds them all or does not exist.
RESEED = {"map_wide_L128_S20_M20_omni": 1, "map_weights_nonsym_L64_S8_M8_omni": 1}


def _seed(base, name):
    return base + 1000 * RESEED.get(name, 0)


def _model(i):
    return DIFF if i % 2 == 0 else OMNI


def mix_case(i, L, n_s, Mm):
    name = f"map_mix_L{L}_S{n_s}_M{Mm}_{_m(_model(i))}"
    b = Builder(L, _model(i), _seed(9600 + i, name), cap=L, n_map=2 * Mm + 1)
    b.four_scans(n_s, Mm=Mm)
    return b.case(name, "mix", K=n_s + Mm, MM=n_s, Mm=Mm, N2=0)


def pure_case(i, Mm):
    name = f"map_pure_M{Mm}_{_m(_model(i))}"
    b = Builder(0, _model(i), _seed(9630 + i, name), cap=PURE_CAP, n_map=2 * Mm + 1)
    b.four_scans(0, Mm=Mm)
    return b.case(name, "pure", K=Mm, MM=0, Mm=Mm, N2=0)


def pure_mapping_case():
    """Pure localisation that also maps: scan 1 matches three map points and appends three reflectors (n = 3 -> 9), scan 2 sees
    those three again and two map points."""
    b = Builder(0, DIFF, _seed(9639, "map_pure_mapping_diff"), cap=PURE_CAP, n_map=5)
    b.scan([], far=3, map_ids=[0, 1, 2])
    b.scan([0, 1, 2], map_ids=[1, 3])
    return b.case("map_pure_mapping_diff", "pure", K=6, MM=0, Mm=3, N2=3)


def growing_case(i, L, n_s, Mm, N2):
    n = 3 + 2 * L
    n16 = (n + 15) & ~15
    cls = {0: "edge", 1: "straddle", 3: "cross"}[N2]
    assert n16 - n == 1 and {"edge": n == n16 - 1, "straddle": n + 2 * N2 == n16 + 1, "cross": n + 2 * N2 > n16 + 1}[cls]
    name = f"map_grow_L{L}_S{n_s}_M{Mm}_N{N2}_{_m(_model(i))}"
    b = Builder(L, _model(i), _seed(9650 + i, name), cap=L + 8, n_map=2 * Mm + 1)
    b.four_scans(n_s, first_new=N2, Mm=Mm)
    return b.case(name, "growing", K=n_s + Mm + N2, MM=n_s, Mm=Mm, N2=N2, n2_class=cls)


def wide_case(i, n_s, Mm):
    L = WIDE_L
    name = f"map_wide_L{L}_S{n_s}_M{Mm}_{_m(_model(i))}"
    b = Builder(L, _model(i), _seed(9670 + i, name), cap=L, n_map=Mm + 2)
    want = EC.musts(L)[:n_s]
    ids = want + [int(j) for j in b.rng.permutation(L) if j not in want][:n_s - len(want)]
    b.scan(ids, map_ids=list(range(Mm)))
    b.scan([EC.triple_of(L)], map_ids=[Mm])
    return b.case(name, "wide", K=n_s + Mm, MM=n_s, Mm=Mm, N2=0)


def pose_case(i, L, n_s, Mm):
    name = f"map_pose_L{L}_S{n_s}_M{Mm}_{_m(_model(i))}"
    b = Builder(L, _model(i), _seed(9680 + i, name), cap=L, n_map=2 * Mm + 1).with_fixes(9690 + i)
    b.four_scans(n_s, Mm=Mm)
    return b.case(name, "pose", K=n_s + Mm, MM=n_s, Mm=Mm, N2=0)


def rotated_weights(count, seed):
    """R diag(l1, l2) R^T with l1, l2 in [0.25, 4]: exactly symmetric (the off-diagonal element is computed once)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, 4))
    for j in range(count):
        a = rng.uniform(0.0, math.pi)
        l1, l2 = 2.0 ** rng.uniform(-2.0, 2.0, size=2)
        c, s = math.cos(a), math.sin(a)
        off = (l1 - l2) * c * s
        out[j] = (l1 * c * c + l2 * s * s, off, off, l1 * s * s + l2 * c * c)
    out[0] = (4.0, 0.0, 0.0, 0.25)                                  # (both ends of the range are met)
    return out


def weights_case(i, non_symmetric):
    L, n_s, Mm = WEIGHT_SHAPE
    cov = rotated_weights(2 * Mm + 1, 9700)
    if non_symmetric:
        cov[Mm] = NON_SYMMETRIC                                     # (the point scan 4 observes three times)
    name = f"map_weights_{'nonsym' if non_symmetric else 'spd'}_L{L}_S{n_s}_M{Mm}_{_m(_model(i))}"
    b = Builder(L, _model(i), _seed(9700 + i, name), cap=L, n_map=2 * Mm + 1, map_cov=cov)
    b.four_scans(n_s, Mm=Mm)
    return b.case(name, "weights", K=n_s + Mm, MM=n_s, Mm=Mm, N2=0, non_symmetric=non_symmetric)


_cases = None


def cases():
    """Every case of this module, by kind: mix, pure, growing, wide, pose, weights."""
    global _cases
    if _cases is None:
        _cases = ([mix_case(i, *s) for i, s in enumerate(MIX_SHAPES)] + [pure_case(i, Mm) for i, Mm in enumerate(PURE_MM)] +
                  [pure_mapping_case()] + [growing_case(i, *s) for i, s in enumerate(GROWING_SHAPES)] +
                  [wide_case(i, *s) for i, s in enumerate(WIDE_SHAPES)] + [pose_case(i, *s) for i, s in enumerate(POSE_SHAPES)] +
                  [weights_case(0, False), weights_case(1, True)])
    return _cases


def case_named(name):
    return next(c for c in cases() if c.name == name)


def rows_of(case, k):
    """Innovation rows of scan k: two per pair and three of a fix."""
    sp, mp, _ = EC.claim3(case, k)
    ev = case.events[k]
    return 2 * (len(sp) + len(mp)) + (3 if len(ev) > 4 and ev[4] is not None else 0)


def block_steps(case, k):
    """How the host cuts scan k: None for a whole scan (at most 64 rows), else per block step (state pairs, map pairs) in the order
    of the record -- the state pairs first, then the map pairs, in steps of 32 pairs (30 with a fix)."""
    sp, mp, _ = EC.claim3(case, k)
    ev = case.events[k]
    fix = len(ev) > 4 and ev[4] is not None
    if 2 * len(ev[3]) + (3 if fix else 0) <= 64:
        return None
    stride, kinds = (30 if fix else 32), [1] * len(sp) + [0] * len(mp)
    return [(sum(kinds[p:p + stride]), len(kinds[p:p + stride]) - sum(kinds[p:p + stride])) for p in range(0, len(ev[3]), stride)]
