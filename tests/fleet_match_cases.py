"""Cases of the fleet scan matcher (rgrid_batch_* of include/rgrid.h, reflector_ekf_slam_amd/fleet_match.py), shared by
tests/test_fleet_match_cpu.py and tests/test_fleet_match_gpu.py.  Built on tests/grid_cases.py: the room grid at 0.05 m
(480 x 480 cells, with update-marker cells) and at 0.1 m (200 x 200), and scans of its occupied points.

A scan here is ``(grid_slot, initial_pose, points_xy)`` as ``ScanMatchFleet.submit`` takes it; slot 0 is the 0.05 m grid, slot 1
the 0.1 m grid.
"""
from __future__ import annotations

import math

import numpy as np

from tests.grid_cases import room_grid, scan_of

# against the oracle: tests/test_grid_gpu.py::test_match_identical_candidate_and_score
SCORE_RTOL, POSE_TOL = 1.2e-7, 1e-12

_grids = None


def grids():
    """[(cells, resolution, max_xy, occupied points)]: slot 0 = 0.05 m, slot 1 = 0.1 m (the grids of tests/test_grid_gpu.py)."""
    global _grids
    if _grids is None:
        c0, m0, o0 = room_grid()
        c1, m1, o1 = room_grid(resolution=0.1, half=10.0)
        _grids = [(c0, 0.05, m0, o0), (c1, 0.1, m1, o1)]
    return _grids


def single_matcher_cases():
    """The four parametrised cases of test_match_identical_candidate_and_score (default options, 0.05 m grid) -> (scans, true poses)."""
    occ = grids()[0][3]
    scans, trues = [], []
    for true, dinit, npts in (((0.8, -0.6, 0.35), (0.10, -0.15, 4.0), 700), ((-2.0, 1.2, -1.9), (-0.12, 0.08, -7.0), 500),
                              ((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 300), ((3.1, 2.2, 0.9), (0.19, 0.19, 14.0), 900)):
        true = np.array(true)
        pts = scan_of(occ, true, n_points=npts, seed=int(10 * abs(true[0]) + npts))
        scans.append((0, true + np.array([dinit[0], dinit[1], math.radians(dinit[2])]), pts))
        trues.append(true)
    return scans, trues


def options_case():
    """The options case of test_match_options_windows_and_errors (0.1 m grid) -> (scan, option values)."""
    occ = grids()[1][3]
    true = np.array([1.0, 1.0, 0.2])
    pts = scan_of(occ, true, n_points=400)
    return (1, true + [0.2, -0.1, 0.03], pts), (0.35, math.radians(6.0), 2.0, 5.0)


def shape_scans():
    """Point counts on both sides of the point block of 16, on both grids (so num_linear and the rotation count differ within
    the call), a scan partly outside its grid, two wholly outside."""
    scans = []
    for k, n in enumerate((1, 15, 16, 17, 33, 300, 900)):
        slot = k % 2
        occ = grids()[slot][3]
        true = np.array([0.5 - 0.3 * k, 0.2 * k - 0.4, 0.4 * k - 1.0])
        pts = scan_of(occ, true, n_points=n, seed=100 + k)
        assert pts.shape[0] == n
        scans.append((slot, true + np.array([0.06, -0.04, math.radians(3.0)]), pts))
    # partly outside: seen from a pose the initial estimate puts 4 m further out, the far wall falls off the 12 m grid
    occ = grids()[0][3]
    true = np.array([5.0, 1.0, 0.3])
    pts = scan_of(occ, true, n_points=200, seed=120)
    scans.append((0, true + np.array([4.0, 0.0, 0.0]), pts))
    # wholly outside: every lookup is kMinProbability
    far = np.array([[30.0, 30.0], [31.0, 29.0]], np.float32)
    scans.append((0, np.zeros(3), far))
    scans.append((1, np.zeros(3), far))
    return scans


def partly_outside_fraction(scan):
    """Fraction of the scan's points that the initial pose puts outside its grid (for the case's own sanity check)."""
    slot, pose, pts = scan
    cells, res, max_xy, _ = grids()[slot]
    c, s = math.cos(pose[2]), math.sin(pose[2])
    wx, wy = pose[0] + c * pts[:, 0] - s * pts[:, 1], pose[1] + s * pts[:, 0] + c * pts[:, 1]
    ix, iy = np.rint((max_xy[1] - wy) / res - 0.5), np.rint((max_xy[0] - wx) / res - 0.5)
    out = (ix < 0) | (iy < 0) | (ix >= cells.shape[1]) | (iy >= cells.shape[0])
    return float(out.mean())


def tile_scans(count=12, n=64):
    """`count` distinct scans of n points against the 0.05 m grid."""
    occ = grids()[0][3]
    rng = np.random.default_rng(77)
    scans = []
    for k in range(count):
        true = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(-3, 3)])
        pts = scan_of(occ, true, n_points=n, seed=200 + k)
        scans.append((0, true + np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), math.radians(rng.uniform(-5, 5))]), pts))
    return scans


def oracle_of(scan, option_values=None):
    """oracle.binding.oracle_match for a scan -> (score, pose, best, info)."""
    from oracle.binding import oracle_match
    slot, pose, pts = scan
    cells, res, max_xy, _ = grids()[slot]
    return oracle_match(np.asarray(pose, np.float64), pts, cells, res, max_xy, *(option_values or ()))


def check_against_oracle(result, oracle):
    score, pose, best, info = oracle
    assert result.status == 0
    assert result.info == info and result.best == best, (result.best, best, result.info, info)
    assert abs(result.score - score) <= SCORE_RTOL * score, (result.score, score)
    assert np.abs(result.pose_estimate - pose).max() < POSE_TOL


def same_bits(a, b):
    """Exact equality of two match results: score bits, pose, best, info (and status where both have one)."""
    return (np.float64(a.score).tobytes() == np.float64(b.score).tobytes() and a.pose_estimate.tobytes() == b.pose_estimate.tobytes()
            and a.best == b.best and a.info == b.info and getattr(a, "status", 0) == getattr(b, "status", 0))
