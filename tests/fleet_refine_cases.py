"""Cases of the fleet refinement (rgrid_batch_refine_* / rgrid_batch_scan_match_* of include/rgrid.h, ScanMatchFleet.refine and
.scan_match), shared by tests/test_fleet_refine_cpu.py and tests/test_fleet_refine_gpu.py.  Built on tests/grid_cases.py and
tests/fleet_match_cases.py: the same two room grids (slot 0 = 0.05 m, slot 1 = 0.1 m).

A "match scan" is ``(grid_slot, prediction, points_xy)`` as ``ScanMatchFleet.submit`` takes it; a "refine scan" is
``(grid_slot, target_translation, start_pose, points_xy)`` as ``ScanMatchFleet.submit_refine`` takes it.
"""
from __future__ import annotations

import math

import numpy as np

from tests import fleet_match_cases as MC
from tests.grid_cases import room_grid, scan_of

# Point counts on both sides of every thread count rgrid_refine_match launches with (T = min(1024, roundup64(n))): one wave, one
# wave full, two waves, the last count below 1024 threads, exactly 1024, and two counts whose evaluation loop wraps (n > 1024).
SHAPE_COUNTS = (1, 3, 63, 64, 65, 127, 129, 500, 1023, 1024, 1025, 2400)

# CeresScanMatcherOptions2D argument sets: default, heavy priors without non-monotonic steps, an iteration limit that binds
OPTION_SETS = ((), (2.0, 10.0, 40.0, 100, False), (1.0, 0.1, 0.4, 3, True))


def threads_of(n):
    """Threads rgrid_refine_match gives a scan of n points."""
    return min(1024, (n + 63) // 64 * 64)


def options_of(values):
    from reflector_ekf_slam_amd.grid import CeresScanMatcherOptions2D
    return CeresScanMatcherOptions2D(*values)


_shape = None


def shape_match_scans():
    """SHAPE_COUNTS alternating between the two grid slots, then fleet_match_cases.shape_scans()'s scan partly outside its grid and
    its cloud wholly outside (match scans: the start poses are the correlative matcher's)."""
    global _shape
    if _shape is None:
        scans = []
        for k, n in enumerate(SHAPE_COUNTS):
            slot = k % 2
            occ = MC.grids()[slot][3]
            true = np.array([0.4 * k - 2.0, 1.5 - 0.25 * k, 0.5 * k - 2.5])
            pts = scan_of(occ, true, n_points=n, seed=400 + k)
            assert pts.shape[0] == n
            scans.append((slot, true + np.array([0.07, -0.05, math.radians(2.5)]), pts))
        other = MC.shape_scans()
        scans += [other[7], other[8]]
        _shape = scans
    return _shape


FAR_CLOUD = np.array([[500.0, 500.0], [501.0, 500.0]], np.float32)     # test_refine_match_follows_the_oracle_iterate_for_iterate's


def refine_scan(match_scan, start_pose):
    slot, prediction, pts = match_scan
    return (slot, np.asarray(prediction, np.float64)[:2].copy(), np.asarray(start_pose, np.float64).copy(), pts)


def oracle_refine(scan, values=()):
    """oracle.binding.oracle_refine_match for a refine scan -> (pose, summary dict)."""
    from oracle.binding import oracle_refine_match
    slot, target, start, pts = scan
    cells, res, max_xy, _ = MC.grids()[slot]
    return oracle_refine_match(target, start, pts, cells, res, max_xy, *values)


_trials = None


def oracle_trials():
    """The map and the six trials of tests/test_grid_gpu.py::test_refine_match_follows_the_oracle_iterate_for_iterate, by its own
    construction: -> (cells, res, max_xy, [(true, prediction, points)]).  Needs the oracle library (the map is the inserter's)."""
    global _trials
    if _trials is None:
        from oracle.binding import oracle_insert
        _, max_xy, occ = room_grid()
        res = 0.05
        cells = np.zeros((480, 480), np.uint16)
        for k, pose in enumerate(((0.0, 0.0, 0.0), (1.0, -0.5, 0.7), (-1.5, 0.8, -1.2))):
            loc = scan_of(occ, pose, n_points=1200, seed=60 + k)
            c, s = math.cos(pose[2]), math.sin(pose[2])
            world = np.stack([pose[0] + c * loc[:, 0] - s * loc[:, 1], pose[1] + s * loc[:, 0] + c * loc[:, 1]], 1).astype(np.float32)
            cells = oracle_insert(cells, res, max_xy, np.array(pose[:2], np.float32), world)
        rng = np.random.default_rng(5)
        trials = []
        for trial in range(6):
            true = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(-3.0, 3.0)])
            pts = scan_of(occ, true, n_points=(3, 64, 500, 700, 2400, 5000)[trial], seed=100 + trial).astype(np.float32)
            prediction = true + rng.uniform(-1, 1, 3) * [0.08, 0.08, 0.04]
            trials.append((true, prediction, pts))
        _trials = (cells, res, max_xy, trials)
    return _trials


def same_refine_bits(a, b):
    """Exact equality of two refine results: pose bytes, both costs' bits, iterations, termination (and status where both have one)."""
    f = lambda v: np.float64(v).tobytes()
    return (np.asarray(a.pose_estimate, np.float64).tobytes() == np.asarray(b.pose_estimate, np.float64).tobytes()
            and f(a.initial_cost) == f(b.initial_cost) and f(a.final_cost) == f(b.final_cost)
            and (a.iterations, a.termination) == (b.iterations, b.termination) and getattr(a, "status", 0) == getattr(b, "status", 0))


def is_zero_refine(r):
    return (not np.asarray(r.pose_estimate).any() and r.initial_cost == 0.0 and r.final_cost == 0.0 and r.iterations == 0
            and r.termination == 0)
