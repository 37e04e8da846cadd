"""The fleet scan matcher's C ABI (rgrid_batch_* of include/rgrid.h) without a GPU: the library loads, exports what the header
declares, agrees with the ctypes mirror on the scan structure and the ABI version, and refuses null handles with a code."""
from __future__ import annotations

import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, "include", "rgrid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _lib():
    from reflector_ekf_slam_amd import fleet_match
    return fleet_match._batch_lib()


def test_scan_structure_size():
    from reflector_ekf_slam_amd import fleet_match
    assert _lib().rgrid_batch_sizeof_scan() == C.sizeof(fleet_match.RgridBatchScan)


def test_abi_version_is_4():
    from reflector_ekf_slam_amd import grid
    assert _lib().rgrid_abi_version() == 4 == grid.RGRID_ABI_VERSION
    assert int(re.search(r"#define\s+RGRID_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4


def test_every_declared_batch_symbol_is_exported():
    names = sorted(set(re.findall(r"\b(rgrid_batch_[a-z0-9_]+)\s*\(", _header())))
    assert {"rgrid_batch_create", "rgrid_batch_destroy", "rgrid_batch_set_grid", "rgrid_batch_match_submit", "rgrid_batch_match_collect",
            "rgrid_batch_sizeof_scan", "rgrid_batch_last_hip_error"} <= set(names)
    L = _lib()
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_null_handles_are_refused_with_a_code():
    from reflector_ekf_slam_amd import fleet_match
    from reflector_ekf_slam_amd.grid import _MatchOptions
    L = _lib()
    INVALID = fleet_match.RGRID_ERR_INVALID
    opt = _MatchOptions(0.2, 0.26, 0.1, 0.1)
    scan = fleet_match.RgridBatchScan()
    cells = (C.c_uint16 * 4)()
    buf = (C.c_double * 8)()
    assert L.rgrid_batch_create(1, 1, 1, 1, 1, 0, None) == INVALID
    h = C.c_void_p(1)
    for bad in ((0, 16, 1, 16, 8), (1, 0, 1, 16, 8), (1, 16, 0, 16, 8), (1, 16, 1, 0, 8), (1, 16, 1, 16, 0)):
        assert L.rgrid_batch_create(*bad, 0, C.byref(h)) == INVALID and h.value is None       # refused before any device call
        h = C.c_void_p(1)
    assert L.rgrid_batch_set_grid(None, 0, C.addressof(cells), 2, 2, 0.05, 1.0, 1.0) == INVALID
    assert L.rgrid_batch_match_submit(None, C.byref(opt), C.addressof(scan), 1) == INVALID
    assert L.rgrid_batch_match_collect(None, C.addressof(buf), C.addressof(buf), C.addressof(buf), None, None) == INVALID
    assert L.rgrid_batch_set_reduction(None, 0) == INVALID
    assert L.rgrid_batch_last_prepare_seconds(None) == 0.0
    assert L.rgrid_batch_last_hip_error(None) == b""
    L.rgrid_batch_destroy(None)


def test_package_exports_and_pose_fixes():
    import numpy as np
    import reflector_ekf_slam_amd as R
    from reflector_ekf_slam_amd import fleet_match as M
    assert R.ScanMatchFleet is M.ScanMatchFleet and R.pose_fixes is M.pose_fixes
    ok = M.FleetMatchResult(0.5, np.array([1.0, 2.0, 0.25]), (3, 0, -1), (107, 4, 8667), 0)
    bad = M.FleetMatchResult(0.0, np.zeros(3), (0, 0, 0), (0, 0, 0), M.RGRID_ERR_EMPTY)
    assert M.pose_fixes([ok, bad, ok]) == [(1.0, 2.0, 0.25), None, (1.0, 2.0, 0.25)]
    arr, count, keep = M.ScanMatchFleet.pack([(1, (0.5, -0.5, 0.1), np.ones((3, 2))), (0, np.zeros(3), np.zeros((0, 2)))])
    assert count == 2 and arr[0].grid == 1 and arr[0].n == 3 and arr[0].points_xy == keep[0].ctypes.data and keep[0].dtype == np.float32
    assert arr[1].n == 0 and arr[1].points_xy is None and tuple(arr[0].initial_pose) == (0.5, -0.5, 0.1)
