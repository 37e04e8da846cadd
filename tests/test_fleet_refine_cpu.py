"""The fleet refinement's C ABI and Python layer without a GPU (rgrid_batch_refine_* / rgrid_batch_scan_match_* of include/rgrid.h,
ScanMatchFleet.refine / .scan_match): the header declares what the library exports, the ctypes mirror agrees with it, a library
without the calls is reported on their first use only, pose_fixes hands out the refined poses -- and the conditions the GPU cases
of tests/fleet_refine_cases.py rely on hold in the oracle."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fleet_match_cases as MC
from tests import fleet_refine_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rgrid_batch_refine_submit", "rgrid_batch_refine_collect", "rgrid_batch_scan_match_submit", "rgrid_batch_scan_match_collect",
       "rgrid_batch_sizeof_refine_scan")


def _header():
    text = open(os.path.join(ROOT, "include", "rgrid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_five_calls_and_the_structure():
    h = _header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
    body = re.search(r"typedef\s+struct\s+rgrid_batch_refine_scan\s*\{(.*?)\}\s*rgrid_batch_refine_scan\s*;", h, flags=re.S).group(1)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["int grid", "int n", "const float *points_xy", "double target_translation[2]", "double initial_pose[3]"]


def test_abi_version_stays_4():
    from reflector_ekf_slam_amd import fleet_match, grid
    assert int(re.search(r"#define\s+RGRID_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4 == grid.RGRID_ABI_VERSION
    assert fleet_match._batch_lib().rgrid_abi_version() == 4


def test_library_exports_them_and_agrees_on_the_layout():
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._refine_lib()
    assert not [n for n in NEW if not hasattr(L, n)]
    assert L.rgrid_batch_sizeof_refine_scan() == C.sizeof(M.RgridBatchRefineScan) == 56
    assert M.RgridBatchRefineScan.target_translation.offset == 16 and M.RgridBatchRefineScan.initial_pose.offset == 32


def test_null_handles_are_refused_with_a_code():
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import _MatchOptions, _RefineOptions
    L = M._refine_lib()
    mo, ro = _MatchOptions(0.2, 0.26, 0.1, 0.1), _RefineOptions(1.0, 0.1, 0.4, 100, 1)
    scan, rscan = M.RgridBatchScan(), M.RgridBatchRefineScan()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    assert L.rgrid_batch_refine_submit(None, C.byref(ro), C.addressof(rscan), 1) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_refine_collect(None, a, a, None) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_scan_match_submit(None, C.byref(mo), C.byref(ro), C.addressof(scan), 1) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_scan_match_collect(None, a, a, a, None, None, a, None) == M.RGRID_ERR_INVALID


class _Without:
    """The built library seen through a filter: without the names in `hidden`, with `replaced` in place of others."""

    def __init__(self, real, hidden=(), replaced=None):
        self._real, self._hidden, self._replaced = real, set(hidden), dict(replaced or {})

    def __getattr__(self, name):
        if name in self._hidden:
            raise AttributeError(name)
        if name in self._replaced:
            return self._replaced[name]
        return getattr(self._real, name)


def test_a_library_without_the_calls_is_reported_by_them_only(monkeypatch):
    from reflector_ekf_slam_amd import _lib
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import _MatchOptions
    real = M._batch_lib()
    for hidden in (NEW, NEW[2:3]):
        old = _Without(real, hidden)
        monkeypatch.setattr(M._batch_lib, "ready", old)
        monkeypatch.setattr(M._refine_lib, "ready", None)
        m = object.__new__(M.ScanMatchFleet)                       # a handle as an older library would have made it
        m._L, m._h, m._pending = old, None, None
        for call in (lambda: m.submit_refine_code([]), m.collect_refine_code, lambda: m.submit_scan_match_code([]), m.collect_scan_match_code,
                     lambda: m.refine([]), lambda: m.scan_match([])):
            with pytest.raises(_lib.LibraryMissing) as e:
                call()
            assert hidden[0] in str(e.value)
        # the calls it has keep working
        assert M._batch_lib() is old and old.rgrid_batch_sizeof_scan() == C.sizeof(M.RgridBatchScan)
        assert m.submit_packed_code(M.ScanMatchFleet.pack([])) == M.RGRID_ERR_INVALID      # (a null handle: refused by the library itself)
        assert old.rgrid_batch_match_submit(None, C.byref(_MatchOptions(0.2, 0.26, 0.1, 0.1)), None, 0) == M.RGRID_ERR_INVALID
    # a library whose structure has another size
    def wrong_size():
        return 48
    monkeypatch.setattr(M._batch_lib, "ready", _Without(real, (), {"rgrid_batch_sizeof_refine_scan": wrong_size}))
    monkeypatch.setattr(M._refine_lib, "ready", None)
    with pytest.raises(_lib.LibraryMissing) as e:
        M._refine_lib()
    assert "48" in str(e.value) and "56" in str(e.value)
    monkeypatch.setattr(M._batch_lib, "ready", real)
    monkeypatch.setattr(M._refine_lib, "ready", None)
    assert M._refine_lib() is real


def test_package_exports_packing_and_pose_fixes():
    import reflector_ekf_slam_amd as R
    from reflector_ekf_slam_amd import fleet_match as M
    assert R.FleetRefineResult is M.FleetRefineResult and R.FleetScanMatchResult is M.FleetScanMatchResult
    coarse = M.FleetMatchResult(0.5, np.array([1.0, 2.0, 0.25]), (3, 0, -1), (107, 4, 8667), 0)
    fine = M.FleetRefineResult(np.array([1.01, 2.02, 0.26]), 0.3, 0.2, 7, 0, 0)
    ok = M.FleetScanMatchResult(coarse, fine)
    bad = M.FleetScanMatchResult(M.FleetMatchResult(0.0, np.zeros(3), (0, 0, 0), (0, 0, 0), M.RGRID_ERR_EMPTY),
                                 M.FleetRefineResult(np.zeros(3), 0.0, 0.0, 0, 0, M.RGRID_ERR_EMPTY))
    assert ok.status == 0 and bad.status == M.RGRID_ERR_EMPTY and ok.pose_estimate is fine.pose_estimate
    assert M.pose_fixes([ok, bad, ok]) == [(1.01, 2.02, 0.26), None, (1.01, 2.02, 0.26)]
    assert M.pose_fixes([fine, bad.fine]) == [(1.01, 2.02, 0.26), None]
    assert M.pose_fixes([coarse, bad.coarse, coarse]) == [(1.0, 2.0, 0.25), None, (1.0, 2.0, 0.25)]       # as before
    arr, count, keep = M.ScanMatchFleet.pack_refine([(1, (0.5, -0.5), (0.6, -0.4, 0.1), np.ones((3, 2))),
                                                     (0, np.zeros(2), np.zeros(3), np.zeros((0, 2)))])
    assert count == 2 and arr[0].grid == 1 and arr[0].n == 3 and arr[0].points_xy == keep[0].ctypes.data and keep[0].dtype == np.float32
    assert tuple(arr[0].target_translation) == (0.5, -0.5) and tuple(arr[0].initial_pose) == (0.6, -0.4, 0.1)
    assert arr[1].n == 0 and arr[1].points_xy is None


def test_shape_case_reaches_every_thread_count():
    scans = RC.shape_match_scans()
    counts = [s[2].shape[0] for s in scans[:len(RC.SHAPE_COUNTS)]]
    assert tuple(counts) == RC.SHAPE_COUNTS and [s[0] for s in scans[:4]] == [0, 1, 0, 1]
    threads = {RC.threads_of(n) for n in counts}
    assert {64, 128, 1024} <= threads and len(threads) >= 5
    assert RC.threads_of(1023) == RC.threads_of(1024) == RC.threads_of(1025) == 1024 and max(counts) > 2 * 1024   # a stride that wraps, twice
    assert 0.05 < MC.partly_outside_fraction(scans[-2]) < 0.95
    assert MC.partly_outside_fraction(scans[-1]) == 1.0


def test_case_conditions_in_the_oracle(oracle_lib):
    """The GPU cases end the ways they are meant to: the iteration limit binds (termination 1), a default case converges
    (termination 0), a cloud far outside the grid keeps its start pose."""
    scans = RC.shape_match_scans()
    k = RC.SHAPE_COUNTS.index(500)
    start = MC.oracle_of(scans[k])[1]                                              # the correlative matcher's answer
    rs = RC.refine_scan(scans[k], start)
    pose, summ = RC.oracle_refine(rs, RC.OPTION_SETS[2])
    assert RC.OPTION_SETS[2][3] == 3 and (summ["iterations"], summ["termination"]) == (3, 1)
    pose, summ = RC.oracle_refine(rs, RC.OPTION_SETS[0])
    assert summ["termination"] == 0 and 3 < summ["iterations"] < 100 and summ["final_cost"] < summ["initial_cost"]
    assert np.abs(pose - start).max() > 1e-4                                       # the refinement moves the matcher's pose
    far = (0, np.zeros(2), np.zeros(3), RC.FAR_CLOUD)
    pose, summ = RC.oracle_refine(far)
    assert np.abs(pose).max() <= 1e-12
