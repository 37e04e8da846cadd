"""The fleet inserter's C ABI and Python layer without a GPU (rgrid_batch_insert_* / rgrid_batch_get_* of include/rgrid.h,
ScanMatchFleet.insert): the header declares what the library exports, the ctypes mirror agrees with it, a library without the calls
is reported on their first use only -- and the conditions the GPU cases of tests/fleet_insert_cases.py rely on hold in the oracle."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fleet_insert_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rgrid_batch_insert_submit", "rgrid_batch_insert_collect", "rgrid_batch_get_limits", "rgrid_batch_get_grid",
       "rgrid_batch_sizeof_insert_scan")


def _header():
    text = open(os.path.join(ROOT, "include", "rgrid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_five_calls_and_the_structures():
    h = _header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
    body = re.search(r"typedef\s+struct\s+rgrid_batch_insert_scan\s*\{(.*?)\}\s*rgrid_batch_insert_scan\s*;", h, flags=re.S).group(1)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["int grid", "int n_returns, n_misses", "const float *returns_xy, *misses_xy", "float origin_xy[2]"]
    body = re.search(r"typedef\s+struct\s+rgrid_insert_options\s*\{(.*?)\}\s*rgrid_insert_options\s*;", h, flags=re.S).group(1)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["float hit_probability, miss_probability", "int insert_free_space"]


def test_library_exports_them_and_agrees_on_the_layout():
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._insert_lib()
    assert not [n for n in NEW if not hasattr(L, n)]
    S = M.RgridBatchInsertScan
    assert L.rgrid_batch_sizeof_insert_scan() == C.sizeof(S) == 40
    assert [f[0] for f in S._fields_] == ["grid", "n_returns", "n_misses", "returns_xy", "misses_xy", "origin_xy"]
    assert (S.n_misses.offset, S.returns_xy.offset, S.misses_xy.offset, S.origin_xy.offset) == (8, 16, 24, 32)
    assert C.sizeof(M._InsertOptions) == 12


def test_abi_version_stays_4():
    from reflector_ekf_slam_amd import fleet_match, grid
    assert int(re.search(r"#define\s+RGRID_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4 == grid.RGRID_ABI_VERSION
    assert fleet_match._insert_lib().rgrid_abi_version() == 4


def test_null_handles_are_refused_with_a_code():
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._insert_lib()
    opt, scan = M._InsertOptions(0.55, 0.49, 1), M.RgridBatchInsertScan()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    assert L.rgrid_batch_insert_submit(None, C.byref(opt), C.addressof(scan), 1) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_insert_collect(None, a) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_get_limits(None, 0, None, None, None, None, None) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_get_grid(None, 0, a, 4) == M.RGRID_ERR_INVALID


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
    refine = M._refine_lib()
    for hidden in (NEW, NEW[3:4]):
        old = _Without(real, hidden)
        monkeypatch.setattr(M._batch_lib, "ready", old)
        monkeypatch.setattr(M._refine_lib, "ready", None)
        monkeypatch.setattr(M._insert_lib, "ready", None)
        m = object.__new__(M.ScanMatchFleet)                       # a handle as an older library would have made it
        m._L, m._h, m._pending = old, None, None
        for call in (lambda: m.submit_insert_code([]), m.collect_insert_code, lambda: m.insert([]), lambda: m.GetGrid(0),
                     lambda: m.GetLimits(0)):
            with pytest.raises(_lib.LibraryMissing) as e:
                call()
            assert hidden[0] in str(e.value)
        # the calls it has keep working
        assert M._batch_lib() is old and M._refine_lib() is old
        assert m.submit_packed_code(M.ScanMatchFleet.pack([])) == M.RGRID_ERR_INVALID      # (a null handle: refused by the library itself)
        assert m.submit_refine_code([]) == M.RGRID_ERR_INVALID
        assert old.rgrid_batch_match_submit(None, C.byref(_MatchOptions(0.2, 0.26, 0.1, 0.1)), None, 0) == M.RGRID_ERR_INVALID
    # a library whose structure has another size
    monkeypatch.setattr(M._batch_lib, "ready", _Without(real, (), {"rgrid_batch_sizeof_insert_scan": lambda: 32}))
    monkeypatch.setattr(M._insert_lib, "ready", None)
    with pytest.raises(_lib.LibraryMissing) as e:
        M._insert_lib()
    assert "32" in str(e.value) and "40" in str(e.value)
    monkeypatch.setattr(M._batch_lib, "ready", real)
    monkeypatch.setattr(M._refine_lib, "ready", refine)
    monkeypatch.setattr(M._insert_lib, "ready", None)
    assert M._insert_lib() is real


def test_package_exports_and_packing():
    import reflector_ekf_slam_amd as R
    from reflector_ekf_slam_amd import fleet_match as M
    assert R.RgridBatchInsertScan is M.RgridBatchInsertScan and R.ScanMatchFleet is M.ScanMatchFleet
    for name in ("pack_insert", "submit_insert_packed_code", "submit_insert_code", "submit_insert", "collect_insert_code", "collect_insert",
                 "insert", "GetGrid", "GetLimits"):
        assert callable(getattr(M.ScanMatchFleet, name)), name
    ret = np.arange(6, dtype=np.float64).reshape(3, 2) + 0.1                       # converted to float32
    arr, count, keep = M.ScanMatchFleet.pack_insert([(2, (0.5, -0.25), ret, None), (0, np.zeros(2), np.zeros((0, 2)), [[1.0, 2.0]])])
    assert count == 2 and (arr[0].grid, arr[0].n_returns, arr[0].n_misses) == (2, 3, 0)
    assert arr[0].returns_xy == keep[0].ctypes.data and keep[0].dtype == np.float32 and np.array_equal(keep[0], ret.astype(np.float32))
    assert arr[0].misses_xy is None and tuple(arr[0].origin_xy) == (0.5, -0.25)
    assert (arr[1].n_returns, arr[1].n_misses) == (0, 1) and arr[1].returns_xy is None and arr[1].misses_xy == keep[3].ctypes.data
    o = M._insert_options(None)
    assert (o.hit_probability, o.miss_probability, o.insert_free_space) == (np.float32(0.55), np.float32(0.49), 1)


def test_shape_counts_sit_on_both_sides_of_the_kernels_strides():
    grids, scans = IC.shape_case()
    assert [(s[2].shape[0], 0 if s[3] is None else s[3].shape[0]) for s in scans] == list(IC.SHAPE_COUNTS)
    assert [s[0] for s in scans] == list(range(8)) and all(g[0].shape == (120, 120) and g[1] == 0.1 for g in grids)
    rets = {c[0] for c in IC.SHAPE_COUNTS}
    rays = {c[0] + c[1] for c in IC.SHAPE_COUNTS}
    assert {63, 64, 65} <= rets and 0 in rays
    assert min(r for r in rays if r) < IC.WG_WAVES < max(rays) and max(rays) > 64 * IC.WG_WAVES        # ... and of its thread count
    assert any(g[0].any() for g in grids) and any(not g[0].any() for g in grids)


def test_growth_sequence_grows_on_every_side_and_doubles_twice_in_a_step(oracle_lib):
    from oracle.binding import oracle_grow
    for (grid, scans), (ny, nx) in zip(IC.growth_case(), IC.GROW_SHAPES):
        assert grid[0].shape == (ny, nx) and (ny % 2 == 1 or nx == 40)
        sides, factors, left = set(), [], set()
        for k, scan in enumerate(scans):
            old = grid[0].shape
            far = scan[2][0]
            lo = (grid[2][0] - grid[1] * old[0], grid[2][1] - grid[1] * old[1])
            left |= {s for s, out in (("+x", far[0] > grid[2][0]), ("-x", far[0] <= lo[0]), ("+y", far[1] > grid[2][1]), ("-y", far[1] <= lo[1])) if out}
            _, _, off = oracle_grow(grid[0], grid[1], grid[2], scan[1], scan[2], scan[3])
            cells, lim = IC.oracle_pair(grid, scan)
            factors.append(cells.shape[0] // old[0])
            assert cells.shape[0] * cells.shape[1] <= IC.GROW_MAX_CELLS
            if cells.shape != old:                                                  # new cells before and behind the old ones, on both axes
                sides |= {s for s, m in (("left", off[0]), ("top", off[1]), ("right", cells.shape[1] - off[0] - old[1]),
                                         ("bottom", cells.shape[0] - off[1] - old[0])) if m > 0}
            grid = (cells, grid[1], (lim[3], lim[4]))
        assert factors[0] == 1 and max(factors) >= 4 and 2 in factors               # none, one doubling, two in one step
        assert sides == {"left", "top", "right", "bottom"} and {"+x", "-y"} <= left  # the scans leave the map on more than one side
        assert grid[0].shape[0] >= 8 * ny


def test_status_case_conditions(oracle_lib):
    from oracle.binding import oracle_grow
    grids, scans, want = IC.status_case()
    grown = lambda k: oracle_grow(grids[k][0], grids[k][1], grids[k][2], scans[k][1], scans[k][2], scans[k][3])[0]
    assert grown(0).size > IC.STATUS_MAX_CELLS                                   # the capacity case really exceeds max_cells
    assert np.isnan(scans[1][2]).any() and want[1] == IC.INVALID
    assert scans[2][2].shape[0] > IC.STATUS_MAX_POINTS and grown(2).shape == grids[2][0].shape
    assert scans[3][2].shape[0] > IC.STATUS_MAX_POINTS and grids[3][0].size < grown(3).size <= IC.STATUS_MAX_CELLS
    assert grown(4).shape == grids[4][0].shape and grids[5][0].size < grown(5).size <= IC.STATUS_MAX_CELLS
    assert len({s[0] for s in scans}) == len(scans)


def test_corner_case_has_a_cell_that_a_ray_crosses_and_a_return_hits(oracle_lib):
    """The return one cell from the origin lies on the ray to the return two cells out: the hit wins there."""
    from oracle.binding import oracle_insert, oracle_lookup_table
    grids, scans = IC.corner_case()
    grid, (_, origin, ret, mis) = grids[0], scans[0]
    hit = int(oracle_lookup_table(0.55)[0]) - 32768
    miss = int(oracle_lookup_table(0.49)[0]) - 32768
    assert hit != miss
    near, far = ret[11 * 25 + 12], ret[10 * 25 + 12]                               # offsets (-1, 0) and (-2, 0) cells from the origin
    assert IC.cell_of(grid, near)[0] - IC.cell_of(grid, origin)[0] == 1 and IC.cell_of(grid, far)[0] - IC.cell_of(grid, origin)[0] == 2
    ray = oracle_insert(grid[0], grid[1], grid[2], origin, np.zeros((0, 2), np.float32), far[None])
    assert ray[IC.cell_of(grid, near)] == miss                                     # the ray to `far` crosses the cell of `near`
    both, _ = IC.oracle_pair(grid, scans[0])
    assert both[IC.cell_of(grid, near)] == hit and both[IC.cell_of(grid, far)] == hit
    assert np.count_nonzero(both == miss) > 100


def test_crowd_is_larger_than_the_chip():
    grids, scans = IC.crowd_case()
    assert len(scans) == IC.CROWD > 256 and len({s[0] for s in scans}) == IC.CROWD
    assert all(100 <= s[2].shape[0] <= 200 for s in scans) and all(g[0].shape == (64, 64) for g in grids)
