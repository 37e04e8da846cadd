"""The fleet texture's C ABI and Python layer without a GPU (rgrid_batch_texture_* of include/rgrid.h,
ScanMatchFleet.draw_textures): the header declares what the library exports, a library without the calls is reported on their first
use only -- and the conditions the GPU cases of tests/fleet_texture_cases.py rely on hold in the oracle, whose geometry a numpy
model restates."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fleet_texture_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rgrid_batch_texture_submit", "rgrid_batch_texture_collect")


def _header():
    text = open(os.path.join(ROOT, "include", "rgrid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_two_calls():
    h = _header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
    args = lambda name: [re.sub(r"\s+", " ", a).strip() for a in re.search(name + r"\s*\((.*?)\)\s*;", h, flags=re.S).group(1).split(",")]
    assert args(NEW[0]) == ["rgrid_batch_t *b", "const int *grids", "int count"]
    assert args(NEW[1]) == ["rgrid_batch_t *b", "int *boxes", "double *slice_max", "long *offsets", "uint8_t *cells", "long cap"]


def test_library_exports_them():
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._texture_lib()
    assert not [n for n in NEW if not hasattr(L, n)]
    assert L is M._batch_lib()


def test_abi_version_stays_4():
    from reflector_ekf_slam_amd import fleet_match, grid
    assert int(re.search(r"#define\s+RGRID_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4 == grid.RGRID_ABI_VERSION
    assert fleet_match._texture_lib().rgrid_abi_version() == 4


def test_null_handles_are_refused_with_a_code():
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._texture_lib()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    assert L.rgrid_batch_texture_submit(None, a, 1) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_texture_submit(None, None, 0) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_texture_collect(None, a, a, a, a, 8) == M.RGRID_ERR_INVALID


class _Without:
    """The built library seen through a filter: without the names in `hidden`."""

    def __init__(self, real, hidden=()):
        self._real, self._hidden = real, set(hidden)

    def __getattr__(self, name):
        if name in self._hidden:
            raise AttributeError(name)
        return getattr(self._real, name)


def test_a_library_without_the_calls_is_reported_by_them_only(monkeypatch):
    from reflector_ekf_slam_amd import _lib
    from reflector_ekf_slam_amd import fleet_match as M
    real = M._batch_lib()
    insert = M._insert_lib()
    for hidden in (NEW, NEW[1:]):
        old = _Without(real, hidden)
        monkeypatch.setattr(M._batch_lib, "ready", old)
        monkeypatch.setattr(M._insert_lib, "ready", None)
        monkeypatch.setattr(M._texture_lib, "ready", None)
        m = object.__new__(M.ScanMatchFleet)                       # a handle as an older library would have made it
        m._L, m._h, m._pending, m.num_grids = old, None, None, 1
        for call in (lambda: m.submit_texture_code([]), m.collect_texture_code, lambda: m.submit_texture([0]), m.collect_texture,
                     lambda: m.draw_textures([]), m.draw_textures, lambda: m.submap_textures([], [])):
            with pytest.raises(_lib.LibraryMissing) as e:
                call()
            assert hidden[0] in str(e.value)
        # the calls it has keep working
        assert M._batch_lib() is old and M._insert_lib() is old
        assert m.submit_packed_code(M.ScanMatchFleet.pack([])) == M.RGRID_ERR_INVALID      # (a null handle: refused by the library itself)
        assert m.submit_insert_code([]) == M.RGRID_ERR_INVALID
        assert m.GetLimits_code(0)[0] == M.RGRID_ERR_INVALID
    monkeypatch.setattr(M._batch_lib, "ready", real)
    monkeypatch.setattr(M._insert_lib, "ready", insert)
    monkeypatch.setattr(M._texture_lib, "ready", None)
    assert M._texture_lib() is real


def test_package_exports_and_the_texture_record():
    import reflector_ekf_slam_amd as R
    from reflector_ekf_slam_amd import fleet_match as M
    assert R.FleetTexture is M.FleetTexture
    for name in ("submit_texture_code", "submit_texture", "collect_texture_code", "collect_texture", "draw_textures", "submap_textures",
                 "set_slots"):
        assert callable(getattr(M.ScanMatchFleet, name)), name
    t = M.FleetTexture(np.zeros((1, 1, 2), np.uint8), (0, 0, 1, 1), (1.0, 2.0))
    cells, box, sm = t                                             # unpacks like GridFrontEnd.DrawTexture's answer
    assert cells is t.cells and box == (0, 0, 1, 1) and sm == (1.0, 2.0)


def test_sweep_holds_its_conditions_in_the_oracle(oracle_lib):
    grids = TC.sweep_case()
    assert len(grids) == len(TC.SWEEP_NAMES) == 8 and TC.SWEEP_MAX_CELLS % 2 == 1
    assert max(g[0].size for g in grids) == TC.SWEEP_MAX_CELLS
    assert sorted((k * TC.SWEEP_MAX_CELLS) % TC.VEC for k in range(8)) == list(range(8))   # every alignment of a slot's start
    shape = lambda k: grids[k][0].shape
    box = [TC.oracle_texture(g)[1] for g in grids]
    tex = [TC.oracle_texture(g)[0] for g in grids]
    ny, nx = shape(0)
    assert nx % 2 == 1 and nx % 8 and nx != ny and 0 < box[0][2] < nx and 0 < box[0][3] < ny and np.count_nonzero(grids[0][0]) > 200
    assert grids[1][0].size == TC.WG_THREADS + 1 and grids[2][0].size == 2 * TC.WG_THREADS - 1
    ny, nx = shape(1)                                                               # the last row only; odd width at an odd offset_x
    assert box[1][1] == ny - 1 and box[1][3] == 1 and box[1][0] % 2 == 1 and box[1][2] % 2 == 1 and not grids[1][0][:-1].any()
    ny, nx = shape(2)                                                               # the last column only
    assert box[2][0] == nx - 1 and box[2][2] == 1 and box[2][3] > 1 and not grids[2][0][:, :-1].any()
    assert shape(3) == (1, 1) and box[3] == (0, 0, 1, 1) and tex[3].tolist() != [[[0, 0]]]
    assert not grids[4][0].any() and box[4] == (0, 0, 1, 1) and tex[4].tolist() == [[[0, 0]]]        # the empty slot
    assert box[5] == (0, 0, 1, 1) and np.count_nonzero(grids[5][0]) == 1 and tex[5].tolist() != [[[0, 0]]]
    ny, nx = shape(6)
    assert box[6] == (nx - 1, ny - 1, 1, 1) and np.count_nonzero(grids[6][0]) == 1
    ny, nx = shape(7)                                                               # all four borders, the whole table
    assert box[7] == (0, 0, nx, ny)
    known = grids[7][0][grids[7][0] != 0]
    assert np.array_equal(np.sort(known), np.arange(1, 32768)) and known.size < grids[7][0].size
    assert len(set(box)) >= 6 and len({g[0].shape for g in grids}) >= 7             # boxes and shapes differ between slots
    sm = [TC.oracle_texture(g)[2] for g in grids]
    assert len(set(sm)) == 8


def test_multi_pass_slot_has_several_passes_and_garbage_behind_it(oracle_lib):
    garbage, grid = TC.multi_pass_case()
    assert grid[0].size > 2 * TC.PASS_CELLS and grid[0].size < garbage[0].size == TC.MULTI_MAX_CELLS and TC.MULTI_MAX_CELLS % 2 == 1
    assert (TC.MULTI_SLOT * TC.MULTI_MAX_CELLS) % TC.VEC not in (0, 4)              # the slot's start: 2-byte aligned, no more
    behind = garbage[0].reshape(-1)[grid[0].size:]
    assert behind.size == TC.MULTI_MAX_CELLS - grid[0].size and behind.all()        # what stays in the pool behind the grid
    tex, box, _ = TC.oracle_texture(grid)
    assert box == (7, 10, 244, 191) and box[2] * box[3] % TC.VEC                     # a tail of single pairs behind the 16-byte stores
    # what a kernel that read on to max_cells would see: the box grows
    past = np.concatenate([grid[0].reshape(-1), behind])
    rows = -(-past.size // grid[0].shape[1])
    seen = np.zeros(rows * grid[0].shape[1], np.uint16)
    seen[:past.size] = past
    assert TC.oracle_texture((seen.reshape(rows, -1), grid[1], grid[2]))[1] != box


def test_the_model_equals_the_oracle_and_every_defect_shows(oracle_lib):
    table = TC.byte_table()
    assert table.shape == (32768, 2) and table[0].tolist() == [0, 0] and len({tuple(p) for p in table.tolist()}) > 200
    grids = TC.sweep_case() + [TC.multi_pass_case()[1]]
    want = [TC.oracle_texture(g) for g in grids]
    for k, g in enumerate(grids):
        assert TC.same_texture(TC.model_texture(g, table), want[k]), k
    for defect in TC.DEFECTS:
        differ = [k for k, g in enumerate(grids) if not TC.same_texture(TC.model_texture(g, table, defect), want[k])]
        assert differ, defect
    swapped = TC.model_texture(grids[1], table, "swapped")[1]
    assert swapped == (want[1][1][1], want[1][1][0], want[1][1][3], want[1][1][2])
    assert TC.model_texture(grids[7], table, "exclusive")[1] == (0, 0, 182, 180)
    got, ref = TC.model_texture(grids[6], table, "slice"), want[6]
    assert got[1] == ref[1] and np.array_equal(got[0], ref[0]) and got[2] != ref[2]


def test_submap_scene_grows_the_initial_submap(oracle_lib):
    from oracle.binding import oracle_grow
    n, res = TC.SUBMAP_N, float(np.float32(TC.SUBMAP_RES))
    scans = TC.submap_scene()
    origin = scans[0][0]
    cells, max_xy = np.zeros((n, n), np.uint16), (float(origin[0]) + 0.5 * n * res, float(origin[1]) + 0.5 * n * res)
    sizes = []
    for org, ret, mis in scans:
        cells, max_xy, _ = oracle_grow(cells, res, max_xy, org, ret, mis)
        sizes.append(cells.shape)
    assert sizes[0] == (n, n) and sizes[-1][0] > n and sizes[-1][0] * sizes[-1][1] <= TC.SUBMAP_MAX_CELLS
