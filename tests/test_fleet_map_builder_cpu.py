"""The fleet MapBuilder's C ABI and Python layer without a GPU (rgrid_batch_add_range_data of include/rgrid.h,
ScanMatchFleet.add_range_data, map_builder.FleetMapBuilder): the header declares what the library exports, the ctypes mirror agrees
with it, a library without the calls is reported on their first use only -- and FleetMapBuilder's own part, which member's scan goes
where and what the host keeps per member, gives on every chain of tests/map_chain_cases.py what a MapBuilder per robot gives, both over
the CPU oracle front end."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fleet_filter_scan_cases as FC
from tests import map_chain_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rgrid_batch_add_range_data", "rgrid_batch_last_call_counts", "rgrid_batch_sizeof_range_data")


def _header():
    text = open(os.path.join(ROOT, "include", "rgrid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _fields(h, name):
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", h, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]


def test_header_declares_the_calls_and_the_structure():
    h = _header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
    assert _fields(h, "rgrid_batch_range_data") == ["int grid", "int n_returns, n_misses", "const float *returns_xy, *misses_xy", "float origin_xy[2]",
                                                    "double ekf_pose[3]"]
    assert re.search(r"rgrid_batch_add_range_data\s*\(\s*rgrid_batch_t\s*\*b,\s*const\s+rgrid_map_builder_options\s*\*opt,\s*"
                     r"const\s+rgrid_batch_range_data\s*\*scans,\s*int\s+count,\s*int\s*\*codes,\s*int\s*\*status,\s*double\s*\*local_poses,\s*"
                     r"float\s*\*origins_in_local,\s*float\s*\*returns_in_local,\s*long\s+cap_points\s*\)", h)
    assert re.search(r"rgrid_batch_last_call_counts\s*\(\s*rgrid_batch_t\s*\*b,\s*int\s+launches_syncs\[2\]\s*\)", h)
    assert re.search(r"rgrid_batch_sizeof_range_data\s*\(\s*void\s*\)", h)


def test_library_exports_them_and_agrees_on_the_layout():
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._range_data_lib()
    assert not [n for n in NEW if not hasattr(L, n)]
    S = M.RgridBatchRangeData
    assert L.rgrid_batch_sizeof_range_data() == C.sizeof(S) == 64
    assert [f[0] for f in S._fields_] == ["grid", "n_returns", "n_misses", "returns_xy", "misses_xy", "origin_xy", "ekf_pose"]
    assert (S.n_returns.offset, S.n_misses.offset, S.returns_xy.offset, S.misses_xy.offset, S.origin_xy.offset, S.ekf_pose.offset) == (4, 8, 16, 24, 32, 40)
    assert (M.SCAN_INSERTED, M.SCAN_DROPPED_EMPTY, M.SCAN_FILTERED_EMPTY) == (0, 1, 2)
    enum = re.search(r"enum\s*\{\s*RGRID_SCAN_INSERTED\s*=\s*0,\s*RGRID_SCAN_DROPPED_EMPTY\s*=\s*1,\s*RGRID_SCAN_FILTERED_EMPTY\s*=\s*2\s*\}", _header())
    assert enum


def test_abi_version_stays_4():
    from reflector_ekf_slam_amd import fleet_match, grid
    assert int(re.search(r"#define\s+RGRID_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4 == grid.RGRID_ABI_VERSION
    assert fleet_match._range_data_lib().rgrid_abi_version() == 4


def test_null_pointers_are_refused_with_a_code():
    """Before any HIP call: there is no GPU here, and no handle."""
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._range_data_lib()
    opt, scan = M._map_builder_options(None), M.RgridBatchRangeData()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    assert L.rgrid_batch_add_range_data(None, C.byref(opt), C.addressof(scan), 1, a, a, a, a, a, 4) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_add_range_data(None, None, None, 0, None, None, None, None, None, 0) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_last_call_counts(None, a) == M.RGRID_ERR_INVALID


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
    from reflector_ekf_slam_amd.map_builder import FleetMapBuilder, RangeData
    real = M._batch_lib()
    filt, insert = M._filter_lib(), M._insert_lib()
    rd = RangeData(np.zeros(2, np.float32), np.ones((3, 2), np.float32), None)
    for hidden in (NEW, NEW[1:2]):
        old = _Without(real, hidden)
        monkeypatch.setattr(M._batch_lib, "ready", old)
        for feature in (M._filter_lib, M._insert_lib, M._range_data_lib):
            monkeypatch.setattr(feature, "ready", None)
        m = object.__new__(M.ScanMatchFleet)                       # a handle as an older library would have made it
        m._L, m._h, m._pending, m._set_slots = old, None, None, set()
        builder = FleetMapBuilder(1, fleet=m)
        for call in (lambda: m.add_range_data_code([rd], [(0.0, 0.0, 0.0)]), lambda: m.add_range_data([], []), m.last_call_counts,
                     lambda: builder.AddRangeData([0.0], [rd], [(0.0, 0.0, 0.0)])):
            with pytest.raises(_lib.LibraryMissing) as e:
                call()
            assert hidden[0] in str(e.value)
        # the calls it has keep working
        assert M._batch_lib() is old and M._filter_lib() is old and M._insert_lib() is old
        assert m.submit_filter_code([]) == M.RGRID_ERR_INVALID and m.submit_insert_code([]) == M.RGRID_ERR_INVALID   # (a null handle: refused by the library itself)
    # a library whose structure has another size
    monkeypatch.setattr(M._batch_lib, "ready", _Without(real, (), {"rgrid_batch_sizeof_range_data": lambda: 56}))
    monkeypatch.setattr(M._range_data_lib, "ready", None)
    with pytest.raises(_lib.LibraryMissing) as e:
        M._range_data_lib()
    assert "56" in str(e.value) and "64" in str(e.value)
    monkeypatch.setattr(M._batch_lib, "ready", real)
    monkeypatch.setattr(M._filter_lib, "ready", filt)
    monkeypatch.setattr(M._insert_lib, "ready", insert)
    monkeypatch.setattr(M._range_data_lib, "ready", None)
    assert M._range_data_lib() is real


def test_package_exports_and_packing():
    import reflector_ekf_slam_amd as R
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd import map_builder as B
    assert R.RgridBatchRangeData is M.RgridBatchRangeData and R.FleetRangeDataResult is M.FleetRangeDataResult and R.FleetMapBuilder is B.FleetMapBuilder
    for name in ("pack_range_data", "add_range_data_packed_code", "add_range_data_code", "add_range_data", "last_call_counts"):
        assert callable(getattr(M.ScanMatchFleet, name)), name
    for name in ("AddRangeData", "ToSubmapTextures", "OccupancyGrids", "SaveMap", "submap_origin"):
        assert callable(getattr(B.FleetMapBuilder, name)), name
    ret = np.arange(6, dtype=np.float64).reshape(3, 2) + 0.1                       # converted to float32
    rds = [B.RangeData(np.array([0.3, -0.2]), ret, None), B.RangeData(np.zeros(2), np.zeros((0, 2)), [[1.0, 2.0]])]
    arr, count, keep = M.ScanMatchFleet.pack_range_data(rds, [(1.0, -2.0, 0.7), (0.0, 0.5, -2.9)], slots=[5, 2])
    assert count == 2 and (arr[0].grid, arr[0].n_returns, arr[0].n_misses) == (5, 3, 0)
    assert arr[0].returns_xy == keep[0].ctypes.data and keep[0].dtype == np.float32 and np.array_equal(keep[0], ret.astype(np.float32))
    assert arr[0].misses_xy is None and tuple(arr[0].origin_xy) == (np.float32(0.3), np.float32(-0.2)) and tuple(arr[0].ekf_pose) == (1.0, -2.0, 0.7)
    assert (arr[1].grid, arr[1].n_returns, arr[1].n_misses) == (2, 0, 1) and arr[1].returns_xy is None and arr[1].misses_xy == keep[3].ctypes.data
    assert keep[3].tolist() == [[1.0, 2.0]] and tuple(arr[1].ekf_pose) == (0.0, 0.5, -2.9)
    assert [s.grid for s in M.ScanMatchFleet.pack_range_data(rds, [(0, 0, 0)] * 2)[0]] == [0, 1]          # default: scan i into slot i
    assert M.ScanMatchFleet.pack_range_data([], [])[1] == 0
    with pytest.raises(ValueError):
        M.ScanMatchFleet.pack_range_data(rds, [(0, 0, 0)])
    # the options: the structure GridFrontEnd.AddRangeData hands to the single handle, field by field
    o = M._map_builder_options(MC.options(0.03, (0.9, 150.0, 100.0)))
    assert (o.resolution, o.voxel_filter_size) == (np.float32(0.03), np.float32(0.025))
    assert (o.adaptive_max_length, o.adaptive_min_num_points, o.adaptive_max_range) == (0.9, 150.0, 100.0)
    assert (o.match.linear_search_window, o.match.translation_delta_cost_weight, o.refine.occupied_space_weight, o.refine.max_num_iterations) == (0.2, 0.1, 1.0, 100)
    assert (o.hit_probability, o.miss_probability, o.insert_free_space) == (np.float32(0.55), np.float32(0.49), 1)
    assert M._map_builder_options(None).resolution == np.float32(0.05)


# ---- FleetMapBuilder over the CPU oracle ---------------------------------------------------------------------------------------------
class OracleFleet:
    """What FleetMapBuilder needs of a ScanMatchFleet, every slot a MapBuilder over a recorded OracleFrontEnd of its own: the stages are
    the oracle's, the composition is map_builder.py's.  TEST INFRASTRUCTURE."""

    def __init__(self, num_grids):
        self.num_grids, self.slots, self.calls = num_grids, {}, []

    def add_range_data_code(self, range_datas, ekf_poses, slots=None, options=None):
        from reflector_ekf_slam_amd.fleet_match import FleetRangeDataResult
        from reflector_ekf_slam_amd.map_builder import MapBuilder
        from tests.oracle_front_end import OracleFrontEnd
        slots = list(range(len(range_datas))) if slots is None else list(slots)
        assert len(set(slots)) == len(slots)                                       # a call names a slot once
        self.calls.append(slots)
        out = []
        for rd, pose, slot in zip(range_datas, ekf_poses, slots):
            if slot not in self.slots:
                rec = MC.Recorder(OracleFrontEnd())
                self.slots[slot] = (MapBuilder(options, front_end=rec), rec)
            mb, rec = self.slots[slot]
            first = len(rec.calls)
            result = mb.AddRangeData(None, rd, pose)
            insert = [c for c in rec.calls[first:] if c.name == "Insert"]
            status = 1 if np.asarray(rd.returns).shape[0] == 0 else (2 if result is None else 0)
            out.append(FleetRangeDataResult(0, status, np.zeros(3) if result is None else result.local_pose,
                                            tuple(insert[0].args[0]) if insert else (0.0, 0.0),
                                            np.zeros((0, 2), np.float32) if result is None else result.range_data_in_local.returns))
        return 0, out

    def GetLimits_code(self, slot):
        if slot in self.slots and self.slots[slot][1].state is not None:
            return 0, tuple(self.slots[slot][1].state[1])
        return -1, (0, 0, 0.0, 0.0, 0.0)

    def GetLimits(self, slot):
        return self.GetLimits_code(slot)[1]

    def GetGrid(self, slot):
        return self.slots[slot][1].state[0]

    def submap_textures(self, slots, origins):
        out = []
        for slot, (ox, oy) in zip(slots, origins):
            fe = self.slots[slot][1].inner
            cells, box, slice_max = fe.DrawTexture()
            out.append({"cells": cells, "width": box[2], "height": box[3], "resolution": fe.GetLimits()[2],
                        "slice_pose": (slice_max[0] - ox, slice_max[1] - oy), "global_pose": (ox, oy)})
        return out


def groups():
    """The chains by what a call has one of: (resolution, adaptive options)."""
    out = {}
    for ch in MC.chains():
        out.setdefault((ch.resolution, ch.adaptive), []).append(ch)
    return out


@pytest.fixture(scope="module")
def single(oracle_lib):
    """Every chain through a MapBuilder of its own over the oracle: [(result, num_range_data, grid and limits or None) per scan], the builder."""
    from reflector_ekf_slam_amd.map_builder import MapBuilder
    from tests.oracle_front_end import OracleFrontEnd
    out = {}
    for ch in MC.chains():
        mb, rows = MapBuilder(MC.options(ch.resolution, ch.adaptive), front_end=OracleFrontEnd()), []
        for t, scan in enumerate(ch.scans):
            result = mb.AddRangeData(float(t), scan.rd, scan.ekf_pose)
            rows.append((result, mb.num_range_data, mb.grid() if mb._have_submap else None))
        out[ch.name] = (rows, mb)
    return out


def test_chains_fall_into_five_groups_and_the_outcomes_chain_is_among_them():
    g = groups()
    assert len(g) == 5 and sum(len(v) for v in g.values()) == 8
    assert sorted(len(v) for v in g.values()) == [1, 1, 1, 1, 4]
    assert max(len(ch.scans) for ch in MC.chains()) == 6


def _same_result(got, want):
    if want is None:
        return got is None
    return (got is not None and got.time == want.time and got.local_pose.tobytes() == np.asarray(want.local_pose, np.float64).tobytes() and
            FC.same_cloud(got.range_data_in_local.returns, want.range_data_in_local.returns))


def test_fleet_map_builder_gives_on_every_chain_what_a_map_builder_per_robot_gives(single):
    from reflector_ekf_slam_amd.map_builder import FleetMapBuilder
    inserted = 0
    for (resolution, adaptive), chains in groups().items():
        fleet = OracleFleet(len(chains))
        fb = FleetMapBuilder(len(chains), MC.options(resolution, adaptive), fleet=fleet)
        assert fb.ToSubmapTextures() == [None] * len(chains) and fb.num_range_data == [0] * len(chains)
        for t in range(max(len(ch.scans) for ch in chains)):
            members = [m for m, ch in enumerate(chains) if t < len(ch.scans)]
            if t % 2:
                members.reverse()                                                  # the order of a call's scans is the caller's
            got = fb.AddRangeData([float(t)] * len(members), [chains[m].scans[t].rd for m in members], [chains[m].scans[t].ekf_pose for m in members], members)
            assert fleet.calls[-1] == members
            for m, g in zip(members, got):
                want, count, state = single[chains[m].name][0][t]
                assert _same_result(g, want), (chains[m].name, t)
                assert fb.num_range_data[m] == count, (chains[m].name, t)
                assert (fb.submap_origin(m) is None) == (state is None), (chains[m].name, t)
                if state is not None:
                    cells, limits = fb.grid(m)
                    assert tuple(limits) == tuple(state[1]) and np.array_equal(cells, state[0]), (chains[m].name, t)
                inserted += g is not None
        for m, (ch, tex) in enumerate(zip(chains, fb.ToSubmapTextures())):
            mb = single[ch.name][1]
            want = mb.ToSubmapTexture()
            assert fb.submap_origin(m) == mb._submap_origin and fb.num_range_data[m] == mb.num_range_data, ch.name
            assert set(tex) == set(want) and np.array_equal(tex["cells"], want["cells"]), ch.name
            assert all(tex[k] == want[k] for k in want if k != "cells"), ch.name
        only = fb.ToSubmapTextures([len(chains) - 1])
        assert len(only) == 1 and np.array_equal(only[0]["cells"], single[chains[-1].name][1].ToSubmapTexture()["cells"])
    assert inserted == sum(r[0] is not None for rows, _ in single.values() for r in rows) >= 20


def test_members_without_a_submap_and_bad_members():
    from reflector_ekf_slam_amd.map_builder import FleetMapBuilder, RangeData
    fleet = OracleFleet(3)
    fb = FleetMapBuilder(3, fleet=fleet)
    empty = RangeData(np.zeros(2, np.float32), np.zeros((0, 2), np.float32), np.ones((2, 2), np.float32))
    assert fb.AddRangeData([0.0], [empty], [(0.0, 0.0, 0.0)], [2]) == [None]
    assert fb.num_range_data == [0, 0, 0] and fb.submap_origin(2) is None and fb.ToSubmapTextures([2, 0]) == [None, None]
    assert fb.SaveMap(2, "unused") is None
    with pytest.raises(ValueError):
        fb.AddRangeData([0.0], [empty], [(0.0, 0.0, 0.0)], [3])
