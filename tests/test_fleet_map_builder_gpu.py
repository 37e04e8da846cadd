"""MapBuilder::AddRangeData for one scan of every robot in one call (rgrid_batch_add_range_data, ScanMatchFleet.add_range_data,
map_builder.FleetMapBuilder) against its specification, the single handle: every slot of a fleet has a GridFrontEnd of its own that is
fed the same scans through GridFrontEnd.AddRangeData (rgrid_add_range_data), and after every call the scan's code, status, pose bytes
and returned cloud and the slot's limits and cells are the handle's, bit for bit.  Nothing has a tolerance.  Shapes are
tests/map_chain_cases.py's (at most 400 returns, 30 misses, 6 scans a chain), except the kernel-edge counts."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import fleet_filter_scan_cases as FC
from tests import map_chain_cases as MC

pytestmark = pytest.mark.gpu

MAX_POINTS, MAX_CELLS = 512, 512 * 512
OK, INVALID, CAPACITY, BUFFER = 0, -1, -4, -5
DEFAULT = ("control", "quarter", "near_minus_pi", "beyond_pi")        # the chains with the default options


def _handle(max_points=MAX_POINTS, max_cells=MAX_CELLS):
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    return GridFrontEnd(max_points=max_points, max_cells=max_cells, max_candidates=1 << 16)


def _handle_state(fe):
    from reflector_ekf_slam_amd.grid import RgridError
    try:
        limits = fe.GetLimits()
    except RgridError:
        return None
    fe._grid_shape = (limits[1], limits[0])
    return fe.GetGrid(), tuple(limits)


def _slot_state(m, slot):
    rc, limits = m.GetLimits_code(slot)
    return None if rc != 0 else (m.GetGrid(slot), tuple(limits))


def _same_state(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a[1] == b[1] and np.array_equal(a[0], b[0]))


def _handle_add(fe, opt, rd, pose):
    """-> (code, status, pose, returns in local) of GridFrontEnd.AddRangeData."""
    from reflector_ekf_slam_amd.grid import RgridError
    try:
        status, local_pose, in_local = fe.AddRangeData(opt, rd.origin, rd.returns, rd.misses if rd.misses is not None and len(rd.misses) else None, pose)
    except RgridError as e:
        return e.code, None, None, None
    return OK, status, local_pose, in_local


class Rig:
    """A fleet and one handle per slot that sees the same scans."""

    def __init__(self, slots, opt, max_points=MAX_POINTS, max_cells=MAX_CELLS, handles=True):
        from reflector_ekf_slam_amd import fleet_match as M
        self.opt, self.slots = opt, slots
        self.m = M.ScanMatchFleet(max_scans=slots, max_points=max_points, num_grids=slots, max_cells=max_cells)
        self.fe = [_handle(max_points, max_cells) for _ in range(slots)] if handles else []
        self.matched = [0, 0]                                                      # scans through match and refine: the fleet's, the handles'

    def tick(self, entries, where=""):
        """entries = [(slot, RangeData, ekf_pose)]: one call of the fleet, one of every named handle; everything compared."""
        had = {slot: _slot_state(self.m, slot) is not None for slot, _, _ in entries}
        rc, results = self.m.add_range_data_code([e[1] for e in entries], [e[2] for e in entries], [e[0] for e in entries], self.opt)
        assert rc == OK and len(results) == len(entries), (where, rc)
        matched = 0
        for (slot, rd, pose), r in zip(entries, results):
            fe = self.fe[slot]
            handle_had = _handle_state(fe) is not None
            code, status, local_pose, in_local = _handle_add(fe, self.opt, rd, pose)
            assert r.code == code, (where, slot, r.code, code)
            if code == OK:
                assert r.status == status, (where, slot, r.status, status)
            if code == OK and status == 0:
                assert r.local_pose.tobytes() == local_pose.tobytes(), (where, slot, r.local_pose - local_pose)
                assert FC.same_cloud(r.returns_in_local, in_local), (where, slot)
                matched += had[slot]
                self.matched[1] += handle_had
            else:
                assert r.status != 0 and not r.returns_in_local.any(), (where, slot)   # rows of a scan that was not inserted: untouched
            assert _same_state(_slot_state(self.m, slot), _handle_state(fe)), (where, slot)
        self.matched[0] += matched
        launches, syncs = self.m.last_call_counts()
        assert (launches >= 5) == (matched > 0) and syncs <= 3, (where, launches, syncs, matched)   # the match and the refinement ran iff a scan needed them
        return results

    def close(self):
        self.m.close()
        for fe in self.fe:
            fe.close()


def _groups():
    out = {}
    for ch in MC.chains():
        out.setdefault((ch.resolution, ch.adaptive), []).append(ch)
    return out


def test_every_chain_against_its_handle():
    """One fleet per (resolution, adaptive options), one slot per chain, none of them set: tick t is ONE call with scan t of every chain
    that still has one.  Covers slot creation, the f / e outcomes (the slot stays unchanged, or absent), sensor origins, yaws beyond pi."""
    groups = _groups()
    assert len(groups) == 5
    matched = [0, 0]
    for (resolution, adaptive), chains in groups.items():
        rig = Rig(len(chains), MC.options(resolution, adaptive))
        for t in range(max(len(ch.scans) for ch in chains)):
            entries = [(k, ch.scans[t].rd, ch.scans[t].ekf_pose) for k, ch in enumerate(chains) if t < len(ch.scans)]
            results = rig.tick(entries, (chains[0].name, t))
            for (k, _, _), r in zip(entries, results):
                kind = chains[k].scans[t].kind
                assert r.code == OK and r.status == {"s": 0, "n": 0, "e": 1, "f": 2}[kind], (chains[k].name, t)
        matched = [a + b for a, b in zip(matched, rig.matched)]
        rig.close()
    assert matched[0] == matched[1] >= 12                                          # what tests/test_map_chain_gpu.py asserts for the same chains


def test_mixed_ticks_and_position_independence():
    """Member j starts at tick j: one call holds members that create their slot, members that are matched and absent members; the
    members are listed in reversed order on odd ticks."""
    chains = [ch for ch in MC.chains() if ch.name in DEFAULT]
    assert len(chains) == 4
    rig = Rig(len(chains), MC.options())
    kinds = set()
    for t in range(max(j + len(ch.scans) for j, ch in enumerate(chains))):
        entries = [(j, ch.scans[t - j].rd, ch.scans[t - j].ekf_pose) for j, ch in enumerate(chains) if 0 <= t - j < len(ch.scans)]
        if t % 2:
            entries.reverse()
        creating = sum(_slot_state(rig.m, slot) is None for slot, _, _ in entries)
        kinds.add((creating > 0, creating < len(entries), len(entries) < len(chains)))
        rig.tick(entries, ("mixed", t))
    assert (True, True, True) in kinds                                             # creation, matching and an absent member in one call
    assert rig.matched[0] == rig.matched[1] == sum(len(ch.scans) - 1 for ch in chains)
    rig.close()


EDGE_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 8192)      # both sides of the wave (64), kgb_to_local's workgroup (256 = 1024 / 4) and the filter's stride (1024)
EDGE_MISSES = (0, 1, 1, 0, 1, 0, 1, 0)


def _edge_scans(tick):
    from reflector_ekf_slam_amd.map_builder import RangeData
    rng = np.random.default_rng(3100 + tick)
    out = []
    for j, (n, nm) in enumerate(zip(EDGE_COUNTS, EDGE_MISSES)):
        ret = FC.cloud(np.random.default_rng(3200 + j), n)                         # the same scene every tick, seen from a pose that moves
        pose = (0.1 * j + 0.02 * tick, -0.05 * j, 0.3 * j + 0.01 * tick)
        if n == 65:                                                                # signed zeros, and a pose that leaves them alone
            ret[:3] = np.array([[-0.0, 0.5], [0.25, -0.0], [-0.0, -0.0]], np.float32)
            pose = (0.0, 0.0, 0.0)
        mis = rng.uniform(-2.0, 2.0, (nm, 2)).astype(np.float32)
        out.append((RangeData(np.array([0.05 * j, 0.0], np.float32), ret, mis), pose))
    return out


def test_kernel_edges_of_the_new_device_code():
    """One call of scans whose return counts sit on both sides of the rotating load's and kgb_to_local's strides; then the same
    scans in reverse order (their slots have grids now: they are matched), then each scan alone."""
    from reflector_ekf_slam_amd import fleet_match as M
    assert EDGE_COUNTS[-1] == min(8192, M.filter_max_points()) and set(EDGE_MISSES) == {0, 1}
    rig = Rig(len(EDGE_COUNTS), MC.options(), max_points=8192)
    first = _edge_scans(0)
    assert any(np.signbit(rd.returns).any() and (rd.returns == 0).any() for rd, _ in first)
    rig.tick([(j, rd, pose) for j, (rd, pose) in enumerate(first)], "edges")
    assert rig.matched == [0, 0]
    rig.tick([(j, rd, pose) for j, (rd, pose) in enumerate(_edge_scans(1))][::-1], "edges reversed")
    assert rig.matched[0] == rig.matched[1] == len(EDGE_COUNTS)
    for j, (rd, pose) in enumerate(_edge_scans(2)):
        rig.tick([(j, rd, pose)], ("edge alone", j))
    assert rig.matched[0] == rig.matched[1] == 2 * len(EDGE_COUNTS)
    rig.close()


def _all_states(rig):
    return [_slot_state(rig.m, k) for k in range(rig.slots)]


def test_statuses_and_refusals():
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.map_builder import RangeData
    chains = {ch.name: ch for ch in MC.chains()}
    control, quarter = chains["control"], chains["quarter"]
    opt = MC.options()
    rig = Rig(4, opt)
    m, L = rig.m, M._range_data_lib()
    rig.tick([(0, control.scans[0].rd, control.scans[0].ekf_pose), (2, quarter.scans[0].rd, quarter.scans[0].ekf_pose)], "before the refusals")
    before, counts = _all_states(rig), m.last_call_counts()
    rd, pose = control.scans[1].rd, control.scans[1].ekf_pose

    def refused(want, *args, **kw):
        rc, results = m.add_range_data_packed_code(*args, **kw)
        assert rc == want and results == [], (rc, want)
        assert all(_same_state(a, b) for a, b in zip(before, _all_states(rig))) and m.last_call_counts() == counts

    pack = M.ScanMatchFleet.pack_range_data
    # ---- the whole call: null pointers (the raw call: the wrapper always passes its own)
    arr, count, keep = pack([rd], [pose], [0])
    co = M._map_builder_options(opt)
    out = [np.zeros(16, np.float64) for _ in range(5)]
    good = [m._h, C.byref(co), C.cast(arr, C.c_void_p), count] + [o.ctypes.data for o in out[:4]]
    for k in (0, 1, 2, 4, 5, 6, 7):
        args = list(good)
        args[k] = None
        assert L.rgrid_batch_add_range_data(*args, None, 0) == INVALID, k
    # ---- count outside [0, max_scans], a slot out of range, a negative count, a null pointer with a positive count, a slot twice
    five = pack([rd] * 5, [pose] * 5, [0, 1, 2, 3, 0])
    refused(INVALID, five, opt)
    refused(INVALID, (arr, -1, keep), opt)
    for slot in (-1, 4):
        refused(INVALID, pack([rd], [pose], [slot]), opt)
    for field, value in (("n_returns", -1), ("n_misses", -1), ("returns_xy", None), ("misses_xy", None)):
        bad = pack([rd], [pose], [0])
        assert bad[0][0].n_misses > 0
        setattr(bad[0][0], field, value)
        refused(INVALID, bad, opt)
    refused(INVALID, pack([rd, rd], [pose, pose], [1, 1]), opt)
    # ---- options the filter, the refinement or the insert refuse
    R = dataclasses.replace
    for bad_opt in (R(opt, voxel_filter_size=0.0), R(opt, adaptive_voxel_options=R(opt.adaptive_voxel_options, max_length=0.0)),
                    R(opt, ceres_scan_matcher_options=R(opt.ceres_scan_matcher_options, rotation_weight=0.0)),
                    R(opt, ceres_scan_matcher_options=R(opt.ceres_scan_matcher_options, max_num_iterations=-1)),
                    R(opt, range_data_inserter_options=R(opt.range_data_inserter_options, hit_probability=1.0)),
                    R(opt, range_data_inserter_options=R(opt.range_data_inserter_options, miss_probability=0.0))):
        refused(INVALID, pack([rd], [pose], [0]), bad_opt)
    # ---- too little room for the returns: nothing is launched
    refused(BUFFER, pack([rd, quarter.scans[1].rd], [pose, quarter.scans[1].ekf_pose], [0, 2]), opt, cap_points=rd.returns.shape[0] + quarter.scans[1].rd.returns.shape[0] - 1)
    # ---- a pending submit of any kind stays pending
    m.submit_filter([(rd.returns, rd.misses)])
    assert m.add_range_data_packed_code(pack([rd], [pose], [0]), opt) == (INVALID, [])
    assert len(m.collect_filter()) == 1
    m.submit_texture([0])
    assert m.add_range_data_packed_code(pack([rd], [pose], [0]), opt) == (INVALID, [])
    assert len(m.collect_texture()) == 1
    refused(INVALID, pack([rd], [pose], [4]), opt)                                 # (and the slots are as they were)
    # ---- a following valid call gives the right bits; enough room exactly is enough
    rig.tick([(0, rd, pose), (2, quarter.scans[1].rd, quarter.scans[1].ekf_pose), (3, chains["beyond_pi"].scans[0].rd, chains["beyond_pi"].scans[0].ekf_pose)],
             "after the refusals")
    assert rig.matched[0] == rig.matched[1] == 2
    # ---- per scan: a cloud above the cap, a NaN return; the neighbours are the handles'
    big = RangeData(rd.origin, FC.cloud(np.random.default_rng(7), MAX_POINTS + 1), rd.misses)
    big_misses = RangeData(rd.origin, rd.returns, FC.cloud(np.random.default_rng(8), MAX_POINTS + 1))
    nan = RangeData(rd.origin, rd.returns.copy(), rd.misses)
    nan.returns[17, 1] = np.nan
    states = _all_states(rig)
    results = rig.tick([(1, big, pose), (0, control.scans[2].rd, control.scans[2].ekf_pose), (3, big_misses, pose)], "capacity")
    assert [r.code for r in results] == [CAPACITY, OK, CAPACITY] and results[1].status == 0
    assert _slot_state(m, 1) is None and _same_state(_slot_state(m, 3), states[3])
    rc, results = m.add_range_data_code([nan, quarter.scans[2].rd], [pose, quarter.scans[2].ekf_pose], [0, 2], opt)
    assert rc == OK and [r.code for r in results] == [INVALID, OK] and results[0].status != 0 and results[1].status == 0
    code, status, local_pose, in_local = _handle_add(rig.fe[2], opt, quarter.scans[2].rd, quarter.scans[2].ekf_pose)
    assert (code, status) == (OK, 0) and results[1].local_pose.tobytes() == local_pose.tobytes() and FC.same_cloud(results[1].returns_in_local, in_local)
    assert _same_state(_slot_state(m, 2), _handle_state(rig.fe[2])) and _same_state(_slot_state(m, 0), _handle_state(rig.fe[0]))
    rig.close()
    # ---- max_cells below the 100 x 100 cells of a new submap: the scan that would create it, not the ones that create nothing
    outcomes = chains["outcomes"]
    small = Rig(3, MC.options(outcomes.resolution, outcomes.adaptive), max_cells=9999)
    results = small.tick([(0, outcomes.scans[0].rd, outcomes.scans[0].ekf_pose), (1, outcomes.scans[2].rd, outcomes.scans[2].ekf_pose),
                          (2, outcomes.scans[1].rd, outcomes.scans[1].ekf_pose)], "max_cells")
    assert [(r.code, r.status) for r in results] == [(OK, 2), (CAPACITY, 2), (OK, 1)] and _all_states(small) == [None, None, None]
    small.close()


def test_budget_does_not_depend_on_the_number_of_scans():
    """Ticks of the same kind -- every scan creates its slot, every scan is matched -- at count 1 and count 8, in both reduction modes."""
    from reflector_ekf_slam_amd import fleet_match as M
    control = [ch for ch in MC.chains() if ch.name == "control"][0]
    opt = MC.options()
    one, eight, launch = Rig(1, opt), Rig(8, opt, handles=False), Rig(8, opt, handles=False)
    launch.m.set_reduction(M.REDUCE_LAUNCH)
    assert one.m.last_call_counts() == (0, 0)
    for t, scan in enumerate(control.scans):
        want = one.tick([(0, scan.rd, scan.ekf_pose)], ("budget", t))[0]
        counts = one.m.last_call_counts()
        assert counts == ((3, 2) if t == 0 else (5, 3))                            # filter, insert, to_local; with match and refine behind the filter
        for rig, extra in ((eight, 0), (launch, 1 if t else 0)):
            rc, results = rig.m.add_range_data_code([scan.rd] * 8, [scan.ekf_pose] * 8, range(8), opt)
            assert rc == OK and rig.m.last_call_counts() == (counts[0] + extra, counts[1])
            assert rig.m.last_call_counts()[0] <= 5 + extra and rig.m.last_call_counts()[1] <= 3
            state = _slot_state(one.m, 0)
            for k, r in enumerate(results):
                assert (r.code, r.status) == (want.code, want.status) and r.local_pose.tobytes() == want.local_pose.tobytes()
                assert FC.same_cloud(r.returns_in_local, want.returns_in_local) and _same_state(_slot_state(rig.m, k), state), (t, k)
    assert one.m.add_range_data_code([], [], [], opt) == (OK, []) and one.m.last_call_counts() == (0, 0)
    for rig in (one, eight, launch):
        rig.close()


def test_the_way_out_uses_the_kept_submap_origins(tmp_path):
    """After a chain, FleetMapBuilder's occupancy grids and saved maps are, byte for byte, those of a MapBuilder over a handle that saw
    the same scans: the origins kept from the call are the submaps'."""
    from reflector_ekf_slam_amd.grid import IMAGE, OCCUPANCY
    from reflector_ekf_slam_amd.map_builder import FleetMapBuilder, MapBuilder
    chains = [ch for ch in MC.chains() if ch.name in DEFAULT]
    fb = FleetMapBuilder(len(chains), MC.options(), max_points=MAX_POINTS, max_cells=MAX_CELLS)
    singles = [MapBuilder(MC.options(), front_end=_handle()) for _ in chains]
    assert fb.OccupancyGrids() == [None] * len(chains)
    for t in range(max(len(ch.scans) for ch in chains)):
        members = [m for m, ch in enumerate(chains) if t < len(ch.scans)]
        got = fb.AddRangeData([float(t)] * len(members), [chains[m].scans[t].rd for m in members], [chains[m].scans[t].ekf_pose for m in members], members)
        for m, g in zip(members, got):
            want = singles[m].AddRangeData(float(t), chains[m].scans[t].rd, chains[m].scans[t].ekf_pose)
            assert g.time == want.time and g.local_pose.tobytes() == want.local_pose.tobytes()
            assert FC.same_cloud(g.range_data_in_local.returns, want.range_data_in_local.returns)
    assert len({fb.submap_origin(m) for m in range(len(chains))}) > 1 and any(o != (0.0, 0.0) for o in fb._submap_origin)
    for mode in (OCCUPANCY, IMAGE):
        for m, got in enumerate(fb.OccupancyGrids(mode=mode)):
            want = singles[m].OccupancyGrid(mode)
            assert fb.submap_origin(m) == singles[m]._submap_origin and fb.num_range_data[m] == singles[m].num_range_data
            assert got.status == OK and got.data.dtype == want.data.dtype and np.array_equal(got.data, want.data), (mode, m)
            assert (got.resolution, got.origin, got.box) == (want.resolution, want.origin, want.box), (mode, m)
    for m, tex in enumerate(fb.ToSubmapTextures()):
        want = singles[m].ToSubmapTexture()
        assert np.array_equal(tex["cells"], want["cells"]) and all(tex[k] == want[k] for k in want if k != "cells"), m
    base = str(tmp_path / "map")
    for m in (1, 3):
        files = fb.SaveMap(m, base)
        mine = [open(f, "rb").read() for f in files]
        assert singles[m].SaveMap(base) == files
        assert mine == [open(f, "rb").read() for f in files] and mine[0].startswith(b"P5\n"), m
    fb._fleet.close()
    for s in singles:
        s._fe.close()
