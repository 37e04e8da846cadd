"""MapBuilder::AddRangeData's composition on the GPU (tests/map_chain_cases.py): (1) reflector_ekf_slam_amd.map_builder.MapBuilder over a
recorded GridFrontEnd, every decision held to tests/witness/map_builder_witness.py and every stage result to its stage witness on the
recorded inputs; (2) GridFrontEnd.AddRangeData, the C entry point, bit-identical to that Python builder on every chain -- status,
pose, returned cloud, grid and limits, the empty outcomes and the sensor origins included; (3) the recorded stage inputs of every
chain's last scan through ScanMatchFleet.filter, scan_match and insert, one slot per chain, bit-identical to what the handle
recorded.  The tests compose nothing themselves: they feed recorded inputs."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fleet_filter_scan_cases as FC
from tests import fleet_match_cases as FM
from tests import fleet_refine_cases as FR
from tests import map_chain_cases as MC

pytestmark = pytest.mark.gpu

MAX_POINTS, MAX_CELLS = 512, 512 * 512


def _front_end():
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    return GridFrontEnd(max_points=MAX_POINTS, max_cells=MAX_CELLS, max_candidates=1 << 16)


@pytest.fixture(scope="module")
def recorded():
    out = {}
    for ch in MC.chains():
        fe = _front_end()
        out[ch.name] = (ch, MC.run_chain(ch, fe))
        fe.close()
    return out


def test_every_decision_and_every_stage_of_every_scan_holds_on_the_handle(recorded):
    matched = 0
    for name, (ch, recs) in recorded.items():
        for k, rec in enumerate(recs):
            comp = MC.composition(rec, ch)
            st, fig = MC.stages(("gpu", name, k), rec, ch, factor=MC.GPU_FACTOR)
            assert MC.holds(comp) == [] and MC.holds(st) == [], (name, k, MC.holds(comp), MC.holds(st), fig)
            matched += fig.refine is not None
            if rec.state_after is not None:
                assert max(rec.state_after[1][:2]) <= 400
    assert matched >= 12


def test_c_entry_point_is_bit_identical_to_the_python_builder_on_every_chain(recorded):
    for name, (ch, recs) in recorded.items():
        fe = _front_end()
        opt = MC.options(ch.resolution, ch.adaptive)
        for k, rec in enumerate(recs):
            rd = rec.scan.rd
            status, pose, in_local = fe.AddRangeData(opt, rd.origin, rd.returns, rd.misses if rd.misses.shape[0] else None, rec.scan.ekf_pose)
            want = 1 if rd.returns.shape[0] == 0 else (2 if rec.result is None else 0)
            assert status == want, (name, k, status)
            if rec.result is not None:
                assert pose.tobytes() == np.asarray(rec.result.local_pose, np.float64).tobytes(), (name, k, pose - rec.result.local_pose)
                assert FC.same_cloud(in_local, rec.result.range_data_in_local.returns), (name, k)
            if rec.state_after is not None:                                        # unchanged by the empty outcomes, too
                assert tuple(fe.GetLimits()) == rec.state_after[1], (name, k)
                fe._grid_shape = (rec.state_after[1][1], rec.state_after[1][0])
                assert np.array_equal(fe.GetGrid(), rec.state_after[0]), (name, k)
        fe.close()


def test_fleet_stages_are_bit_identical_on_the_recorded_inputs_of_every_last_scan(recorded):
    """filter is one call per set of filter options (a call has one set), scan_match and insert one call each."""
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import AdaptiveVoxelFilterOptions
    last = [(ch, recs[-1]) for ch, recs in recorded.values()]
    assert all("Match" in rec.calls for _, rec in last)
    m = M.ScanMatchFleet(max_scans=len(last), max_points=MAX_POINTS, num_grids=len(last), max_cells=MAX_CELLS)
    groups = {}
    for slot, (ch, rec) in enumerate(last):
        groups.setdefault(ch.adaptive, []).append(rec)
        cells, (nx, ny, res, mx, my) = rec.calls["Match"].before
        m.SetGrid(slot, cells, res, (mx, my))
    assert len(groups) == 3
    for adaptive, recs in groups.items():
        got = m.filter([(r.calls["VoxelFilter"].args[0], r.calls["VoxelFilter2"].args[0]) for r in recs], 0.025, AdaptiveVoxelFilterOptions(*adaptive))
        for r, g in zip(recs, got):
            want = (r.calls["VoxelFilter"].result, r.calls["VoxelFilter2"].result, r.calls["AdaptiveVoxelFilter"].result)
            assert g.status == FC.OK and FC.same_result(g, want), adaptive
    opt = MC.options()
    got = m.scan_match([(slot, rec.calls["Match"].args[0], rec.calls["Match"].args[1]) for slot, (_, rec) in enumerate(last)],
                       opt.real_time_scan_matcher_options, opt.ceres_scan_matcher_options)
    for (ch, rec), g in zip(last, got):
        assert g.status == FC.OK and FM.same_bits(g.coarse, rec.calls["Match"].result), ch.name
        assert FR.same_refine_bits(g.fine, rec.calls["RefineMatch"].result), ch.name
    codes = m.insert([(slot,) + tuple(rec.calls["Insert"].args[:3]) for slot, (_, rec) in enumerate(last)], opt.range_data_inserter_options)
    assert codes == [FC.OK] * len(last)
    for slot, (ch, rec) in enumerate(last):
        assert tuple(m.GetLimits(slot)) == rec.calls["Insert"].after[1], ch.name
        assert np.array_equal(m.GetGrid(slot), rec.calls["Insert"].after[0]), ch.name
    m.close()
