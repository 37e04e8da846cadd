"""The occupancy grid and the saved map on the GPU (rgrid_occupancy_grid, rgrid_batch_occupancy_* of include/rgrid.h): the cases of
tests/occupancy_cases.py through GridFrontEnd.OccupancyGrid and ScanMatchFleet.occupancy_grids, in both modes, against the witness
fed with the oracle's texture (tests/witness/occupancy_witness.py, pinned against libcairo by tests/test_occupancy_cpu.py) and
against each other.  Every comparison is exact."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fleet_texture_cases as TC
from tests import occupancy_cases as OC
from tests.witness import occupancy_witness as W

pytestmark = pytest.mark.gpu
MODES = (OC.OCCUPANCY, OC.IMAGE)


@pytest.fixture(scope="module")
def M():
    from reflector_ekf_slam_amd import fleet_match
    return fleet_match


@pytest.fixture(scope="module")
def want(oracle_lib):
    """The witness's answer for every case, computed once: {(family, index, mode): (data, origin, box) or None}."""
    out = {}
    families = {"sweep": OC.sweep_case(), "edge": OC.edge_cases(), "quirk": OC.quirk_cases(), "far": [OC.out_of_domain_case()],
                "replay": [OC.replay_case()]}
    for name, cases in families.items():
        for k, case in enumerate(cases):
            for mode in MODES:
                out[name, k, mode] = OC.expected(case, mode)
    return out


def _fleet(M, cases, max_cells, max_scans=None):
    fleet = M.ScanMatchFleet(max_scans=max_scans or len(cases), max_points=64, num_grids=len(cases), max_cells=max_cells, max_rotations=8)
    for k, (grid, _) in enumerate(cases):
        fleet.SetGrid(k, *grid)
    return fleet


@pytest.fixture(scope="module")
def sweep_fleet(M, oracle_lib):
    return _fleet(M, OC.sweep_case(), TC.SWEEP_MAX_CELLS, max_scans=24)


@pytest.fixture(scope="module")
def edge_fleet(M, oracle_lib):
    return _fleet(M, OC.edge_cases() + OC.quirk_cases() + [OC.out_of_domain_case(), OC.replay_case()], OC.EDGE_MAX_CELLS)


def _single(case, mode):
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    grid, origin = case
    fe = GridFrontEnd(max_points=64, max_cells=max(grid[0].size, 64), max_candidates=64)
    fe.SetGrid(*grid)
    return fe.OccupancyGrid(origin, mode)


@pytest.mark.parametrize("mode", MODES)
def test_sweep_in_any_order_alone_and_repeated(M, sweep_fleet, want, mode):
    cases = OC.sweep_case()
    origins = [o for _, o in cases]
    for order in (list(range(8)), [7, 3, 0, 5, 1, 6, 2, 4], [4], [7, 7, 1, 7], [2, 0, 2]):
        got = sweep_fleet.occupancy_grids(order, [origins[k] for k in order], mode)
        assert len(got) == len(order)
        for g, k in zip(got, order):
            assert g.status == 0 and OC.same(g, want["sweep", k, mode]), (order, k)
            assert g.resolution == cases[k][0][1]


@pytest.mark.parametrize("mode", MODES)
def test_sweep_single_handle_equals_witness_and_fleet(M, sweep_fleet, want, mode):
    cases = OC.sweep_case()
    fleet = sweep_fleet.occupancy_grids(range(8), [o for _, o in cases], mode)
    for k, case in enumerate(cases):
        one = _single(case, mode)
        assert OC.same(one, want["sweep", k, mode]), k
        assert OC.same(fleet[k], (one.data, one.origin, one.box)) and fleet[k].resolution == one.resolution, k


@pytest.mark.parametrize("mode", MODES)
def test_edge_boxes_strides_long_rows_and_quirks(M, edge_fleet, want, mode):
    edges, quirks = OC.edge_cases(), OC.quirk_cases()
    cases = edges + quirks
    got = edge_fleet.occupancy_grids(range(len(cases)), [o for _, o in cases], mode)
    for k, g in enumerate(got):
        key = ("edge", k, mode) if k < len(edges) else ("quirk", k - len(edges), mode)
        assert g.status == 0 and OC.same(g, want[key]), key
    for form, g in zip(OC.QUIRK_FORMS, got[len(edges):]):                           # the quirk row / column is there
        assert (g.width - g.box[3] - 10, g.height - g.box[2] - 10) == form


def test_edge_boxes_through_the_single_handle(want):
    edges = OC.edge_cases()
    picks = [k for k, (w, h) in enumerate(OC.EDGE_BOXES + OC.STRIDE_BOXES + OC.LONG_BOXES) if (w, h) in
             ((1, 1), (OC.T + 1, 2 * OC.T + 1), (2 * OC.T + 1, 1), (1, OC.T), (5, 15), (5, 16), (5, 17), OC.LONG_BOXES[0], OC.LONG_BOXES[1])]
    assert len(picks) == 9
    for k in picks:
        for mode in MODES:
            assert OC.same(_single(edges[k], mode), want["edge", k, mode]), (k, mode)
    for k, case in enumerate(OC.quirk_cases()):
        assert OC.same(_single(case, OC.IMAGE), want["quirk", k, OC.IMAGE]), k


def test_out_of_domain_slot_is_refused_alone(M, edge_fleet, want):
    from reflector_ekf_slam_amd.grid import RgridError
    edges, quirks, far = OC.edge_cases(), OC.quirk_cases(), OC.out_of_domain_case()
    slot = len(edges) + len(quirks)
    assert want["far", 0, OC.OCCUPANCY] is None
    order = [3, slot, len(edges), slot, 20]
    cases = edges + quirks + [far]
    got = edge_fleet.occupancy_grids(order, [cases[k][1] for k in order], OC.OCCUPANCY)
    for g, k in zip(got, order):
        if k == slot:
            assert g.status == M.RGRID_ERR_CAPACITY and g.data.size == 0 and g.origin == (0.0, 0.0)
            assert g.box == TC.oracle_texture(far[0])[1]
        else:
            key = ("edge", k, OC.OCCUPANCY) if k < len(edges) else ("quirk", k - len(edges), OC.OCCUPANCY)
            assert g.status == 0 and OC.same(g, want[key]), k
    with pytest.raises(RgridError) as e:
        _single(far, OC.OCCUPANCY)
    assert e.value.code == M.RGRID_ERR_CAPACITY


@pytest.mark.parametrize("mode", MODES)
def test_translation_is_replayed_not_taken_from_slice_max(M, edge_fleet, want, mode):
    """A grid for which t = slice_max in place of (slice_max - o) + o gives another origin (tests/occupancy_cases.replay_case)."""
    case = OC.replay_case()
    slot = len(OC.edge_cases()) + len(OC.quirk_cases()) + 1
    got = edge_fleet.occupancy_grids([slot], [case[1]], mode)[0]
    assert got.status == 0 and OC.same(got, want["replay", 0, mode])
    assert OC.same(_single(case, mode), want["replay", 0, mode])
    tex = TC.oracle_texture(case[0])
    wrong = W.occupancy(W.paint(tex, case[0][1], case[1], "slice_max"), case[0][1])[1]
    assert tuple(got.origin) != wrong


def test_garbage_behind_a_slot_is_not_read(M, oracle_lib):
    garbage, grid = TC.multi_pass_case()
    fleet = M.ScanMatchFleet(max_scans=2, max_points=64, num_grids=TC.MULTI_SLOT + 1, max_cells=TC.MULTI_MAX_CELLS, max_rotations=8)
    fleet.SetGrid(TC.MULTI_SLOT, *garbage)
    fleet.SetGrid(TC.MULTI_SLOT, *grid)
    origin = (float(np.float32(0.2)), float(np.float32(-0.4)))
    for mode in MODES:
        got = fleet.occupancy_grids([TC.MULTI_SLOT], [origin], mode)[0]
        assert got.box == (7, 10, 244, 191) and OC.same(got, OC.expected((grid, origin), mode)), mode


def test_buffer_protocol_leaves_the_submit_pending(M, sweep_fleet, want):
    cases = OC.sweep_case()
    order = [0, 7, 4]
    origins = [cases[k][1] for k in order]
    sweep_fleet.submit_occupancy(order, origins, OC.IMAGE)
    need = sum(want["sweep", k, OC.IMAGE][0].size for k in order)
    rc, info = sweep_fleet.collect_occupancy_code(cap=need - 1)
    assert rc == M.RGRID_ERR_BUFFER and sweep_fleet._pending == 3
    at = 0
    for (status, size, origin, box, offset), k in zip(info, order):
        data, o, b = want["sweep", k, OC.IMAGE]
        assert status == 0 and size == (data.shape[1], data.shape[0]) and origin == o and box == b and offset == at
        at += data.size
    assert sweep_fleet.submit_occupancy_code(order, origins) == M.RGRID_ERR_INVALID       # one pending submit at a time
    assert sweep_fleet.submit_texture_code(order) == M.RGRID_ERR_INVALID
    rc, got = sweep_fleet.collect_occupancy_code(cap=need)
    assert rc == 0 and sweep_fleet._pending is None
    for g, k in zip(got, order):
        assert OC.same(g, want["sweep", k, OC.IMAGE]), k
    assert sweep_fleet.collect_occupancy_code()[0] == M.RGRID_ERR_INVALID


def test_refusals_launch_nothing_and_leave_the_handle_usable(M, sweep_fleet, want):
    cases = OC.sweep_case()
    o = [cases[0][1]]
    L = M._occupancy_lib()
    ids = np.array([0], np.int32)
    org = np.array(o, np.float64)
    assert sweep_fleet.submit_occupancy_code([0], o, 2) == M.RGRID_ERR_INVALID             # another mode
    assert sweep_fleet.submit_occupancy_code([0], o, -1) == M.RGRID_ERR_INVALID
    assert sweep_fleet.submit_occupancy_code([8], o) == M.RGRID_ERR_INVALID                # a slot out of range
    assert sweep_fleet.submit_occupancy_code([-1], o) == M.RGRID_ERR_INVALID
    assert sweep_fleet.submit_occupancy_code(list(range(8)) * 4, [cases[k][1] for k in range(8)] * 4) == M.RGRID_ERR_INVALID   # count > max_scans
    assert L.rgrid_batch_occupancy_submit(sweep_fleet._h, 0, None, org.ctypes.data, 1) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_occupancy_submit(sweep_fleet._h, 0, ids.ctypes.data, None, 1) == M.RGRID_ERR_INVALID
    assert sweep_fleet._pending is None and sweep_fleet.collect_occupancy_code()[0] == M.RGRID_ERR_INVALID
    unset = M.ScanMatchFleet(max_scans=2, max_points=64, num_grids=2, max_cells=64, max_rotations=8)
    assert unset.submit_occupancy_code([1], o) == M.RGRID_ERR_INVALID                      # a slot not yet set
    assert sweep_fleet.submit_occupancy_code([], []) == 0 and sweep_fleet.collect_occupancy() == []      # count == 0: a submit, nothing launched
    got = sweep_fleet.occupancy_grids([0], o)
    assert OC.same(got[0], want["sweep", 0, OC.OCCUPANCY])


def test_texture_and_occupancy_submits_exclude_each_other(M, sweep_fleet, want):
    cases = OC.sweep_case()
    sweep_fleet.submit_texture([1, 2])
    assert sweep_fleet.submit_occupancy_code([1], [cases[1][1]]) == M.RGRID_ERR_INVALID
    assert sweep_fleet.collect_occupancy_code()[0] == M.RGRID_ERR_INVALID                  # another kind: the texture stays pending
    tex = sweep_fleet.collect_texture()
    assert TC.same_texture(tex[0], TC.oracle_texture(cases[1][0])) and TC.same_texture(tex[1], TC.oracle_texture(cases[2][0]))
    sweep_fleet.submit_occupancy([1], [cases[1][1]])
    assert sweep_fleet.submit_texture_code([1]) == M.RGRID_ERR_INVALID
    assert sweep_fleet.collect_texture_code()[0] == M.RGRID_ERR_INVALID
    assert OC.same(sweep_fleet.collect_occupancy()[0], want["sweep", 1, OC.OCCUPANCY])


def test_textures_and_slots_are_unchanged_by_the_occupancy_call(M, sweep_fleet):
    cases = OC.sweep_case()
    before = sweep_fleet.draw_textures(range(8))
    sweep_fleet.occupancy_grids(range(8), [o for _, o in cases], OC.OCCUPANCY)
    sweep_fleet.occupancy_grids([7, 0], [cases[7][1], cases[0][1]], OC.IMAGE)
    after = sweep_fleet.draw_textures(range(8))
    for k, (grid, _) in enumerate(cases):
        assert TC.same_texture(before[k], TC.oracle_texture(grid)) and TC.same_texture(after[k], before[k]), k
        assert np.array_equal(sweep_fleet.GetGrid(k), grid[0]) and sweep_fleet.GetLimits(k) == (grid[0].shape[1], grid[0].shape[0], grid[1], *grid[2])


def test_map_builder_publishes_and_saves_what_the_fleet_and_the_witness_give(M, oracle_lib, tmp_path):
    """The texture tests' submap scene through MapBuilder's write path (three inserts, the submap grows), then PublishMap and
    HandleSaveMap; the same scans through the fleet's inserter give the same grids."""
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    from reflector_ekf_slam_amd.map_builder import MapBuilder, RangeData
    builder = MapBuilder(front_end=GridFrontEnd(max_points=1024, max_cells=TC.SUBMAP_MAX_CELLS, max_candidates=1 << 16))
    n, res = TC.SUBMAP_N, float(np.float32(TC.SUBMAP_RES))
    scans = TC.submap_scene()
    origin = scans[0][0]
    fleet = M.ScanMatchFleet(max_scans=2, max_points=1024, num_grids=2, max_cells=TC.SUBMAP_MAX_CELLS, max_rotations=8)
    fleet.SetGrid(1, np.zeros((n, n), np.uint16), res, (float(origin[0]) + 0.5 * n * res, float(origin[1]) + 0.5 * n * res))
    for org, ret, mis in scans:
        builder.InsertIntoSubmap(RangeData(org, ret, mis))
        assert [int(s) for s in fleet.insert([(1, org, ret, mis)])] == [0]
    cells, limits = builder.grid()
    assert cells.shape[0] > n and np.array_equal(fleet.GetGrid(1), cells)           # grown, and the two write paths agree
    submap_origin = (float(origin[0]), float(origin[1]))
    case = ((cells, limits[2], (limits[3], limits[4])), submap_origin)
    for mode in MODES:
        want = OC.expected(case, mode)
        got = builder.OccupancyGrid(mode)
        assert OC.same(got, want) and got.resolution == limits[2], mode
        assert OC.same(fleet.occupancy_grids([1], [submap_origin], mode)[0], want), mode
    base = str(tmp_path / "map")
    pgm, yaml = builder.SaveMap(base)
    assert (pgm, yaml) == (base + ".pgm", base + ".yaml")
    painting = W.paint(TC.oracle_texture(case[0]), limits[2], submap_origin)
    assert open(pgm, "rb").read() == W.pgm_bytes(painting, limits[2])
    assert open(yaml, "rb").read() == W.yaml_bytes(painting, limits[2], pgm)
