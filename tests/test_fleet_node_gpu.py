"""node_replay.FleetNode over the three HIP fleets (-m gpu): three robots with different lidars, scan counts and start ticks against
three single Nodes over the CPU oracle's components, and its mapper against a single MapBuilder (HIP GridFrontEnd) per robot that is
fed exactly what FleetNode logged."""
from __future__ import annotations

import numpy as np
import pytest

from tests import oracle_fleet_node as OF

pytestmark = pytest.mark.gpu

SHAPES = ((14, 1440), (12, 2880), (9, 1440))          # (scans, beams) per robot
START = (0, 3, 1)
INSERTED = [13, 11, 8]                                # every processed scan of every robot, on both sides
MAX_OBS = 32


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    from reflector_ekf_slam_amd import synth
    from reflector_ekf_slam_amd.node_replay import synth_dump
    d = tmp_path_factory.mktemp("fleet_node_gpu")
    cfgs = [synth.SessionConfig(f"node{i}", 40, 12, synth.DIFF, seed=31 + i, speed=1.0, row_spacing=6.0) for i in range(3)]
    return [synth_dump(str(d / f"robot{i}.npz"), cfg, max_scans=n, n_beams=beams) for i, (cfg, (n, beams)) in enumerate(zip(cfgs, SHAPES))]


@pytest.fixture(scope="module")
def nodes(oracle_lib, dumps):
    from reflector_ekf_slam_amd.node_replay import Node
    from tests.oracle_node import oracle_backend
    out = []
    for d in dumps:
        node = Node(d.meta, OF.recording(oracle_backend()))
        node.run(d)
        out.append(node)
    return out


@pytest.fixture(scope="module")
def fleet_node(dumps):
    from reflector_ekf_slam_amd.node_replay import FleetNode
    fn = FleetNode([d.meta for d in dumps])
    fn.run(dumps, START)
    yield fn
    fn.detector.close()
    fn.fleet.close()
    fn.map_builder._fleet.close()


def test_the_oracle_nodes_meet_the_conditions(dumps, nodes):
    assert [(len(d.scan_t), int(d.scan_off[1] - d.scan_off[0])) for d in dumps] == list(SHAPES)
    for node, want in zip(nodes, INSERTED):
        assert len(node.log.observations) == want and sum(p is not None for p in node.log.match_poses) == want
        assert all(6 <= c.shape[0] <= 15 for _, c in node.log.observations)
        assert 3 < node.slam.n <= 33


def test_fleet_node_against_three_oracle_nodes(dumps, nodes, fleet_node):
    fn = fleet_node
    assert fn.has_filter == [True] * 3 and all(not log.skipped for log in fn.logs)
    # centres, observation times and range data bit for bit; the poses within 1e-9; which scans were inserted
    assert OF.differences(fn, nodes, pose_tol=1e-9, match_poses=False) == []
    assert [sum(p is not None for p in log.match_poses) for log in fn.logs] == INSERTED == [len(log.observations) for log in fn.logs]
    n = fn.fleet.n()
    assert (fn.fleet.flags() == 0).all()
    for m, node in enumerate(nodes):
        got, want = fn.fleet.get_state(m, want_sigma=False), node.slam.GetState()
        assert n[m] == node.slam.n and got.time == want.time
        err = float(np.abs(got.mu - want.mu).max())
        print(f"robot {m}: n = {n[m]}, max|mu - oracle| = {err:.3e}")
        assert err < 1e-9
        path = np.array(fn.logs[m].path)
        scan_entries = np.array([p for p in node.log.path if p[0] in set(path[:, 0])])
        assert path.shape[0] == INSERTED[m] and np.abs(path[:, 1:] - np.array([i[2] for i in node.map_builder.inputs])).max() < 1e-9
        assert scan_entries.shape[0] >= path.shape[0]
    # the pass-throughs
    marks = fn.markers()
    assert [e.shape for e in marks] == [((k - 3) // 2, 5) for k in n.tolist()]
    assert [e.shape for e in fn.markers([2, 0])] == [marks[2].shape, marks[0].shape]
    grids = fn.occupancy_grids()
    assert len(grids) == 3 and all(g is not None and g.data.size > 0 for g in grids)


def test_the_mapper_got_what_a_map_builder_per_robot_gets(fleet_node, tmp_path):
    """FleetNode's logged (stamp, RangeData, pose) of every robot through a single MapBuilder over a HIP GridFrontEnd of its own:
    local_pose, range_data_in_local, the final cells and limits are the same bits.  No tolerance."""
    from reflector_ekf_slam_amd.map_builder import MapBuilder, MapBuilderOptions
    fn = fleet_node
    for m, log in enumerate(fn.logs):
        mb = MapBuilder(MapBuilderOptions(), max_points=8192, max_cells=2048 * 2048)
        assert len(log.mapper_inputs) == len(log.match_results) == INSERTED[m]
        for k, ((stamp, rd, pose), got) in enumerate(zip(log.mapper_inputs, log.match_results)):
            want = mb.AddRangeData(stamp, rd, pose)
            assert want is not None and got is not None, (m, k)
            assert got.time == want.time and got.local_pose.tobytes() == np.asarray(want.local_pose, np.float64).tobytes(), (m, k)
            a, b = got.range_data_in_local.returns, want.range_data_in_local.returns
            assert a.shape == b.shape == rd.returns.shape and a.tobytes() == b.tobytes(), (m, k)
        assert mb.num_range_data == fn.map_builder.num_range_data[m] == INSERTED[m]
        cells, limits = fn.map_builder.grid(m)
        want_cells, want_limits = mb.grid()
        assert tuple(limits) == tuple(want_limits) and np.array_equal(cells, want_cells) and (cells != 0).any(), m
        if m == 1:
            mine = [open(f, "rb").read() for f in fn.SaveMap(m, str(tmp_path / "fleet"))]
            theirs = [open(f, "rb").read() for f in mb.SaveMap(str(tmp_path / "fleet"))]
            assert mine == theirs and mine[0].startswith(b"P5\n")
        mb._fe.close()


def test_save_reflector_result_is_the_fleets_saved_map(fleet_node, tmp_path):
    fn = fleet_node
    for reference_bytes in (True, False):
        a = fn.SaveReflectorResult(1, str(tmp_path / f"node{reference_bytes}"), reference_bytes=reference_bytes)
        b = str(tmp_path / f"fleet{reference_bytes}.txt")
        fn.fleet.save_map_txt(1, b, reference_bytes=reference_bytes)
        got = open(a, "rb").read()
        assert a.endswith(".txt") and got == open(b, "rb").read() and got.count(b"\n") == 2 and len(got) > 100


def test_a_scan_with_too_many_centres_raises_before_the_filter_sees_it(dumps):
    """More than RFLEET_MAX_OBS centres: ValueError, and the filter's state is what it was."""
    from reflector_ekf_slam_amd.node_replay import FleetNode
    from tests.detect_cases import beams_for_width, plate_scan
    from reflector_ekf_slam_amd.detect import LaserScan
    n, r = 7200, 2.0
    nb = beams_for_width(0.18, r, n)
    sc = plate_scan(n, [(50 + 200 * k, nb, r, 200.0) for k in range(MAX_OBS + 2)], stamp=2.0)
    msg = lambda stamp: LaserScan(stamp, sc.angle_min, sc.angle_max, sc.angle_increment, sc.scan_time, sc.range_min, sc.range_max, sc.ranges, sc.intensities)
    fn = FleetNode([dumps[0].meta])
    assert fn.tick([], [(0, msg(1.0))]) == [] and fn.has_filter == [True]
    before = fn.fleet.get_state(0)
    with pytest.raises(ValueError) as e:
        fn.tick([], [(0, msg(2.0))])
    assert str(MAX_OBS + 2) in str(e.value)
    after = fn.fleet.get_state(0)
    assert after.time == before.time and np.array_equal(after.mu, before.mu) and fn.logs[0].observations == []
    fn.detector.close(); fn.fleet.close(); fn.map_builder._fleet.close()
