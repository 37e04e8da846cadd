"""node_replay.FleetNode's own part -- which message goes where, the first-scan rule, odometry before the filter exists, which pose
goes to the mapper -- without a GPU: a FleetNode over the oracle fleet backend of tests/oracle_fleet_node.py against B single Nodes
over ``oracle_backend()``.  Both sides run the same code underneath, so every comparison is exact (== / array_equal)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import oracle_fleet_node as OF

# (scans, beams) per robot: different lidars, one robot with fewer scans; START: the tick of each robot's first scan
SHAPES = ((6, 1440), (5, 2880), (4, 1440))
START = (0, 2, 1)


def _configs():
    from reflector_ekf_slam_amd import synth
    return [synth.SessionConfig(f"node{i}", 40, 12, synth.DIFF, seed=31 + i, speed=1.0, row_spacing=6.0) for i in range(3)]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    from reflector_ekf_slam_amd.node_replay import synth_dump
    d = tmp_path_factory.mktemp("fleet_node")
    return [synth_dump(str(d / f"robot{i}.npz"), cfg, max_scans=n, n_beams=beams, seed=5 + i)
            for i, (cfg, (n, beams)) in enumerate(zip(_configs(), SHAPES))]


def _nodes(dumps, metas=None):
    from reflector_ekf_slam_amd.node_replay import Node
    from tests.oracle_node import oracle_backend
    nodes = []
    for i, d in enumerate(dumps):
        node = Node(d.meta if metas is None else metas[i], OF.recording(oracle_backend()))
        node.run(d)
        nodes.append(node)
    return nodes


@pytest.fixture(scope="module")
def nodes(oracle_lib, dumps):
    return _nodes(dumps)


def _fleet_node(dumps, cls=None, metas=None):
    from reflector_ekf_slam_amd.node_replay import FleetNode
    node = (cls or FleetNode)([d.meta for d in dumps] if metas is None else metas, OF.oracle_fleet_backend())
    node.run(dumps, START)
    return node


def _same_filters(fleet_node, nodes):
    n = fleet_node.fleet.n()
    for m, node in enumerate(nodes):
        got, want = fleet_node.fleet.get_state(m), node.slam.GetState()
        if not (n[m] == node.slam.n and got.time == want.time and np.array_equal(got.mu, want.mu) and np.array_equal(got.sigma, want.sigma)):
            return False
    return True


def test_the_dumps_are_what_the_test_needs(dumps, nodes):
    assert [len(d.scan_t) for d in dumps] == [s for s, _ in SHAPES]
    assert [int(d.scan_off[1] - d.scan_off[0]) for d in dumps] == [b for _, b in SHAPES]
    assert len(set(START)) == 3
    for d, node in zip(dumps, nodes):
        assert d.odom_t[0] < d.scan_t[0]                                           # odometry arrives before the filter exists
        assert ((d.odom_t > d.scan_t[0]) & (d.odom_t < d.scan_t[1])).any()         # ... and between the first scan and the second
        assert len(node.log.observations) == len(d.scan_t) - 1                     # the first scan is not processed
        assert all(1 <= c.shape[0] <= 32 for _, c in node.log.observations)
        assert sum(p is not None for p in node.log.match_poses) == len(d.scan_t) - 1   # every processed scan is inserted
        assert node.slam.n > 3


def test_fleet_node_is_b_nodes(dumps, nodes):
    fn = _fleet_node(dumps)
    assert OF.differences(fn, nodes) == []
    assert _same_filters(fn, nodes)
    assert fn.has_filter == [True] * 3 and all(not log.skipped for log in fn.logs)
    for m, node in enumerate(nodes):                                               # the submaps, through the mapper's own door
        cells, limits = fn.map_builder.grid(m)
        want_cells, want_limits = node.map_builder.grid()
        assert tuple(limits) == tuple(want_limits) and np.array_equal(cells, want_cells)
        assert [rd.returns.shape[0] for _, rd, _ in fn.logs[m].mapper_inputs] and all(rd.misses.shape == (0, 2) for _, rd, _ in fn.logs[m].mapper_inputs)


def test_tick_by_hand_is_run(dumps, nodes):
    """``run``'s schedule, restated: member m's k-th segment in tick START[m] + k, members in any order inside a tick."""
    from reflector_ekf_slam_amd.node_replay import FleetNode
    fn = FleetNode([d.meta for d in dumps], OF.oracle_fleet_backend())
    assert fn.tick() == [] and fn.tick([], []) == []
    last = max(s + len(d.scan_t) for s, d in zip(START, dumps))
    reached = []
    for tick in range(last):
        od, sc = [], []
        for m in (2, 0, 1):
            d, k = dumps[m], tick - START[m]
            if not 0 <= k < len(d.scan_t):
                continue
            lo = d.scan_t[k - 1] if k else -np.inf
            od += [(m, d.odom_t[i], d.odom_pose[i], d.odom_twist[i]) for i in range(len(d.odom_t)) if lo < d.odom_t[i] <= d.scan_t[k]]
            sc.append((m, d.scan(k)))
        reached.append(fn.tick(od, sc))
    assert reached[0] == [] and reached[1] == [0] and sorted(reached[3]) == [0, 1, 2]      # first scans reach nobody
    assert OF.differences(fn, nodes) == []
    with pytest.raises(ValueError):
        fn.tick([], [(0, dumps[0].scan(0)), (0, dumps[0].scan(1))])
    with pytest.raises(ValueError):
        fn.tick([], [(3, dumps[0].scan(0))])


def test_a_processed_first_scan_is_caught(dumps, nodes):
    """Planted defect: the first scan of a member is processed as every other scan is (the reference only constructs the filter)."""
    from reflector_ekf_slam_amd.node_replay import FleetNode

    class ProcessesTheFirstScan(FleetNode):
        def tick(self, odometry=(), scans=()):
            scans = list(scans)
            new = [(m, sc) for m, sc in scans if not self.has_filter[m]]
            out = super().tick(odometry, scans)
            return out + (super().tick((), new) if new else [])

    diff = OF.differences(_fleet_node(dumps, ProcessesTheFirstScan), nodes)
    assert {m for m, _ in diff} == {0, 1, 2} and all("scans processed" in what for _, what in diff)


def test_odometry_before_the_first_scan_reaching_the_filter_is_caught(dumps, nodes):
    """Planted defect: a member's filter exists from its first odometry message on, so the odometry in front of its first scan
    reaches the filter (the first scan is still not processed).  Handing that odometry over late instead would show nothing: the
    filter drops a message older than its state (reflector_ekf_slam.cc:211-212), and the first scan never reaches the detector."""
    from reflector_ekf_slam_amd.node_replay import FleetNode

    class FilterFromTheFirstOdometry(FleetNode):
        def tick(self, odometry=(), scans=()):
            odometry, scans = list(odometry), list(scans)
            self.early = getattr(self, "early", set())
            for m, t, _, _ in odometry:
                if not self.has_filter[m]:
                    self.fleet.set_state(m, float(t), np.array(self.metas[m]["initial_pose"], np.float64), np.zeros((3, 3)), vt=np.zeros(3))
                    self.has_filter[m] = True
                    self.early.add(m)
            first = {m for m, _ in scans if m in self.early}
            self.early -= first
            return super().tick(odometry, [(m, sc) for m, sc in scans if m not in first])

    fn = _fleet_node(dumps, FilterFromTheFirstOdometry)
    diff = OF.differences(fn, nodes)
    assert {m for m, _ in diff} == {0, 1, 2} and any("pose to the mapper" in what for _, what in diff)
    assert not _same_filters(fn, nodes)


def test_a_shared_map(dumps, nodes, tmp_path):
    """The second pass: robots 0 and 2 localise against the reflector map robot 0 saved, robot 1 has none."""
    from reflector_ekf_slam_amd.node_replay import FleetNode
    saved = nodes[0].SaveReflectorResult(str(tmp_path / "map0"), reference_bytes=False)
    metas = [dict(d.meta, map_path=saved if m != 1 else "") for m, d in enumerate(dumps)]
    with_map = _nodes(dumps, metas)
    fn = _fleet_node(dumps, metas=metas)
    assert fn.fleet._map[1] == {0, 2} and fn.fleet._map[0].reflector_map_.shape[0] == (nodes[0].slam.n - 3) // 2
    assert OF.differences(fn, with_map) == [] and _same_filters(fn, with_map)
    assert with_map[0].slam.n < nodes[0].slam.n                                    # the map took robot 0's reflectors
    assert OF.differences(fn, nodes) != []
    for m in range(3):                                                             # SaveReflectorResult: the loaded points first
        a, b = fn.SaveReflectorResult(m, str(tmp_path / f"fleet{m}")), with_map[m].SaveReflectorResult(str(tmp_path / f"node{m}"))
        assert open(a, "rb").read() == open(b, "rb").read()
    other = str(tmp_path / "other.txt")
    open(other, "w").write(open(saved).read())
    with pytest.raises(ValueError):
        FleetNode([dict(metas[0]), dict(metas[1]), dict(metas[2], map_path=other)], OF.oracle_fleet_backend())


def test_docstring_names_what_is_out_of_scope():
    from reflector_ekf_slam_amd import node_replay
    doc = " ".join(node_replay.FleetNode.__doc__.split())
    for what in ("USE_GPS", "PointCloudCallback", "pose log after every odometry message", "device-to-device"):
        assert what in doc, what
    import reflector_ekf_slam_amd as R
    assert R.FleetNode is node_replay.FleetNode and R.FleetBackend is node_replay.FleetBackend
