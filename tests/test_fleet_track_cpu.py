"""The fleet's pose track, what can be checked without a GPU: the C ABI of its three calls, ``pose_with_covariance``, FleetNode's
``pose_log`` over the oracle backend of tests/oracle_fleet_track.py against B single Nodes (both sides run the same code underneath:
every comparison is exact), two planted defects, and the staleness guard of profiles/fleet_track_bench.json."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import math
import os

import numpy as np
import pytest

from tests import oracle_fleet_node as OF
from tests import oracle_fleet_track as OT
from tests.fleet_harness import ROOT, _lib, fleet_mod

# the dumps of tests/test_fleet_node_cpu.py
SHAPES = ((6, 1440), (5, 2880), (4, 1440))
START = (0, 2, 1)
TRACK_BENCH_SOURCES = ["include/rfleet.h", "reflector_ekf_slam_amd/csrc/fleet_dev.h", "reflector_ekf_slam_amd/csrc/fleet_host.h", "reflector_ekf_slam_amd/csrc/fleet_kernels.hip",
                       "reflector_ekf_slam_amd/csrc/rfleet_api.hip", "reflector_ekf_slam_amd/fleet.py", "scripts/fleet_track_bench.py"]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_the_track_calls_are_exported_and_the_record_has_the_bindings_layout():
    L = _lib()
    for name in ("rfleet_set_tracking", "rfleet_take_track", "rfleet_sizeof_track_rec"):
        assert hasattr(L, name), name
    F = fleet_mod()
    assert L.rfleet_sizeof_track_rec() == C.sizeof(F.RfleetTrackRec) == F.TRACK_DTYPE.itemsize == 144
    for name, _ in F.RfleetTrackRec._fields_:
        assert getattr(F.RfleetTrackRec, name).offset == F.TRACK_DTYPE.fields[name][1], name
    assert F._track_lib() is L


def test_null_handles_are_refused_before_any_hip_call():
    F = fleet_mod()
    L = F._track_lib()
    counts = (C.c_int * 4)()
    out = (F.RfleetTrackRec * 4)()
    assert L.rfleet_set_tracking(None, 1, 0) == -1
    assert L.rfleet_take_track(None, None, 0, C.addressof(counts), C.addressof(out), 4, None) == -1
    assert L.rfleet_take_track(None, None, 4, C.addressof(counts), None, 0, None) == -1


# ---- StatePosetoRosPose -----------------------------------------------------------------------------------------------------------
def test_pose_with_covariance_sets_the_nine_entries_of_the_reference():
    from reflector_ekf_slam_amd import pose_with_covariance
    sg = np.arange(1.0, 10.0).reshape(3, 3) * 0.125                   # not symmetric: every entry tells where it came from
    for theta in (0.0, 1.25, -3.0, math.pi):
        pos, quat, cov = pose_with_covariance([2.0, -3.5, theta], sg)
        assert pos == (2.0, -3.5, 0.0)
        assert quat == (0.0, 0.0, math.sin(theta / 2), math.cos(theta / 2))   # src/ros_node.cc:804-807
        assert cov.shape == (36,)
        want = {0: sg[0, 0], 1: sg[0, 1], 5: sg[0, 2], 6: sg[1, 0], 7: sg[1, 1], 11: sg[1, 2], 30: sg[2, 0], 31: sg[2, 1], 35: sg[2, 2]}
        for k in range(36):
            assert cov[k] == want.get(k, 0.0), k


# ---- FleetNode(pose_log=True) over the oracle -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    from reflector_ekf_slam_amd import synth
    from reflector_ekf_slam_amd.node_replay import synth_dump
    d = tmp_path_factory.mktemp("fleet_track")
    cfgs = [synth.SessionConfig(f"node{i}", 40, 12, synth.DIFF, seed=31 + i, speed=1.0, row_spacing=6.0) for i in range(3)]
    return [synth_dump(str(d / f"robot{i}.npz"), cfg, max_scans=n, n_beams=beams, seed=5 + i) for i, (cfg, (n, beams)) in enumerate(zip(cfgs, SHAPES))]


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


def _fleet_node(dumps, cls=None, **kw):
    from reflector_ekf_slam_amd.node_replay import FleetNode
    fn = (cls or FleetNode)([d.meta for d in dumps], OT.oracle_fleet_track_backend(), **kw)
    fn.run(dumps, START)
    return fn


def _pose_log_differences(fn, nodes):
    return [m for m, node in enumerate(nodes) if [e[:4] for e in fn.logs[m].pose_log] != node.log.path]


def test_pose_log_is_the_single_nodes_path(dumps, nodes):
    fn = _fleet_node(dumps, pose_log=True)
    assert fn.fleet.track_calls == 1 and fn.fleet.tracking
    assert OF.differences(fn, nodes) == []
    for m, node in enumerate(nodes):
        log = fn.logs[m]
        assert [e[:4] for e in log.pose_log] == node.log.path                      # exactly: stamps and poses, in message order
        assert len(log.pose_log) > len(log.path) > 0
        assert all(e[4].shape == (3, 3) for e in log.pose_log)
        stamps = [e[0] for e in log.pose_log]
        assert [e for e in log.pose_log if e[0] in {p[0] for p in log.path}][-1][:4] == log.path[-1]
        # odometry before the member's first scan appears in neither log
        d = dumps[m]
        early = d.odom_t[d.odom_t < d.scan_t[0]]
        assert early.size > 0 and not set(early.tolist()) & set(stamps) and not set(early.tolist()) & {p[0] for p in node.log.path}
        assert min(stamps) > d.scan_t[0]
        # the covariance beside the last entry is the filter's
        assert np.array_equal(log.pose_log[-1][4], fn.fleet.poses()[2][m])
    assert all(not r for r in fn.fleet.records)                                    # run's last harvest left nothing behind


def test_without_pose_log_no_tracking_call_reaches_the_backend(dumps, nodes):
    from reflector_ekf_slam_amd.node_replay import FleetNode
    assert not hasattr(OF.OracleFilterFleet, "track") and not hasattr(OF.OracleFilterFleet, "take_track")
    fn = FleetNode([d.meta for d in dumps], OF.oracle_fleet_backend())             # the existing tests' backend: it has neither call
    fn.run(dumps, START)
    assert OF.differences(fn, nodes) == [] and all(log.pose_log == [] for log in fn.logs)
    fn = _fleet_node(dumps)
    assert fn.fleet.track_calls == 0 and all(log.pose_log == [] for log in fn.logs)


def test_a_tick_of_odometry_only_does_not_harvest(dumps):
    from reflector_ekf_slam_amd.node_replay import FleetNode
    fn = FleetNode([dumps[0].meta], OT.oracle_fleet_track_backend(), pose_log=True)
    d = dumps[0]
    fn.tick([], [(0, d.scan(0))])
    taken = []
    take = fn.fleet.take_track
    fn.fleet.take_track = lambda members=None: taken.append(1) or take(members)
    od = [(0, d.odom_t[i], d.odom_pose[i], d.odom_twist[i]) for i in range(len(d.odom_t)) if d.scan_t[0] < d.odom_t[i] <= d.scan_t[1]]
    assert len(od) >= 2 and fn.tick(od[:1]) == [] and fn.tick(od[1:]) == [] and taken == [] and fn.logs[0].pose_log == []
    fn.harvest_pose_log()
    assert taken == [1] and [e[0] for e in fn.logs[0].pose_log] == [float(o[1]) for o in od]


def test_a_node_that_logs_scans_without_reflectors_is_caught(dumps, nodes):
    """Planted defect: the K > 0 test of src/ros_node.cc:524 is missing.  A scan without a reflector in view is played to both sides."""
    from reflector_ekf_slam_amd.detect import LaserScan
    from reflector_ekf_slam_amd.node_replay import FleetNode, Node
    from tests.oracle_node import oracle_backend

    class LogsEveryScan(FleetNode):
        def harvest_pose_log(self):
            for m, tr in enumerate(self.fleet.take_track()):
                self.logs[m].pose_log += [(float(tr.t[r]), *(float(v) for v in tr.mu[r]), tr.sigma[r]) for r in range(len(tr))]

    d = dumps[0]
    sc = d.scan(1)
    dark = LaserScan(sc.stamp, sc.angle_min, sc.angle_max, sc.angle_increment, sc.scan_time, sc.range_min, sc.range_max, sc.ranges,
                     np.zeros_like(sc.intensities))
    od = [(0, d.odom_t[i], d.odom_pose[i], d.odom_twist[i]) for i in range(len(d.odom_t)) if d.scan_t[0] < d.odom_t[i] <= d.scan_t[1]]
    node = Node(d.meta, oracle_backend())
    node.ScanCallback(d.scan(0))
    for o in od:
        node.OdometryCallback(*o[1:])
    node.ScanCallback(dark)
    assert node.log.observations[-1][1].shape[0] == 0 and len(node.log.path) == len(od)
    logs = {}
    for cls in (FleetNode, LogsEveryScan):
        fn = cls([d.meta], OT.oracle_fleet_track_backend(), pose_log=True)
        fn.tick([], [(0, d.scan(0))])
        assert fn.tick(od, [(0, dark)]) == [0]
        logs[cls] = [e[:4] for e in fn.logs[0].pose_log]
    assert logs[FleetNode] == node.log.path
    assert logs[LogsEveryScan] != node.log.path and logs[LogsEveryScan][:-1] == node.log.path


def test_a_node_that_logs_odometry_from_before_the_filter_is_caught(dumps, nodes):
    """Planted defect: the filter exists (and is tracked) from the first odometry message on, so messages in front of the first
    scan are logged."""
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

    assert _pose_log_differences(_fleet_node(dumps, pose_log=True), nodes) == []
    fn = _fleet_node(dumps, FilterFromTheFirstOdometry, pose_log=True)
    assert _pose_log_differences(fn, nodes) == [0, 1, 2]
    for m, d in enumerate(dumps):
        assert fn.logs[m].pose_log[0][0] < d.scan_t[0]


# ---- the measurement describes the tree --------------------------------------------------------------------------------------------
def test_fleet_track_bench_describes_the_tree():
    """profiles/fleet_track_bench.json was measured on the fleet sources of this tree (SHA-256 by content)."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "fleet_track_bench.json")))
    sums = rec["_sources_sha256"]
    assert sorted(sums) == sorted(TRACK_BENCH_SOURCES)
    for rel in TRACK_BENCH_SOURCES:
        have = hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
        assert have == sums[rel], f"{rel} changed since profiles/fleet_track_bench.json was measured: measure again (scripts/fleet_track_bench.py)"
    for B in ("4", "64", "256"):
        for leg in ("untracked_submit_sync", "tracked_submit_take_track", "submit_poses_per_message"):
            s = rec[leg][B]
            assert 0 < s["min"] <= s["median"] <= s["max"]
        assert rec["per_message_min_over_tracked_max"][B] == rec["submit_poses_per_message"][B]["min"] / rec["tracked_submit_take_track"][B]["max"]
