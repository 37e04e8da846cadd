"""The three fleets of reflector_ekf_slam_amd.node_replay.FleetNode over the CPU ORACLE: every member is one of the components of
tests/oracle_node.py, looped over, so that a FleetNode over this backend and B Nodes over ``oracle_backend()`` run the same code
underneath and differ in nothing but FleetNode's own message flow (test infrastructure only).  ``differences`` holds the two to
each other; ``recording`` makes a Backend whose map builder keeps what its Node handed to it."""
from __future__ import annotations

import dataclasses

import numpy as np

from reflector_ekf_slam_amd.ekf_slam import Map, Observation, save_map_txt
from reflector_ekf_slam_amd.node_replay import Backend, FleetBackend
from tests.oracle_node import OracleDetector, OracleSlam, oracle_backend

BAD_SCAN = -3


class OracleDetectorFleet:
    def __init__(self, opts, s2b):
        self.members = [OracleDetector(o, tuple(s)) for o, s in zip(opts, np.asarray(s2b, np.float64).reshape(-1, 3))]

    def HandleOdometryData(self, member, msg):
        self.members[member].HandleOdometryData(msg)

    def detect(self, scans):
        out = []
        for member, scan in scans:
            try:
                out.append((0, self.members[member].HandleLaserScan(scan)))
            except ValueError:                                                     # the oracle's refusal of a malformed message
                out.append((BAD_SCAN, Observation(float(scan.stamp))))
        return out

    def range_data(self, members=None):
        return [self.members[m].GetRangeData() for m in (range(len(self.members)) if members is None else members)]


class OracleFilterFleet:
    """ReflectorEKFSLAMFleet's calls that FleetNode uses, every member an OracleSlam made by its ``set_state``."""

    def __init__(self, opts):
        self.options = list(opts)
        self.B = len(self.options)
        self.slams = [None] * self.B
        self._map = None

    def set_map(self, xy, cov, members=None):
        self._map = (Map(np.asarray(xy), np.asarray(cov)), set(range(self.B) if members is None else members))

    def set_state(self, i, t, mu, sigma, vt=None):
        assert np.asarray(mu).shape == (3,) and not np.asarray(sigma).any() and (vt is None or not np.asarray(vt).any())
        slam = OracleSlam(dataclasses.replace(self.options[i], init_time=float(t), init_pose=tuple(float(v) for v in mu), map_path=""))
        if self._map is not None and i in self._map[1]:
            slam._map = self._map[0]
            slam._o.set_map(slam._map.reflector_map_, slam._map.reflector_map_coviarance_)
        self.slams[i] = slam

    def submit(self, events):
        for ev in events:
            member, kind, t, v, cloud = ev[:5]
            o = self.slams[member]._o
            if kind == 0:
                o.handle_odometry(t, v[0], v[1], v[2])
            else:
                o.handle_observation(t, cloud, None)

    def poses(self):
        t, mu, sg = np.zeros(self.B), np.zeros((self.B, 3)), np.zeros((self.B, 3, 3))
        for i, s in enumerate(self.slams):
            if s is not None:
                t[i], mu[i], sg[i] = s.pose()
        return t, mu, sg

    def n(self):
        return np.array([3 if s is None else s.n for s in self.slams], np.int32)

    def flags(self):
        return np.zeros(self.B, np.int32)

    def get_state(self, i, want_sigma=True):
        return self.slams[i].GetState()

    def save_map_txt(self, member, path, reference_bytes=False):
        s = self.slams[member]
        save_map_txt(path, s.GetState(), s.GetGlobalMap(), reference_bytes=reference_bytes)


class OracleMapBuilders:
    """FleetMapBuilder's AddRangeData over one oracle MapBuilder per member: ``oracle_backend().make_map_builder()``, looped."""

    def __init__(self, B):
        make = oracle_backend().make_map_builder
        self.builders = [make() for _ in range(B)]

    def AddRangeData(self, times, range_datas, ekf_poses, members=None):
        members = list(range(len(range_datas))) if members is None else list(members)
        assert len(set(members)) == len(members)
        return [self.builders[m].AddRangeData(t, rd, pose) for m, t, rd, pose in zip(members, times, range_datas, ekf_poses)]

    def grid(self, member):
        return self.builders[member].grid()


def oracle_fleet_backend() -> FleetBackend:
    return FleetBackend(make_detector_fleet=OracleDetectorFleet, make_filter_fleet=OracleFilterFleet, make_map_builder=OracleMapBuilders)


# ---- the single-robot side: a Backend whose map builder keeps what it was given ------------------------------------------------------
class RecordingMapBuilder:
    def __init__(self, inner):
        self.inner, self.inputs, self.results = inner, [], []

    def AddRangeData(self, time, range_data, ekf_pose):
        self.inputs.append((time, range_data, tuple(ekf_pose)))
        res = self.inner.AddRangeData(time, range_data, ekf_pose)
        self.results.append(res)
        return res

    def __getattr__(self, name):
        return getattr(self.inner, name)


def recording(backend: Backend) -> Backend:
    return Backend(backend.make_detector, backend.make_ekf, lambda: RecordingMapBuilder(backend.make_map_builder()))


def differences(fleet_node, nodes, pose_tol=0.0, match_poses=True):
    """What FleetNode's member logs differ in from B single ``Node``s over ``recording(...)`` backends that saw the same dumps: a list
    of (member, what).  Centres, observation times and range data are compared bit for bit; the poses handed to the mapper, the path
    and (with ``match_poses``) the match poses to ``pose_tol`` (0: bit for bit); which scans the mapper inserted is always compared."""
    def close(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return a.shape == b.shape and (np.array_equal(a, b) if pose_tol == 0.0 else bool((np.abs(a - b) <= pose_tol).all()))

    out = []
    for m, (log, node) in enumerate(zip(fleet_node.logs, nodes)):
        want_obs, want_in = node.log.observations, node.map_builder.inputs
        if len(log.observations) != len(want_obs) or len(log.mapper_inputs) != len(want_in):
            out.append((m, f"{len(log.observations)} scans processed, {len(log.mapper_inputs)} to the mapper; the node: {len(want_obs)}, {len(want_in)}"))
            continue
        for k, ((t, c), (wt, wc)) in enumerate(zip(log.observations, want_obs)):
            if t != wt:
                out.append((m, f"scan {k}: observation time"))
            if c.shape != wc.shape or c.tobytes() != wc.tobytes():
                out.append((m, f"scan {k}: centres"))
        for k, ((t, rd, pose), (wt, wrd, wpose)) in enumerate(zip(log.mapper_inputs, want_in)):
            if t != wt:
                out.append((m, f"scan {k}: stamp to the mapper"))
            if np.asarray(rd.origin, np.float32).tobytes() != np.asarray(wrd.origin, np.float32).tobytes():
                out.append((m, f"scan {k}: range data origin"))
            if rd.returns.shape != wrd.returns.shape or rd.returns.tobytes() != wrd.returns.tobytes():
                out.append((m, f"scan {k}: range data returns"))
            if not close(pose, wpose):
                out.append((m, f"scan {k}: pose to the mapper"))
        seen = [p for (_, c), (_, _, p) in zip(log.observations, log.mapper_inputs) if c.shape[0] > 0]
        if [p[1:] for p in log.path] != seen or len(log.path) != sum(c.shape[0] > 0 for _, c in want_obs):
            out.append((m, "path: one entry per scan that saw reflectors, the pose after its update"))
        if pose_tol == 0.0 and not set(log.path) <= set(node.log.path):
            out.append((m, "path: an entry the node does not have"))
        for k, (g, w) in enumerate(zip(log.match_poses, node.log.match_poses)):
            if (g is None) != (w is None) or (match_poses and g is not None and not close(g, w)):
                out.append((m, f"scan {k}: match pose"))
        if len(log.match_poses) != len(node.log.match_poses):
            out.append((m, "match poses: count"))
    return out
