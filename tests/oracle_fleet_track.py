"""tests/oracle_fleet_node.py's oracle filter fleet with the pose track (``track`` / ``take_track``) of ReflectorEKFSLAMFleet, for
FleetNode(pose_log=True) without a GPU: every member is an OracleSlam of tests/oracle_node.py, and a record is that member's
``pose()`` behind the message (test infrastructure only)."""
from __future__ import annotations

import numpy as np

from reflector_ekf_slam_amd.fleet import MemberTrack
from reflector_ekf_slam_amd.node_replay import FleetBackend
from tests import oracle_fleet_node as OF


class OracleFilterFleetWithTrack(OF.OracleFilterFleet):
    def __init__(self, opts):
        super().__init__(opts)
        self.tracking = False
        self.records = [[] for _ in range(self.B)]
        self.track_calls = 0

    def track(self, on=True, max_records=0):
        self.tracking = bool(on)
        self.track_calls += 1

    def submit(self, events):
        for ev in events:
            member = ev[0]
            before = self.slams[member].pose()[0]
            super().submit([ev])
            if self.tracking:
                kind, t, cloud = ev[1], ev[2], ev[4]
                _, mu3, sg = self.slams[member].pose()
                K = 0 if kind == 0 or cloud is None else int(np.asarray(cloud).size // 2)
                self.records[member].append((float(t), int(kind), K, int(kind == 0 and t < before), mu3, sg, self.slams[member].n))

    def take_track(self, members=None):
        out = []
        for m in (range(self.B) if members is None else members):
            r, self.records[m] = self.records[m], []
            z = np.zeros(len(r), np.int32)
            out.append(MemberTrack(np.array([x[0] for x in r]), np.array([x[1] for x in r], np.int32), np.array([x[2] for x in r], np.int32),
                                   np.array([x[3] for x in r], np.int32), np.array([x[4] for x in r]).reshape(-1, 3),
                                   np.array([x[5] for x in r]).reshape(-1, 3, 3), np.array([x[6] for x in r], np.int32), z, z, z, z, 0))
        return out


def oracle_fleet_track_backend() -> FleetBackend:
    return FleetBackend(make_detector_fleet=OF.OracleDetectorFleet, make_filter_fleet=OracleFilterFleetWithTrack,
                        make_map_builder=OF.OracleMapBuilders)
