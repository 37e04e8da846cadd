"""Test infrastructure for the fleet filter's wide scans at the node's level: the oracle fleet backend of tests/oracle_fleet_node.py
with a filter fleet that accepts ``wide_scans`` (the oracle knows no limit on a scan's width), and the two messages of the 34-plate
scan of tests/test_fleet_node_gpu.py, for a FleetNode and a single Node to be fed alike."""
from __future__ import annotations

from reflector_ekf_slam_amd.node_replay import FleetBackend
from tests import oracle_fleet_node as OF

PLATES = 34


class WideOracleFilterFleet(OF.OracleFilterFleet):
    wide = False

    def wide_scans(self, on=True):
        self.wide = bool(on)


def wide_oracle_fleet_backend() -> FleetBackend:
    return FleetBackend(make_detector_fleet=OF.OracleDetectorFleet, make_filter_fleet=WideOracleFilterFleet, make_map_builder=OF.OracleMapBuilders)


def plate_messages(stamps=(1.0, 2.0), plates=PLATES):
    """The same hand-built scan of `plates` reflector plates (7200 beams, 2 m away) at each stamp."""
    from reflector_ekf_slam_amd.detect import LaserScan
    from tests.detect_cases import beams_for_width, plate_scan
    n, r = 7200, 2.0
    nb = beams_for_width(0.18, r, n)
    sc = plate_scan(n, [(50 + 200 * k, nb, r, 200.0) for k in range(plates)], stamp=stamps[0])
    return [LaserScan(t, sc.angle_min, sc.angle_max, sc.angle_increment, sc.scan_time, sc.range_min, sc.range_max, sc.ranges, sc.intensities)
            for t in stamps]


def single_node(meta, messages):
    """A single Node over the recording oracle backend, fed the messages."""
    from reflector_ekf_slam_amd.node_replay import Node
    from tests.oracle_node import oracle_backend
    node = Node(meta, OF.recording(oracle_backend()))
    for msg in messages:
        node.ScanCallback(msg)
    return node
