"""reflector_ekf_slam_amd -- MI355X-native hot path of ShihanWang/reflector_ekf_slam.

Only what the path needs: ``csrc/`` (HIP kernels + the C ABI of include/*.h), the
host-side mirrors of the reference's two interfaces (``ekf_slam``, ``detect``), their
fleet forms (``fleet``, ``fleet_detect``), the fleet scan matcher (``fleet_match``), the
synthetic session generator (``synth``) and the session driver (``session``).
"""
from .ekf_slam import (DIFF, OMNI, EKFOptions, Map, Observation, OdometryData,  # noqa: F401
                       ReflectorEKFSLAM, ReflectorMatchResult, RekfError, State)
from .fleet import FleetSnapshot, ReflectorEKFSLAMFleet, linked_scan_event  # noqa: F401
from .fleet_detect import (DetectLink, LaserReflectorDetectFleet, PointCloud, PointCloudReflectorDetectFleet, cloud_events,  # noqa: F401
                           linked_scan_events, scan_events)
from .grid import OccupancyGrid  # noqa: F401
from .fleet_match import (FleetFilterResult, FleetOccupancyGrid, FleetRangeDataResult, FleetRefineResult, FleetScanMatchResult, FleetTexture,  # noqa: F401
                          RgridBatchFilterScan, RgridBatchInsertScan, RgridBatchRangeData, ScanMatchFleet, gravity_aligned_scans, pose_fixes)
from .map_builder import FleetMapBuilder  # noqa: F401
from .node_replay import FleetBackend, FleetNode, pose_with_covariance  # noqa: F401
