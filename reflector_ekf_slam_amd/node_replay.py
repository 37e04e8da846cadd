"""Node-level replay of BASELINE.json configs[0] without ROS: the message flow of the reference's ``Node``
(/root/reference/src/ros_node.cc) over an on-disk dump of the two topics it subscribes to.

    odometry message  -> OdometryCallback  (src/ros_node.cc:627-660): detector.HandleOdometryData, slam.HandleOdometryMessage,
                                                                      GetState -> path
    laser scan        -> ScanCallback      (src/ros_node.cc:420-558): the FIRST scan only constructs the EKF (init_time = its
                                                                      stamp, Q11); later ones: HandleLaserScan ->
                                                                      HandleObservationMessage -> GetState ->
                                                                      MapBuilder::AddRangeData(GetRangeData(), ekf pose)
    SaveReflectorResult (src/ros_node.cc:75-140): the two-line txt map (optionally the reference's very bytes)

Dump schema ``rekf-dump-v1`` -- one numpy ``.npz`` (what a rosbag of this node holds, minus ROS):
    meta         json string: {"schema": "rekf-dump-v1", "odom_model": "diff"|"omni", "initial_pose": [x, y, yaw],
                 "sensor_to_base_link": [x, y, yaw], "linear_velocity_sigma", "angular_velocity_sigma", "observation_sigma",
                 "detector": {intensity_min, reflector_min_length, reflector_length_error, range_min, range_max},
                 "map_path": ""}                                                       (launch/slam.launch, src/ros_node.cc:150-300)
    odom_t       [No]     float64   nav_msgs/Odometry header.stamp (s)
    odom_pose    [No, 4]  float64   pose.position.x, .y, pose.orientation.z, .w
    odom_twist   [No, 3]  float64   twist.linear.x, .y, twist.angular.z
    scan_t       [Ns]     float64   sensor_msgs/LaserScan header.stamp (s)
    scan_params  [Ns, 6]  float32   angle_min, angle_max, angle_increment, scan_time, range_min, range_max
    scan_off     [Ns + 1] int64     beam offsets into ranges / intensities
    ranges, intensities  [sum of beams] float32
Messages are replayed in stamp order (ties: odometry first -- ros::spin() is single-threaded, src/ros_node.cc:68).

The three components are injected (``Backend``): the default is the HIP path (detect.LaserReflectorDetect, ReflectorEKFSLAM,
map_builder.MapBuilder); the GPU suite runs the same harness over the CPU oracle's components for comparison.

``FleetNode`` is the same node for B robots over the three fleets (``FleetBackend``: LaserReflectorDetectFleet,
ReflectorEKFSLAMFleet, map_builder.FleetMapBuilder): a ``tick`` hands every robot its odometry and its scan, with launches and
synchronisations that do not grow with B.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, field

import numpy as np

SCHEMA = "rekf-dump-v1"


# ------------------------------------------------------------------------------------------------ dump I/O
@dataclass
class Dump:
    meta: dict
    odom_t: np.ndarray
    odom_pose: np.ndarray
    odom_twist: np.ndarray
    scan_t: np.ndarray
    scan_params: np.ndarray
    scan_off: np.ndarray
    ranges: np.ndarray
    intensities: np.ndarray

    def scan(self, k: int):
        from .detect import LaserScan
        a, b = int(self.scan_off[k]), int(self.scan_off[k + 1])
        p = self.scan_params[k]
        return LaserScan(float(self.scan_t[k]), float(p[0]), float(p[1]), float(p[2]), float(p[3]), float(p[4]), float(p[5]),
                         self.ranges[a:b], self.intensities[a:b])

    def events(self):
        """(kind, index) in stamp order, odometry before a scan of the same stamp."""
        ev = [(float(t), 0, i) for i, t in enumerate(self.odom_t)] + [(float(t), 1, i) for i, t in enumerate(self.scan_t)]
        ev.sort()
        return [("odom" if k == 0 else "scan", i) for _, k, i in ev]


def write_dump(path: str, meta: dict, odom, scans) -> None:
    """odom: iterable of (t, px, py, qz, qw, vx, vy, wz); scans: iterable of LaserScan-like objects."""
    odom = np.asarray(list(odom), dtype=np.float64).reshape(-1, 8)
    scans = list(scans)
    off = np.zeros(len(scans) + 1, np.int64)
    for k, s in enumerate(scans):
        off[k + 1] = off[k] + len(s.ranges)
    m = dict(meta)
    m["schema"] = SCHEMA
    np.savez_compressed(
        path, meta=np.array(json.dumps(m)), odom_t=odom[:, 0], odom_pose=odom[:, 1:5], odom_twist=odom[:, 5:8],
        scan_t=np.array([s.stamp for s in scans], np.float64),
        scan_params=np.array([[s.angle_min, s.angle_max, s.angle_increment, s.scan_time, s.range_min, s.range_max] for s in scans],
                             np.float32).reshape(-1, 6),
        scan_off=off,
        ranges=np.concatenate([np.asarray(s.ranges, np.float32) for s in scans]) if scans else np.zeros(0, np.float32),
        intensities=np.concatenate([np.asarray(s.intensities, np.float32) for s in scans]) if scans else np.zeros(0, np.float32))


def read_dump(path: str) -> Dump:
    z = np.load(path, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    if meta.get("schema") != SCHEMA:
        raise ValueError(f"{path}: not a {SCHEMA} dump (schema = {meta.get('schema')!r})")
    d = Dump(meta, z["odom_t"], z["odom_pose"], z["odom_twist"], z["scan_t"], z["scan_params"], z["scan_off"], z["ranges"],
             z["intensities"])
    if d.scan_off.shape[0] != d.scan_t.shape[0] + 1 or d.scan_off[-1] != d.ranges.shape[0] or d.ranges.shape != d.intensities.shape:
        raise ValueError(f"{path}: inconsistent scan arrays")
    return d


def synth_dump(path: str, cfg, max_scans: int = 60, n_beams: int = 1440, seed: int = 1, sensor_to_base_link=(0.13686, 0.0, 0.0)) -> Dump:
    """A synthetic bag for the harness: a ``synth`` session's odometry (true poses as the odometer's pose, its noisy twist)
    and one simulated LaserScan per scan event."""
    from types import SimpleNamespace

    from . import synth
    sess = synth.make_session(cfg, max_scans=max_scans)
    rng = np.random.Generator(np.random.PCG64(seed))
    odom, scans = [], []
    for e in range(sess.n_events):
        t = float(sess.ev_time[e])
        x, y, th = sess.true_pose[e]
        if sess.ev_type[e] == synth.EV_ODOM:
            odom.append((t, x, y, math.sin(th / 2), math.cos(th / 2), sess.odom[e][0], sess.odom[e][1], sess.odom[e][2]))
        else:
            scans.append(SimpleNamespace(**synth.make_laser_scan(sess.landmarks, sess.true_pose[e], t, rng, n_beams=n_beams,
                                                                 sensor_xy=tuple(sensor_to_base_link[:2]))))
    meta = {"odom_model": "diff" if cfg.odom_model == synth.DIFF else "omni", "initial_pose": [float(v) for v in sess.init_pose],
            "sensor_to_base_link": [float(v) for v in sensor_to_base_link],
            "linear_velocity_sigma": cfg.sigma_v, "angular_velocity_sigma": cfg.sigma_w, "observation_sigma": cfg.sigma_obs,
            "detector": {"intensity_min": 160.0, "reflector_min_length": 0.18, "reflector_length_error": 0.06, "range_min": 0.3,
                         "range_max": 10.0},
            "map_path": ""}
    write_dump(path, meta, odom, scans)
    return read_dump(path)


# ------------------------------------------------------------------------------------------------ the node
@dataclass
class Backend:
    """Factories of the three components ``Node`` owns (include/ros_node.h:131-140)."""
    make_detector: object          # (ReflectorDetectOptions, sensor_to_base_link xyyaw) -> HandleOdometryData / HandleLaserScan / GetRangeData
    make_ekf: object               # (EKFOptions) -> HandleOdometryMessage / HandleObservationMessage / pose() / GetState()
    make_map_builder: object       # () -> AddRangeData(time, RangeData, (x, y, yaw))


def hip_backend(max_landmarks: int = 64, device: int = 0, auto_grow: bool = True) -> Backend:
    from .detect import LaserReflectorDetect
    from .ekf_slam import ReflectorEKFSLAM
    from .map_builder import MapBuilder, MapBuilderOptions
    return Backend(
        make_detector=lambda opt, s2b: LaserReflectorDetect(opt, max_beams=8192, device=device, sensor_to_base_link=s2b),
        make_ekf=lambda opt: ReflectorEKFSLAM(opt, max_landmarks=max_landmarks, device=device, auto_grow=auto_grow),
        make_map_builder=lambda: MapBuilder(MapBuilderOptions(), max_points=16384, max_cells=2048 * 2048))


@dataclass
class ReplayLog:
    path: list = field(default_factory=list)                 # (stamp, x, y, theta) after every callback that publishes (ekf_path_)
    observations: list = field(default_factory=list)         # (obs time, centres) per processed scan
    match_poses: list = field(default_factory=list)          # MatchingResult.local_pose per scan (or None)


class Node:
    """The reference's ``Node`` minus ROS: same callbacks, same order of calls into the three components."""

    def __init__(self, meta: dict, backend: Backend):
        from .detect import ReflectorDetectOptions
        self.meta = meta
        self.backend = backend
        d = meta.get("detector", {})
        self.detector = backend.make_detector(ReflectorDetectOptions(**d), tuple(meta.get("sensor_to_base_link", (0.0, 0.0, 0.0))))
        self.slam = None
        self.map_builder = backend.make_map_builder()
        self.log = ReplayLog()

    def _ekf_options(self, time):
        from .ekf_slam import DIFF, OMNI, EKFOptions
        m = self.meta
        return EKFOptions(use_imu=False, init_time=float(time), init_pose=tuple(m.get("initial_pose", (0.0, 0.0, 0.0))),
                          map_path=m.get("map_path", ""), odom_model=DIFF if m.get("odom_model", "diff") == "diff" else OMNI,
                          linear_velocity_cov=float(m["linear_velocity_sigma"]) ** 2,        # the node squares the launch sigmas
                          angular_velocity_cov=float(m["angular_velocity_sigma"]) ** 2,      # (src/ros_node.cc:207-238)
                          observation_cov=float(m["observation_sigma"]) ** 2)

    def OdometryCallback(self, t, pose4, twist3):                                            # src/ros_node.cc:627-660
        from .ekf_slam import OdometryData
        px, py, qz, qw = (float(v) for v in pose4)
        vx, vy, wz = (float(v) for v in twist3)
        odom = OdometryData(float(t), (vx, vy, 0.0), (0.0, 0.0, wz), (px, py, 0.0), (qw, 0.0, 0.0, qz))
        self.detector.HandleOdometryData(odom)
        if self.slam is not None:
            self.slam.HandleOdometryMessage(odom)
            _, mu3, _ = self.slam.pose()                                                     # GetState(): the pose is all the node reads
            self.log.path.append((float(t), float(mu3[0]), float(mu3[1]), float(mu3[2])))

    def ScanCallback(self, scan):                                                            # src/ros_node.cc:420-558
        from .map_builder import RangeData
        if self.slam is None:
            self.slam = self.backend.make_ekf(self._ekf_options(scan.stamp))                 # the first scan is not processed (Q11)
            return
        obs = self.detector.HandleLaserScan(scan)
        self.slam.HandleObservationMessage(obs)
        _, mu3, _ = self.slam.pose()
        self.log.observations.append((obs.time_, np.array(obs.cloud_, np.float32)))
        if obs.cloud_.shape[0] > 0:                                                          # :524: publishes only with reflectors in view
            self.log.path.append((float(scan.stamp), float(mu3[0]), float(mu3[1]), float(mu3[2])))
        rd = self.detector.GetRangeData()
        res = self.map_builder.AddRangeData(float(scan.stamp), RangeData(rd.origin, rd.returns, np.zeros((0, 2), np.float32)),
                                            (float(mu3[0]), float(mu3[1]), float(mu3[2])))
        self.log.match_poses.append(None if res is None else np.array(res.local_pose))

    def SaveReflectorResult(self, filebase: str, reference_bytes: bool = True) -> str:       # src/ros_node.cc:75-140
        from .ekf_slam import save_map_txt
        if self.slam is None:
            return ""
        path = filebase + ".txt"
        save_map_txt(path, self.slam.GetState(), self.slam.GetGlobalMap(), reference_bytes=reference_bytes)
        return path

    def run(self, dump: Dump) -> ReplayLog:
        for kind, i in dump.events():
            if kind == "odom":
                self.OdometryCallback(dump.odom_t[i], dump.odom_pose[i], dump.odom_twist[i])
            else:
                self.ScanCallback(dump.scan(i))
        return self.log


def replay(dump: Dump, backend: Backend | None = None) -> Node:
    node = Node(dump.meta, backend or hip_backend())
    node.run(dump)
    return node


def pose_with_covariance(mu3, sigma3):
    """The fields Node::StatePosetoRosPose (src/ros_node.cc:796-819) fills from a state: -> (position (x, y, 0), orientation
    (x, y, z, w) = (0, 0, sin(theta / 2), cos(theta / 2)), covariance [36]) with exactly the entries 0, 1, 5, 6, 7, 11, 30, 31, 35 of the
    row-major 6 x 6 set, from sigma(0..2, 0..2) in that order (:809-817), and zeros elsewhere."""
    mu3 = np.asarray(mu3, np.float64).reshape(3)
    sg = np.asarray(sigma3, np.float64).reshape(3, 3)
    cov = np.zeros(36)
    cov[[0, 1, 5, 6, 7, 11, 30, 31, 35]] = sg.reshape(-1)
    return ((float(mu3[0]), float(mu3[1]), 0.0), (0.0, 0.0, math.sin(float(mu3[2]) / 2), math.cos(float(mu3[2]) / 2)), cov)


# ------------------------------------------------------------------------------------------------ the node of a fleet
@dataclass
class FleetBackend:
    """Factories of the three fleets ``FleetNode`` owns: what ``Backend`` is to ``Node``."""
    make_detector_fleet: object    # ([ReflectorDetectOptions], sensor_to_base_link [B, 3]) -> HandleOdometryData(member, msg) / submit / collect / range_data
    make_filter_fleet: object      # ([EKFOptions]) -> set_state / set_map / submit / poses / n / marker_ellipses / save_map_txt
                                   # (and track / take_track, for a FleetNode with pose_log=True only)
    make_map_builder: object       # (B) -> AddRangeData(times, range_datas, poses, members) / OccupancyGrids / SaveMap


def hip_fleet_backend(max_landmarks: int = 64, device: int = 0, max_beams: int = 8192, max_cells: int = 2048 * 2048,
                      max_rotations: int = 1024) -> FleetBackend:
    """The three HIP fleets.  ``max_rotations`` is the single handle's limit (rgrid_match: 1024): a lidar that sees 24 m needs about
    255 rotated scans for the node's 15 degree window, one more than ScanMatchFleet's default of 256 a little beyond that."""
    from .fleet import ReflectorEKFSLAMFleet
    from .fleet_detect import LaserReflectorDetectFleet
    from .map_builder import FleetMapBuilder, MapBuilderOptions
    return FleetBackend(
        make_detector_fleet=lambda opts, s2b: LaserReflectorDetectFleet(opts, max_beams=max_beams, device=device, sensor_to_base_link=s2b),
        make_filter_fleet=lambda opts: ReflectorEKFSLAMFleet(opts, max_landmarks=max_landmarks, device=device),
        make_map_builder=lambda B: FleetMapBuilder(B, MapBuilderOptions(), max_points=max_beams, max_cells=max_cells, max_rotations=max_rotations,
                                                           device=device))


@dataclass
class FleetReplayLog:
    """One member's part of a ``FleetNode``'s log."""
    path: list = field(default_factory=list)                 # (stamp, x, y, theta) of every scan that saw reflectors (:524)
    observations: list = field(default_factory=list)         # (obs time, centres) per processed scan
    match_poses: list = field(default_factory=list)          # MatchingResult.local_pose per processed scan (or None)
    match_results: list = field(default_factory=list)        # the MatchingResult itself (or None)
    mapper_inputs: list = field(default_factory=list)        # (stamp, RangeData, (x, y, yaw)): exactly what the mapper was given
    skipped: list = field(default_factory=list)              # (stamp, detector status) of every scan the detector refused
    pose_log: list = field(default_factory=list)             # FleetNode(pose_log=True): (stamp, x, y, theta, sigma3x3) after every odometry
                                                             # message of a member whose filter exists and every scan that saw reflectors,
                                                             # in message order: ``Node``'s ``log.path`` with the covariance beside it


class FleetNode:
    """The reference's default-build ``Node`` (src/ros_node.cc:420-660) for B robots over the three fleets: member m is what a ``Node``
    made from ``metas[m]`` is, and a ``tick`` gives every member the messages ``Node.OdometryCallback`` / ``Node.ScanCallback`` would
    get -- its odometry in the order given, then its scan -- with a number of launches and synchronisations that does not grow with B:

        odometry  -> the detector fleet always; an ``odom_event`` of the tick's ONE ``fleet.submit`` only for a member whose filter
                     exists (:630-638)
        a member's first scan only creates its filter: set_state(member, stamp, initial_pose, zeros, vt = 0); the scan itself is
                     not processed (:424-441)
        the other scans: detector submit / collect -> ``scan_events`` of the status-0 scans, with the odometry events, in ONE
                     ``fleet.submit`` -> ``poses()`` -> ``range_data(members)`` -> ONE ``AddRangeData(stamps, range datas, poses,
                     members)`` with the pose after the update (:546-552)

    ``map_path`` of a meta is served by the filter fleet's ONE shared map (``load_map_txt`` -> ``set_map`` for the members that name
    it): two different non-empty paths in one fleet raise ValueError.  A scan the detector refuses (status != 0) is logged in
    ``skipped`` and left out for that member -- the reference exits there.  A scan with more than ``fleet.MAX_OBS`` centres raises
    ValueError before anything is submitted to the filter: include/rfleet.h puts such scans out of scope on a fleet that has not
    switched wide scans on.

    ``wide_scans=True`` switches them on (``fleet.wide_scans()``): scans of up to ``fleet.MAX_OBS_WIDE`` centres -- as many as the
    detector fleets hand over -- go through, in the tick's ONE submit, which then launches k_fleet_step_wide; more than that raises
    ValueError.  With ``wide_scans=False`` no wide call reaches the backend.

    ``pose_log=True``: the pose log after every odometry message (``Node`` keeps one in ``log.path``) is opt-in and costs no
    synchronisation per message: the filter fleet's pose track is switched on (``fleet.track()``), the tick's ONE launch writes a
    record per message, and ``logs[m].pose_log`` is filled from ``fleet.take_track()`` where the tick synchronises anyway (behind
    ``poses()``) and once more at the end of ``run`` (``harvest_pose_log``); a tick of odometry only adds no synchronisation.  With
    ``pose_log=False`` no tracking call reaches the backend.

    OUT OF SCOPE: the USE_GPS ordering of ScanCallback (:450-508: predict, match, then the update with the pose fix);
    PointCloudCallback; a device-to-device route from the detector's returns into rgrid_batch_add_range_data (the range
    data crosses the host once per tick, DESIGN.md 10.11 "not built")."""

    def __init__(self, metas, backend: FleetBackend | None = None, pose_log: bool = False, wide_scans: bool = False):
        from .detect import ReflectorDetectOptions
        from .ekf_slam import load_map_txt
        self.metas = [dict(m) for m in metas]
        self.B = len(self.metas)
        self.backend = backend or hip_fleet_backend()
        paths = sorted({m.get("map_path", "") for m in self.metas} - {""})
        if len(paths) > 1:
            raise ValueError(f"a fleet has one shared map; the metas name {len(paths)}: {paths}")
        s2b = np.array([tuple(m.get("sensor_to_base_link", (0.0, 0.0, 0.0))) for m in self.metas], np.float64).reshape(self.B, 3)
        self.detector = self.backend.make_detector_fleet([ReflectorDetectOptions(**m.get("detector", {})) for m in self.metas], s2b)
        self.fleet = self.backend.make_filter_fleet([self._ekf_options(m) for m in self.metas])
        self.map_builder = self.backend.make_map_builder(self.B)
        if paths:
            loaded = load_map_txt(paths[0])
            if loaded.reflector_map_.shape[0] > 0:
                self.fleet.set_map(loaded.reflector_map_, loaded.reflector_map_coviarance_,
                                   [i for i, m in enumerate(self.metas) if m.get("map_path", "") == paths[0]])
        self.has_filter = [False] * self.B
        self.logs = [FleetReplayLog() for _ in range(self.B)]
        self.pose_log = bool(pose_log)
        if self.pose_log:
            self.fleet.track(True)
        self.wide_scans = bool(wide_scans)
        if self.wide_scans:
            self.fleet.wide_scans(True)

    @staticmethod
    def _ekf_options(m):
        from .ekf_slam import DIFF, OMNI, EKFOptions
        return EKFOptions(use_imu=False, init_time=0.0, init_pose=tuple(m.get("initial_pose", (0.0, 0.0, 0.0))), map_path="",
                          odom_model=DIFF if m.get("odom_model", "diff") == "diff" else OMNI,
                          linear_velocity_cov=float(m["linear_velocity_sigma"]) ** 2,        # the node squares the launch sigmas
                          angular_velocity_cov=float(m["angular_velocity_sigma"]) ** 2,      # (src/ros_node.cc:207-238)
                          observation_cov=float(m["observation_sigma"]) ** 2)

    def tick(self, odometry=(), scans=()):
        """odometry = [(member, t, pose4, twist3), ...] (pose4 = position x, y, orientation z, w; twist3 = linear x, y, angular z);
        scans = [(member, LaserScan), ...], at most one per member.  -> the members whose scan reached the mapper."""
        from . import fleet as F
        from .ekf_slam import OdometryData
        from .fleet_detect import scan_events
        from .map_builder import RangeData
        scans = [(int(m), sc) for m, sc in scans]
        listed = [m for m, _ in scans]
        if len(set(listed)) != len(listed) or any(not 0 <= m < self.B for m in listed):
            raise ValueError("at most one scan per member, and a member is a number below B")
        events = []
        for member, t, pose4, twist3 in odometry:                                            # src/ros_node.cc:627-660
            member = int(member)
            px, py, qz, qw = (float(v) for v in pose4)
            vx, vy, wz = (float(v) for v in twist3)
            self.detector.HandleOdometryData(member, OdometryData(float(t), (vx, vy, 0.0), (0.0, 0.0, wz), (px, py, 0.0), (qw, 0.0, 0.0, qz)))
            if self.has_filter[member]:
                events.append(F.odom_event(member, t, vx, vy, wz))
        first = [(m, sc) for m, sc in scans if not self.has_filter[m]]
        later = [(m, sc) for m, sc in scans if self.has_filter[m]]
        kept = []
        if later:
            observations = self.detector.detect(later)
            for (m, sc), (status, obs) in zip(later, observations):
                if status != 0:
                    self.logs[m].skipped.append((float(sc.stamp), int(status)))
                elif obs.cloud_.shape[0] > (F.MAX_OBS_WIDE if self.wide_scans else F.MAX_OBS):
                    raise ValueError(f"member {m}: {obs.cloud_.shape[0]} centres in one scan, the fleet filter takes "
                                     f"{F.MAX_OBS_WIDE if self.wide_scans else F.MAX_OBS}")
                else:
                    kept.append((m, sc, obs))
            events += scan_events(later, observations)
        if events:
            self.fleet.submit(events)
        for m, sc in first:                                                                  # :424-441: the first scan is not processed (Q11)
            self.fleet.set_state(m, float(sc.stamp), np.array(self.metas[m].get("initial_pose", (0.0, 0.0, 0.0)), np.float64),
                                 np.zeros((3, 3)), vt=np.zeros(3))
            self.has_filter[m] = True
        if not kept:
            return []
        members = [m for m, _, _ in kept]
        _, mu, _ = self.fleet.poses()
        if self.pose_log:
            self.harvest_pose_log()                                                          # (the tick has synchronised: nothing waits)
        range_datas = self.detector.range_data(members)
        stamps = [float(sc.stamp) for _, sc, _ in kept]
        poses = [(float(mu[m, 0]), float(mu[m, 1]), float(mu[m, 2])) for m in members]
        rds = [RangeData(rd.origin, rd.returns, np.zeros((0, 2), np.float32)) for rd in range_datas]
        results = self.map_builder.AddRangeData(stamps, rds, poses, members)
        for (m, sc, obs), stamp, rd, pose, res in zip(kept, stamps, rds, poses, results):
            log = self.logs[m]
            log.observations.append((obs.time_, np.array(obs.cloud_, np.float32)))
            if obs.cloud_.shape[0] > 0:                                                      # :524: publishes only with reflectors in view
                log.path.append((stamp,) + pose)
            log.mapper_inputs.append((stamp, rd, pose))
            log.match_poses.append(None if res is None else np.array(res.local_pose))
            log.match_results.append(res)
        return members

    def harvest_pose_log(self):
        """Moves the filter fleet's pose track into ``logs[m].pose_log``: every odometry record (a dropped one too: the node publishes
        the unchanged pose, :640-660) and every scan record with reflectors in view (:524).  Synchronises."""
        for m, tr in enumerate(self.fleet.take_track()):
            log = self.logs[m].pose_log
            for r in range(len(tr)):
                if tr.kind[r] == 0 or tr.K[r] > 0:
                    log.append((float(tr.t[r]), float(tr.mu[r, 0]), float(tr.mu[r, 1]), float(tr.mu[r, 2]), tr.sigma[r].copy()))

    # -- what the node hands out ------------------------------------------------------------------
    def markers(self, members=None):
        """ReflectorToRosMarkers' ellipses of the listed members (src/ros_node.cc:736-791), one launch."""
        return self.fleet.marker_ellipses(members)

    def occupancy_grids(self, members=None):
        """Node::PublishMap's message fields of the listed members (None where a member has no submap), one launch."""
        return self.map_builder.OccupancyGrids(members)

    def SaveReflectorResult(self, member: int, filebase: str, reference_bytes: bool = True) -> str:   # src/ros_node.cc:75-140
        if not self.has_filter[int(member)]:
            return ""
        path = filebase + ".txt"
        self.fleet.save_map_txt(int(member), path, reference_bytes=reference_bytes)
        return path

    def SaveMap(self, member: int, filebase: str):                                           # src/ros_node.cc:947-1001
        return self.map_builder.SaveMap(int(member), filebase)

    def run(self, dumps, start_tick=None):
        """Replays B ``rekf-dump-v1`` dumps: member m's k-th segment -- its odometry since its previous scan and its k-th scan -- goes
        into tick ``start_tick[m] + k`` (default 0); odometry behind its last scan into the tick after it.  -> the logs."""
        dumps = list(dumps)
        if len(dumps) != self.B:
            raise ValueError("one dump per member")
        start = [0] * self.B if start_tick is None else [int(v) for v in start_tick]
        ticks = {}
        for m, d in enumerate(dumps):
            k, od = start[m], []
            for kind, i in d.events():
                if kind == "odom":
                    od.append((m, d.odom_t[i], d.odom_pose[i], d.odom_twist[i]))
                else:
                    ticks.setdefault(k, ([], []))
                    ticks[k][0].extend(od)
                    ticks[k][1].append((m, d.scan(i)))
                    k, od = k + 1, []
            if od:
                ticks.setdefault(k, ([], []))[0].extend(od)
        for k in sorted(ticks):
            self.tick(*ticks[k])
        if self.pose_log:
            self.harvest_pose_log()
        return self.logs


def replay_fleet(dumps, backend: FleetBackend | None = None, start_tick=None) -> FleetNode:
    dumps = list(dumps)
    node = FleetNode([d.meta for d in dumps], backend)
    node.run(dumps, start_tick)
    return node
