"""The 2D fleet tick, measured with and without the host between the detector's launch and the filter's: B robots, one 3600-beam scan
per robot per tick, C2-sized filter members (capacity 128), two odometry messages per robot per tick,

* ``composed``: detect (submit + collect: the host waits for the detector's stream and copies the centres out) -> scan_events ->
  ReflectorEKFSLAMFleet.submit (the centres copied into the ring segment) -> poses();
* ``linked``:   det.submit -> det.link() -> submit_linked (k_fleet_bind moves the centres on the device) -> poses() (the tick's one
  wait) -> det.collect() (returns at once; it is part of the tick because a host that wants the range data calls it).

Both legs run on the same build, in one process, alternating, --reps repetitions each, on detector and filter fleets of their own
that see the same messages; every repetition warms up and then times --ticks ticks with the host clock around the tick.  Member b
stands still at one of the poses of scripts/fleet_detect_bench.py's C2 world whose scan yields at most 32 centres, so both filters
take the narrow launch and reach a steady state.  Prints ONE JSON line (and writes it to --out): us per tick as min / median / max per
leg and size, composed minimum over linked maximum (> 1: every linked repetition beat every composed one), the largest difference of
the two filters' poses at the end (they see the same bits: 0), and the SHA-256 of the sources it was measured on.

  python scripts/fleet_link_bench.py --out profiles/fleet_link_bench.json
"""
from __future__ import annotations

import argparse
import copy
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

SOURCES = ["include/rlink.h", "include/rdet.h", "include/rfleet.h", "reflector_ekf_slam_amd/csrc/det2d_batch.hip", "reflector_ekf_slam_amd/csrc/det_batch_host.h", "reflector_ekf_slam_amd/csrc/det_batch_dev.h",
           "reflector_ekf_slam_amd/csrc/fleet_link.h", "reflector_ekf_slam_amd/csrc/fleet_link.hip", "reflector_ekf_slam_amd/csrc/fleet_host.h",
           "reflector_ekf_slam_amd/csrc/rfleet_api.hip", "reflector_ekf_slam_amd/fleet.py", "reflector_ekf_slam_amd/fleet_detect.py",
           "scripts/fleet_detect_bench.py", "scripts/fleet_link_bench.py"]
MAX_OBS = 32


def stats(us):
    r = sorted(us)
    return {"min": r[0], "median": float(np.median(r)), "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import fleet_detect_bench as FD
    from reflector_ekf_slam_amd import (EKFOptions, LaserReflectorDetectFleet, OdometryData, ReflectorEKFSLAMFleet, linked_scan_events,
                                        scan_events)
    from reflector_ekf_slam_amd.detect import ReflectorDetectOptions
    from reflector_ekf_slam_amd.fleet import odom_event

    def detector(B):
        return LaserReflectorDetectFleet([ReflectorDetectOptions()] * B, max_beams=FD.N_BEAMS, sensor_to_base_link=FD.S2B)

    pool = FD.make_scans()
    probe = detector(len(pool))
    counts = [obs.cloud_.shape[0] for _, obs in probe.detect(list(enumerate(pool)))]
    probe.close()
    pool = [s for s, k in zip(pool, counts) if 0 < k <= MAX_OBS]
    kept = [k for k in counts if 0 < k <= MAX_OBS]
    total = args.warmup + args.ticks
    result = {"workload": f"B members standing still, one {FD.N_BEAMS}-beam synth.make_laser_scan scan per member per tick (member b sees pose b mod "
                          f"{len(pool)} of the C2 world: {min(kept)} to {max(kept)} centres), filter capacity 128, two odometry messages per member per tick",
              "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps,
              "unit": "us per tick (host clock around a tick that ends in the filter's synchronisation)", "composed": {}, "linked": {},
              "composed_min_over_linked_max": {}, "linked_is_a_speed_up": {}, "max_abs_pose_diff": {}}
    still = OdometryData(0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))

    for B in args.sizes:
        det = {"composed": detector(B), "linked": detector(B)}
        flt = {leg: ReflectorEKFSLAMFleet([EKFOptions(init_time=0.0)] * B, max_landmarks=128) for leg in det}
        clock = {leg: 1.0 for leg in det}
        us = {leg: [] for leg in det}
        for _ in range(args.reps):
            for leg in ("composed", "linked"):
                d, f = det[leg], flt[leg]
                dt = 0.0
                for k in range(total):
                    clock[leg] += 0.1
                    t = clock[leg]
                    events, scans = [], []
                    for b in range(B):
                        for back in (0.06, 0.01):
                            msg = copy.copy(still)
                            msg.time = t - back
                            d.HandleOdometryData(b, msg)
                            events.append(odom_event(b, t - back, 0.0, 0.0, 0.0))
                        s = copy.copy(pool[b % len(pool)])
                        s.stamp = t
                        scans.append((b, s))
                    t0 = time.perf_counter()
                    if leg == "composed":
                        obs = d.detect(scans)
                        f.submit(events + scan_events(scans, obs))
                        f.poses()
                    else:
                        d.submit(scans)
                        link = d.link()
                        f.submit_linked(events + linked_scan_events(link), link)
                        f.poses()
                        obs = d.collect()
                    t1 = time.perf_counter()
                    assert all(st == 0 for st, _ in obs)
                    if k >= args.warmup:
                        dt += t1 - t0
                us[leg].append(1e6 * dt / args.ticks)
        taken, status, _ = flt["linked"].link_status()
        assert not status.any() and taken.tolist() == [kept[b % len(pool)] for b in range(B)]
        assert not flt["linked"].flags().any() and not flt["composed"].flags().any()
        result["composed"][str(B)], result["linked"][str(B)] = stats(us["composed"]), stats(us["linked"])
        ratio = result["composed"][str(B)]["min"] / result["linked"][str(B)]["max"]
        result["composed_min_over_linked_max"][str(B)] = ratio
        result["linked_is_a_speed_up"][str(B)] = bool(ratio > 1.0)
        result["max_abs_pose_diff"][str(B)] = float(np.abs(flt["linked"].poses()[1] - flt["composed"].poses()[1]).max())
        for h in (*det.values(), *flt.values()):
            h.close()

    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
