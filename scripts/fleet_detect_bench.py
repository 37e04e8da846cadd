"""Fleet detection, measured: B robots, one 3600-beam scan per robot per tick, odometry fed to every robot,

* ``batch``:   one LaserReflectorDetectFleet.detect per tick (ONE launch of k_det2d_batch, one workgroup per scan); the scans are
  copied into the staging area by the call;
* ``staged``:  the same, with every scan received straight into its member's staging slice (read in place: the copy a driver
  that writes there never pays; the write into the slice is outside the timed region);
* ``handles``: the same scans through B LaserReflectorDetect handles, round robin on this thread -- the only way to serve a
  fleet without the batch.

All legs run in the same process, alternating, --reps repetitions each; every repetition warms up and then times --ticks ticks with
the host clock around calls that each end in a synchronisation (collect / the handle's own wait).  Prints ONE JSON line (and
writes it to --out): scans/s as min / median / max, us per tick, the share of the batch tick that is host copy
((batch - staged) / batch, medians), and the SHA-256 of the sources it was measured on.

  python scripts/fleet_detect_bench.py --out profiles/fleet_detect_bench.json
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/fleet_detect_bench.py --only-batch 256 --reps 1   (k_det2d_batch's own time)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SOURCES = ["include/rdet.h", "reflector_ekf_slam_amd/csrc/det2d_batch.hip", "reflector_ekf_slam_amd/csrc/det_batch_host.h", "reflector_ekf_slam_amd/csrc/det_batch_dev.h",
           "reflector_ekf_slam_amd/csrc/det2d.hip",
           "reflector_ekf_slam_amd/fleet_detect.py", "reflector_ekf_slam_amd/detect.py", "scripts/fleet_detect_bench.py"]
N_POSES = 16          # distinct poses (scans); member b of tick k sees scan (b + k) % N_POSES
N_BEAMS = 3600
S2B = (0.13686, 0.0, 0.0)


def make_scans():
    from reflector_ekf_slam_amd import synth
    from reflector_ekf_slam_amd.detect import LaserScan
    rng = np.random.Generator(np.random.PCG64(4100))
    lms = synth.make_world(synth.C2, rng)
    lo, hi = lms.min(0), lms.max(0)
    out = []
    for _ in range(N_POSES):
        pose = (float(rng.uniform(lo[0], hi[0])), float(rng.uniform(lo[1], hi[1])), float(rng.uniform(-math.pi, math.pi)))
        d = synth.make_laser_scan(lms, pose, 0.0, rng, n_beams=N_BEAMS)
        out.append(LaserScan(d["stamp"], d["angle_min"], d["angle_max"], d["angle_increment"], d["scan_time"], d["range_min"],
                             d["range_max"], np.ascontiguousarray(d["ranges"], np.float32), np.ascontiguousarray(d["intensities"], np.float32)))
    return out


def odom_msg(t, b):
    from reflector_ekf_slam_amd import OdometryData
    th = 0.3 * t + 0.01 * b
    return OdometryData(t, (1.0, 0.0, 0.0), (0.0, 0.0, 0.3), (t, 0.1 * b, 0.0), (math.cos(th / 2), 0.0, 0.0, math.sin(th / 2)))


def stats(rates):
    r = sorted(rates)
    return {"min": r[0], "median": float(np.median(r)), "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--handle-sizes", type=int, nargs="*", default=[4, 64])
    ap.add_argument("--only-batch", type=int, default=0, help="run the batch legs at this size only (profiling runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.only_batch:
        args.batch_sizes, args.handle_sizes = [args.only_batch], []

    import copy
    from reflector_ekf_slam_amd import LaserReflectorDetectFleet
    from reflector_ekf_slam_amd.detect import LaserReflectorDetect, ReflectorDetectOptions
    base = make_scans()
    total = args.warmup + args.ticks
    result = {"workload": f"B members, one {N_BEAMS}-beam synth.make_laser_scan scan per member per tick ({N_POSES} distinct poses in the C2 "
                          "world, member b of tick k sees pose (b + k) mod 16), two odometry samples per member per tick",
              "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps, "unit": "scans/s (aggregate, one GPU, one host thread)",
              "batch": {}, "staged": {}, "handles": {}}

    def scan_at(b, k, t):
        s = copy.copy(base[(b + k) % N_POSES])
        s.stamp = t
        return s

    for B in sorted(set(args.batch_sizes) | set(args.handle_sizes)):
        fl = handles = None
        if B in args.batch_sizes:
            fl = LaserReflectorDetectFleet([ReflectorDetectOptions()] * B, max_beams=N_BEAMS, sensor_to_base_link=S2B)
            views = [fl.staging(b) for b in range(B)]
        if B in args.handle_sizes:
            handles = [LaserReflectorDetect(ReflectorDetectOptions(), max_beams=N_BEAMS, sensor_to_base_link=S2B) for b in range(B)]
        rb, rs, rh = [], [], []
        clock = 1.0                       # the legs share one time line: every tick is 0.1 s after the one before, whoever runs it

        def tick_batch(k, t, staged):
            for b in range(B):
                fl.HandleOdometryData(b, odom_msg(t - 0.06, b)); fl.HandleOdometryData(b, odom_msg(t - 0.01, b))
            scans = []
            for b in range(B):
                s = scan_at(b, k, t)
                if staged:
                    s.ranges, s.intensities = views[b][0][:N_BEAMS], views[b][1][:N_BEAMS]
                scans.append((b, s))
            return scans

        for _ in range(args.reps):
            for leg in ("batch", "staged", "handles"):
                if leg != "handles" and fl is None or leg == "handles" and handles is None:
                    continue
                dt = 0.0
                for k in range(total):
                    clock += 0.1
                    if leg == "handles":
                        msgs = [scan_at(b, k, clock) for b in range(B)]
                        for b, g in enumerate(handles):
                            g.HandleOdometryData(odom_msg(clock - 0.06, b)); g.HandleOdometryData(odom_msg(clock - 0.01, b))
                        t0 = time.perf_counter()
                        out = [g.HandleLaserScan(m) for g, m in zip(handles, msgs)]
                        t1 = time.perf_counter()
                    else:
                        scans = tick_batch(k, clock, leg == "staged")
                        if leg == "staged":                       # the driver's write into the slice: not the detector's time
                            for b in range(B):
                                src = base[(b + k) % N_POSES]
                                views[b][0][:N_BEAMS] = src.ranges; views[b][1][:N_BEAMS] = src.intensities
                        t0 = time.perf_counter()
                        out = fl.detect(scans)
                        t1 = time.perf_counter()
                        assert all(st == 0 for st, _ in out)
                    if k >= args.warmup:
                        dt += t1 - t0
                {"batch": rb, "staged": rs, "handles": rh}[leg].append(B * args.ticks / dt)
        if fl is not None:
            result["batch"][str(B)] = dict(stats(rb), us_per_tick=1e6 * B / float(np.median(rb)))
            result["staged"][str(B)] = dict(stats(rs), us_per_tick=1e6 * B / float(np.median(rs)))
            ub, us = result["batch"][str(B)]["us_per_tick"], result["staged"][str(B)]["us_per_tick"]
            result["batch"][str(B)]["host_copy_us_per_tick"] = ub - us
            result["batch"][str(B)]["host_copy_share"] = (ub - us) / ub
        if handles is not None:
            result["handles"][str(B)] = dict(stats(rh), us_per_tick=1e6 * B / float(np.median(rh)))
        if fl is not None:
            fl.close()
        for g in handles or []:
            g.close()

    f, h = result["batch"], result["handles"]
    if "64" in f and "64" in h:
        result["batch64_min_over_handles64_max"] = f["64"]["min"] / h["64"]["max"]
        result["speedup_claimed"] = bool(f["64"]["min"] > h["64"]["max"])
    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
