"""Fleet 3D detection, measured: B robots, one 28 800-point 16-ring sweep of the C4 world per robot per tick,

* ``batch``:   one PointCloudReflectorDetectFleet.detect per tick (ONE launch of k_det3d_batch, one workgroup per cloud); the clouds are
  copied into the staging area by the call;
* ``staged``:  the same, with every cloud written straight into its member's staging slice (read in place: the copy a driver that
  receives there never pays; the write into the slice is outside the timed region);
* ``handles``: the same clouds through B PointCloudReflectorDetect handles, round robin on this thread -- the only way to serve a fleet
  without the batch.

Every (size, repetition, leg) is a PROCESS OF ITS OWN under its own ``timeout -k 10``: this script starts them one after the other, the
legs alternating, and stops at the first one that fails.  A leg warms up, then times --ticks ticks with the host clock around calls that
each end in a synchronisation, and prints one JSON line with its scans/s and the SHA-256 of the centres of its last tick; the batch and
staged legs of a repetition must agree on that hash with the handles leg (same clouds, same bits).  The parent writes scans/s as
min / median / max per leg and size to --out.

  python scripts/fleet_detect3d_bench.py --out profiles/fleet_detect3d_bench.json
  python scripts/fleet_detect3d_bench.py --leg batch --size 64          (one leg, in this process)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SOURCES = ["include/rdet.h", "reflector_ekf_slam_amd/csrc/det3d_batch.hip", "reflector_ekf_slam_amd/csrc/det_batch_host.h", "reflector_ekf_slam_amd/csrc/det_batch_dev.h",
           "reflector_ekf_slam_amd/csrc/det3d.hip",
           "reflector_ekf_slam_amd/fleet_detect.py", "reflector_ekf_slam_amd/detect.py", "scripts/fleet_detect3d_bench.py"]
N_POSES = 16          # distinct poses (clouds); member b of tick k sees cloud (b + k) % N_POSES
LEGS = ("batch", "staged", "handles")


def make_clouds():
    from reflector_ekf_slam_amd import synth
    rng = np.random.Generator(np.random.PCG64(4103))
    lms = synth.make_world(synth.C4, rng)
    lo, hi = lms.min(0), lms.max(0)
    out = []
    for _ in range(N_POSES):
        pose = (float(rng.uniform(lo[0] + 5, hi[0] - 5)), float(rng.uniform(lo[1] + 5, hi[1] - 5)), float(rng.uniform(-math.pi, math.pi)))
        out.append(np.ascontiguousarray(synth.make_point_cloud(lms, pose, rng), np.float32))
    return out


def run_leg(leg, B, ticks, warmup):
    from reflector_ekf_slam_amd import PointCloudReflectorDetectFleet
    from reflector_ekf_slam_amd.detect import PointCloudOptions, PointCloudReflectorDetect
    base = make_clouds()
    n_pts = base[0].shape[0]
    assert all(c.shape == (n_pts, 4) for c in base)
    if leg == "handles":
        handles = [PointCloudReflectorDetect(PointCloudOptions(), max_points=n_pts) for _ in range(B)]
    else:
        fl = PointCloudReflectorDetectFleet([PointCloudOptions()] * B, max_points=n_pts)
        views = [fl.staging(b) for b in range(B)]
    dt, last = 0.0, None
    for k in range(warmup + ticks):
        t = 1.0 + 0.1 * k
        if leg == "handles":
            t0 = time.perf_counter()
            out = [g.HandlePointCloud(t, base[(b + k) % N_POSES]).cloud_ for b, g in enumerate(handles)]
            t1 = time.perf_counter()
        else:
            if leg == "staged":                                   # the driver's write into the slice: not the detector's time
                for b in range(B):
                    views[b][:n_pts] = base[(b + k) % N_POSES]
                clouds = [(b, t, views[b][:n_pts]) for b in range(B)]
            else:
                clouds = [(b, t, base[(b + k) % N_POSES]) for b in range(B)]
            t0 = time.perf_counter()
            res = fl.detect(clouds)
            t1 = time.perf_counter()
            assert all(st == 0 for st, _ in res), [st for st, _ in res]
            out = [ob.cloud_ for _, ob in res]
        if k >= warmup:
            dt += t1 - t0
        last = out
    h = hashlib.sha256()
    for c in last:
        h.update(np.int32(c.shape[0]).tobytes()); h.update(np.ascontiguousarray(c).tobytes())
    return {"leg": leg, "B": B, "scans_per_s": B * ticks / dt, "us_per_tick": 1e6 * dt / ticks, "centres_sha256": h.hexdigest(),
            "centres_last_tick": int(sum(c.shape[0] for c in last)), "points_per_cloud": n_pts}


def stats(rates):
    r = sorted(rates)
    return {"min": r[0], "median": float(np.median(r)), "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--leg", choices=LEGS, default=None, help="run this one leg in this process and print its JSON line")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds a leg's process may take")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(run_leg(args.leg, args.size, args.ticks, args.warmup)))
        return

    result = {"workload": f"B members, one 28 800-point synth.make_point_cloud sweep per member per tick ({N_POSES} distinct poses in the C4 "
                          "world, member b of tick k sees pose (b + k) mod 16)",
              "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps, "unit": "scans/s (aggregate, one GPU, one host thread)",
              "batch": {}, "staged": {}, "handles": {}}
    for B in args.sizes:
        rates = {leg: [] for leg in LEGS}
        per_tick = {leg: [] for leg in LEGS}
        for rep in range(args.reps):
            hashes = {}
            for leg in LEGS:                                          # the legs alternate: each its own process, its own time limit
                cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--size", str(B),
                       "--ticks", str(args.ticks), "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:
                    sys.exit(f"leg {leg} B={B} rep={rep}: exit status {p.returncode}; nothing further is started")
                r = json.loads(p.stdout.strip().splitlines()[-1])
                rates[leg].append(r["scans_per_s"]); per_tick[leg].append(r["us_per_tick"])
                hashes[leg] = r["centres_sha256"]
                print(f"B={B} rep={rep} {leg}: {r['scans_per_s']:.0f} scans/s, {r['us_per_tick']:.0f} us per tick", file=sys.stderr, flush=True)
            if len(set(hashes.values())) != 1:
                sys.exit(f"B={B} rep={rep}: the legs' centres differ: {hashes}")
        for leg in LEGS:
            result[leg][str(B)] = dict(stats(rates[leg]), us_per_tick=float(np.median(per_tick[leg])))
        ub, us = result["batch"][str(B)]["us_per_tick"], result["staged"][str(B)]["us_per_tick"]
        result["batch"][str(B)]["host_copy_us_per_tick"] = ub - us
    f, h = result["batch"], result["handles"]
    if "64" in f and "64" in h:
        result["batch64_min_over_handles64_max"] = f["64"]["min"] / h["64"]["max"]
        result["speedup_claimed"] = bool(f["64"]["min"] > h["64"]["max"])
    result["centres_equal_across_legs"] = True
    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
