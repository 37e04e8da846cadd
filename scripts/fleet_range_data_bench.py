"""The link between the fleet detector and the fleet mapper, measured: B robots, one 3600-beam synth.make_laser_scan scan per robot,

* ``range`` leg: after one ``detect`` per repetition, ``LaserReflectorDetectFleet.range_data()`` -- ONE launch of
  k_det2d_batch_range_data and one synchronisation -- against B x ``GetRangeData(member)`` (two C calls and one blocking copy per
  member) on the same handle.  A warm-up, then --reps repetitions, the two alternating; a repetition times --calls calls of each with
  the host clock (every call ends in a synchronisation) and the rows of both must be the same bytes.  us per call: the whole fleet's
  range data once.
* ``node`` leg: a ``node_replay.FleetNode`` tick of B robots (detector, filter and mapper fleets) against the same messages through B
  single ``Node``s over ``hip_backend()``, on dumps of --scans scans of 1440 beams (four distinct robots, member b replays robot
  b mod 4).  The first scans only create the filters and the second create the submaps; the ticks behind them are timed.  us per tick
  of the whole fleet.

Every step -- the ``range`` leg of one size, one side of one repetition of the ``node`` leg -- is a PROCESS OF ITS OWN under its own
``timeout -k 10``; this script starts them one after the other and stops at the first that fails.  The parent writes min / median /
max per leg and size to --out; a size that was not run is absent ("unmeasured").

  python scripts/fleet_range_data_bench.py --out profiles/fleet_range_data_bench.json
  python scripts/fleet_range_data_bench.py --leg range --size 64          (one step, in this process)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SOURCES = ["include/rdet.h", "reflector_ekf_slam_amd/csrc/det2d_batch.hip", "reflector_ekf_slam_amd/csrc/det_batch_host.h", "reflector_ekf_slam_amd/csrc/det_batch_dev.h",
           "reflector_ekf_slam_amd/fleet_detect.py",
           "reflector_ekf_slam_amd/node_replay.py", "reflector_ekf_slam_amd/map_builder.py", "scripts/fleet_range_data_bench.py"]
N_BEAMS = 3600
N_POSES = 8
STEPS = ("range", "node_fleet", "node_single")


def make_scans():
    from reflector_ekf_slam_amd import synth
    from reflector_ekf_slam_amd.detect import LaserScan
    rng = np.random.Generator(np.random.PCG64(4211))
    lms = synth.make_world(synth.C2, rng)
    lo, hi = lms.min(0), lms.max(0)
    out = []
    for _ in range(N_POSES):
        pose = (float(rng.uniform(lo[0] + 5, hi[0] - 5)), float(rng.uniform(lo[1] + 5, hi[1] - 5)), float(rng.uniform(-3.0, 3.0)))
        s = synth.make_laser_scan(lms, pose, 5.0, rng, n_beams=N_BEAMS)
        out.append(LaserScan(s["stamp"], s["angle_min"], s["angle_max"], s["angle_increment"], s["scan_time"], s["range_min"], s["range_max"],
                             s["ranges"], s["intensities"]))
    return out


def run_range(B, reps, calls):
    import dataclasses
    from reflector_ekf_slam_amd import LaserReflectorDetectFleet
    from reflector_ekf_slam_amd.detect import ReflectorDetectOptions
    base = make_scans()
    fl = LaserReflectorDetectFleet([ReflectorDetectOptions()] * B, max_beams=N_BEAMS, sensor_to_base_link=(0.13686, 0.0, 0.0))
    batch_us, member_us, rows = [], [], 0
    for rep in range(reps + 1):                                       # (repetition 0 is the warm-up)
        res = fl.detect([(b, dataclasses.replace(base[(b + rep) % N_POSES], stamp=5.0 + 0.1 * rep)) for b in range(B)])
        assert all(st == 0 for st, _ in res)
        t0 = time.perf_counter()
        for _ in range(calls):
            got = fl.range_data()
        t1 = time.perf_counter()
        for _ in range(calls):
            one = [fl.GetRangeData(b) for b in range(B)]
        t2 = time.perf_counter()
        assert all(g.returns.tobytes() == o.returns.tobytes() and g.origin.tobytes() == o.origin.tobytes() for g, o in zip(got, one))
        rows = int(sum(g.returns.shape[0] for g in got))
        if rep:
            batch_us.append(1e6 * (t1 - t0) / calls)
            member_us.append(1e6 * (t2 - t1) / calls)
    fl.close()
    return {"step": "range", "B": B, "batch_us": batch_us, "per_member_us": member_us, "rows_per_call": rows}


def make_dumps(scans):
    from reflector_ekf_slam_amd import synth
    from reflector_ekf_slam_amd.node_replay import synth_dump
    d = tempfile.mkdtemp(prefix="fleet_range_data_bench_")
    return [synth_dump(os.path.join(d, f"robot{i}.npz"), synth.SessionConfig(f"bench{i}", 40, 12, synth.DIFF, seed=31 + i, speed=1.0, row_spacing=6.0),
                       max_scans=scans, n_beams=1440) for i in range(4)]


def segments(d):
    """[(odometry [(t, pose4, twist3)], scan)] of a dump, as FleetNode.run cuts it."""
    out, od = [], []
    for kind, i in d.events():
        if kind == "odom":
            od.append((d.odom_t[i], d.odom_pose[i], d.odom_twist[i]))
        else:
            out.append((od, d.scan(i)))
            od = []
    return out


def run_node(step, B, scans, warm):
    from reflector_ekf_slam_amd import node_replay as NR
    dumps = make_dumps(scans)
    segs = [segments(d) for d in dumps]
    metas = [dumps[b % 4].meta for b in range(B)]
    us = []
    if step == "node_fleet":
        node = NR.FleetNode(metas)
        for k in range(scans):
            od = [(b, t, p, tw) for b in range(B) for t, p, tw in segs[b % 4][k][0]]
            sc = [(b, segs[b % 4][k][1]) for b in range(B)]
            t0 = time.perf_counter()
            node.tick(od, sc)
            us.append(1e6 * (time.perf_counter() - t0))
        inserted = [sum(p is not None for p in log.match_poses) for log in node.logs]
    else:
        nodes = [NR.Node(m, NR.hip_backend()) for m in metas]
        for k in range(scans):
            t0 = time.perf_counter()
            for b, node in enumerate(nodes):
                od, sc = segs[b % 4][k]
                for t, p, tw in od:
                    node.OdometryCallback(t, p, tw)
                node.ScanCallback(sc)
            us.append(1e6 * (time.perf_counter() - t0))
        inserted = [sum(p is not None for p in node.log.match_poses) for node in nodes]
    assert inserted == [scans - 1] * B, inserted
    return {"step": step, "B": B, "us_per_tick": float(np.mean(us[warm:])), "ticks_timed": scans - warm}


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": float(np.median(s)), "max": s[-1]}


def child(args, step, B):
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--leg", step, "--size", str(B),
           "--reps", str(args.reps), "--calls", str(args.calls), "--scans", str(args.scans), "--warm-ticks", str(args.warm_ticks)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(f"step {step} B={B}: exit status {p.returncode}; nothing further is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls of each kind a repetition of the range leg times")
    ap.add_argument("--scans", type=int, default=8, help="scans per robot of the node leg")
    ap.add_argument("--warm-ticks", type=int, default=3, help="ticks of the node leg that are not timed (filters, submaps, one matched tick)")
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--node-sizes", type=int, nargs="*", default=[4, 64])
    ap.add_argument("--leg", choices=STEPS, default=None, help="run this one step in this process and print its JSON line")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a step's process may take")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.leg == "range":
        print(json.dumps(run_range(args.size, args.reps, args.calls)))
        return
    if args.leg:
        print(json.dumps(run_node(args.leg, args.size, args.scans, args.warm_ticks)))
        return

    result = {"workload": f"range: B members, one {N_BEAMS}-beam synth.make_laser_scan scan per member ({N_POSES} poses in the C2 world); "
                          f"node: B robots replaying {args.scans}-scan 1440-beam dumps of four synth sessions",
              "reps": args.reps, "calls": args.calls, "unit": "us per call (range: the whole fleet's range data once; node: one tick of the whole fleet)",
              "range_data": {}, "get_range_data_per_member": {}, "fleet_node_tick": {}, "single_nodes_tick": {}}

    def write():
        result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")

    for B in args.sizes:
        r = child(args, "range", B)
        result["range_data"][str(B)] = dict(stats(r["batch_us"]), rows_per_call=r["rows_per_call"])
        result["get_range_data_per_member"][str(B)] = stats(r["per_member_us"])
        ratio = min(r["per_member_us"]) / max(r["batch_us"])              # the slowest batch repetition against the fastest per-member one
        result["range_data"][str(B)]["per_member_min_over_batch_max"] = ratio
        result["range_data"][str(B)]["speedup_claimed"] = bool(ratio > 1.0)
        print(f"range B={B}: batch {stats(r['batch_us'])}, per member {stats(r['per_member_us'])}", file=sys.stderr, flush=True)
        write()
    for B in args.node_sizes:
        us = {"node_fleet": [], "node_single": []}
        for rep in range(args.reps):
            for step in us:                                           # the two sides alternate: each its own process, its own time limit
                us[step].append(child(args, step, B)["us_per_tick"])
                print(f"node B={B} rep={rep} {step}: {us[step][-1]:.0f} us per tick", file=sys.stderr, flush=True)
        result["fleet_node_tick"][str(B)] = stats(us["node_fleet"])
        result["single_nodes_tick"][str(B)] = stats(us["node_single"])
        ratio = min(us["node_single"]) / max(us["node_fleet"])
        result["fleet_node_tick"][str(B)]["single_min_over_fleet_max"] = ratio
        result["fleet_node_tick"][str(B)]["speedup_claimed"] = bool(ratio > 1.0)
        write()
    write()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
