"""Fleet voxel filters, measured: B robots, one 3600-return scan with 3600 misses per robot per tick, the filter stage of
MapBuilder::AddRangeData at the default options (voxel size 0.025 m, adaptive filter 0.9 m / 500 points / 100 m),

* ``batch``:   one ScanMatchFleet.filter per tick (ONE launch of kgb_filter, one workgroup per scan, one wait);
* ``handles``: the same scans through B GridFrontEnd handles -- VoxelFilter of the returns, VoxelFilter of the misses and
  AdaptiveVoxelFilter of the first, robot after robot on this thread: the only way to filter a fleet's scans without the batch.

Every (size, repetition, leg) is a step of its own: a fresh child process under a time limit of its own, and the first step that
fails, faults or runs out of time ends the run with nothing started after it.  A step warms up, times --ticks ticks with the host
clock around calls that each end in a synchronisation, and checks the first and the last member's three clouds of the last tick
against the other leg's by their SHA-256.  Prints ONE JSON line (and writes it to --out): scans/s as min / median / max over --reps
repetitions, us per tick, the ratio of the batch's minimum to the handles' maximum, and the SHA-256 of the sources it was
measured on.  A speed-up is claimed only where the batch's minimum exceeds the handles' maximum.

  python scripts/fleet_filter_scan_bench.py --out profiles/fleet_filter_scan_bench.json
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

SOURCES = ["include/rgrid.h", "reflector_ekf_slam_amd/csrc/rgrid_batch.hip", "reflector_ekf_slam_amd/csrc/rgrid.hip",
           "reflector_ekf_slam_amd/csrc/rgrid_dev.h", "reflector_ekf_slam_amd/fleet_match.py", "reflector_ekf_slam_amd/grid.py",
           "scripts/fleet_filter_scan_bench.py"]
N_POSES = 16          # distinct scans; member b of tick k filters scan (b + k) % N_POSES
N_RETURNS = N_MISSES = 3600
LEGS = ("batch", "handles")


def make_scans():
    """N_POSES (returns, misses) in the sensor frame: an elliptic outer wall and four pillars seen from a pose inside (the scene of
    scripts/fleet_insert_bench.py), misses on a circle of 30 m."""
    rng = np.random.default_rng(4400)
    th = np.linspace(0, 2 * math.pi, 6000, endpoint=False)
    occ = [np.stack([9.0 * np.cos(th), 6.5 * np.sin(th)], 1)]
    for cx, cy in ((2.0, 1.5), (-3.5, 2.5), (4.0, -3.0), (-1.0, -4.0)):
        occ.append(np.stack([cx + 0.35 * np.cos(th[::10]), cy + 0.35 * np.sin(th[::10])], 1))
    occ = np.concatenate(occ)
    out = []
    for _ in range(N_POSES):
        origin = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3)])
        p = occ[np.sort(rng.choice(occ.shape[0], size=N_RETURNS, replace=False))] + rng.normal(0, 0.01, (N_RETURNS, 2)) - origin
        ang = np.sort(rng.uniform(-math.pi, math.pi, N_MISSES))
        m = np.stack([30.0 * np.cos(ang), 30.0 * np.sin(ang)], 1) + rng.normal(0, 0.01, (N_MISSES, 2))
        out.append((np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(m, dtype=np.float32)))
    return out


def digest(clouds):
    h = hashlib.sha256()
    for c in clouds:
        h.update(np.int64(c.shape[0]).tobytes())
        h.update(np.ascontiguousarray(c, dtype=np.float32).tobytes())
    return h.hexdigest()


def step(leg, B, ticks, warmup):
    """One leg at one size in this process -> {"rate": scans/s, "digest": of the last tick's first and last member}."""
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    base = make_scans()
    last = None
    dt = 0.0
    if leg == "batch":
        fm = M.ScanMatchFleet(max_scans=B, max_points=N_RETURNS, num_grids=1, max_cells=64, max_rotations=1)
    else:
        handles = [GridFrontEnd(max_points=N_RETURNS, max_cells=64, max_candidates=1 << 10) for _ in range(B)]
    for k in range(warmup + ticks):
        scans = [base[(b + k) % N_POSES] for b in range(B)]
        if leg == "batch":
            t0 = time.perf_counter()
            res = fm.filter(scans)
            t1 = time.perf_counter()
            assert not any(r.status for r in res)
            last = [c for r in (res[0], res[-1]) for c in (r.returns, r.misses, r.filtered)]
        else:
            t0 = time.perf_counter()
            res = []
            for g, (ret, mis) in zip(handles, scans):
                fr = g.VoxelFilter(ret, 0.025)
                res.append((fr, g.VoxelFilter(mis, 0.025), g.AdaptiveVoxelFilter(fr)))
            t1 = time.perf_counter()
            last = [c for r in (res[0], res[-1]) for c in r]
        if k >= warmup:
            dt += t1 - t0
    return {"rate": B * ticks / dt, "digest": digest(last), "kept": [int(c.shape[0]) for c in last[:3]]}


def stats(rates):
    r = sorted(rates)
    return {"min": r[0], "median": float(np.median(r)), "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds one (size, repetition, leg) may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", nargs=2, metavar=("LEG", "B"), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args.step[0], int(args.step[1]), args.ticks, args.warmup)))
        return

    result = {"workload": f"B members, one scan of {N_RETURNS} returns and {N_MISSES} misses per member per tick ({N_POSES} distinct scans, member b of "
                          f"tick k filters scan (b + k) mod {N_POSES}), voxel size 0.025 m, default adaptive options (0.9 m, 500 points, 100 m)",
              "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps, "unit": "scans/s (aggregate, one GPU, one host thread)"}
    for leg in LEGS:
        result[leg] = {}
    for B in sorted(set(args.sizes)):
        rates = {leg: [] for leg in LEGS}
        for _ in range(args.reps):
            seen = {}
            for leg in LEGS:                                        # the legs alternate; each step is a process of its own
                cmd = [sys.executable, os.path.abspath(__file__), "--step", leg, str(B), "--ticks", str(args.ticks), "--warmup", str(args.warmup)]
                try:
                    done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    sys.exit(f"step {leg} B={B} ran out of its {args.step_timeout:.0f} s: nothing more is started")
                if done.returncode != 0:
                    sys.stderr.write(done.stderr[-2000:])
                    sys.exit(f"step {leg} B={B} ended with status {done.returncode}: nothing more is started")
                seen[leg] = json.loads(done.stdout.strip().splitlines()[-1])
                rates[leg].append(seen[leg]["rate"])
            assert seen["batch"]["digest"] == seen["handles"]["digest"], (B, seen)      # both legs filter to the same bits
            result["kept_points_first_member"] = seen["batch"]["kept"]
        for leg in LEGS:
            result[leg][str(B)] = dict(stats(rates[leg]), us_per_tick=1e6 * B / float(np.median(rates[leg])))
        result.setdefault("batch_min_over_handles_max", {})[str(B)] = result["batch"][str(B)]["min"] / result["handles"][str(B)]["max"]
        result.setdefault("speedup_claimed", {})[str(B)] = bool(result["batch"][str(B)]["min"] > result["handles"][str(B)]["max"])

    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
