"""Fleet MapBuilder, measured: B robots, one scan of 3600 returns and 3600 misses per robot per tick through
MapBuilder::AddRangeData at the default options, on maps that the warm-up ticks have built,

* ``fleet``:   one FleetMapBuilder.AddRangeData per tick (ONE C call, rgrid_batch_add_range_data: at most five launches and three
  waits whatever B is);
* ``handles``: the same scans through B GridFrontEnd.AddRangeData handles (rgrid_add_range_data), robot after robot on this thread;
* ``python``:  the composition a fleet node made before the call existed: gravity_aligned_scans (numpy over every raw point) ->
  ScanMatchFleet.filter -> scan_match -> the filtered clouds moved by the refined pose in numpy -> insert, a robot's first submap set
  by hand, every stage collected before the next.

Every (size, repetition, leg) is a step of its own: a fresh child process under a time limit of its own, and the first step that
fails, faults or runs out of time ends the run with nothing started after it.  A step warms up (which builds the maps), times
--ticks ticks with the host clock around calls that each end in a synchronisation, and hands out the SHA-256 of the first and the
last member's poses of every timed tick and of their grids and limits at the end; after every repetition the three legs' hashes are
compared.  Prints ONE JSON line (and writes it to --out): scans/s as min / median / max over --reps repetitions, us per tick, the
ratio of the fleet's minimum to each other leg's maximum, and the SHA-256 of the sources it was measured on.  A speed-up is claimed
only where the fleet's minimum exceeds the other leg's maximum.

  python scripts/fleet_map_builder_bench.py --out profiles/fleet_map_builder_bench.json
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
           "reflector_ekf_slam_amd/csrc/rgrid_dev.h", "reflector_ekf_slam_amd/csrc/rgrid_refine_dev.h", "reflector_ekf_slam_amd/fleet_match.py",
           "reflector_ekf_slam_amd/map_builder.py", "reflector_ekf_slam_amd/grid.py", "scripts/fleet_map_builder_bench.py"]
N_POSES = 16          # distinct robot positions; member b stands at position b % N_POSES
N_VIEWS = 4           # noisy scans of every position; tick k uses view k % N_VIEWS
N_RETURNS = N_MISSES = 3600
MAX_CELLS = 1024 * 1024
LEGS = ("fleet", "handles", "python")


def make_scans():
    """[position][view] -> (RangeData in the tracking frame, EKF pose): an elliptic outer wall and four pillars (the scene of
    scripts/fleet_insert_bench.py) seen from a pose inside, misses on a circle of 12 m; the EKF pose is the true one plus a few centimetres."""
    from reflector_ekf_slam_amd.map_builder import RangeData
    rng = np.random.default_rng(4700)
    th = np.linspace(0, 2 * math.pi, 6000, endpoint=False)
    occ = [np.stack([9.0 * np.cos(th), 6.5 * np.sin(th)], 1)]
    for cx, cy in ((2.0, 1.5), (-3.5, 2.5), (4.0, -3.0), (-1.0, -4.0)):
        occ.append(np.stack([cx + 0.35 * np.cos(th[::10]), cy + 0.35 * np.sin(th[::10])], 1))
    occ = np.concatenate(occ)
    out = []
    for _ in range(N_POSES):
        x, y, yaw = rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(-math.pi, math.pi)
        c, s = math.cos(yaw), math.sin(yaw)
        views = []
        for _ in range(N_VIEWS):
            w = occ[np.sort(rng.choice(occ.shape[0], size=N_RETURNS, replace=False))] + rng.normal(0, 0.01, (N_RETURNS, 2)) - (x, y)
            ang = np.sort(rng.uniform(-math.pi, math.pi, N_MISSES))
            m = np.stack([12.0 * np.cos(ang), 12.0 * np.sin(ang)], 1)
            body = lambda p: np.ascontiguousarray(np.stack([c * p[:, 0] + s * p[:, 1], -s * p[:, 0] + c * p[:, 1]], 1), dtype=np.float32)   # noqa: E731
            ekf = (x + rng.normal(0, 0.03), y + rng.normal(0, 0.03), yaw + rng.normal(0, 0.01))
            views.append((RangeData(np.array([0.2, -0.1], np.float32), body(w), body(m)), ekf))
        out.append(views)
    return out


class PythonComposition:
    """MapBuilder::AddRangeData for B robots out of the single-kind fleet calls, as map_builder.MapBuilder composes it for one."""

    def __init__(self, B, options):
        from reflector_ekf_slam_amd import fleet_match as M
        self.M, self.o = M, options
        self.m = M.ScanMatchFleet(max_scans=B, max_points=N_RETURNS, num_grids=B, max_cells=MAX_CELLS)
        self.have = [False] * B

    def tick(self, rds, poses):
        import reflector_ekf_slam_amd.map_builder as MB
        o, m = self.o, self.m
        f32 = np.float32
        filtered = m.filter(self.M.gravity_aligned_scans(rds, poses), o.voxel_filter_size, o.adaptive_voxel_options)
        live = [j for j, r in enumerate(filtered) if r.filtered.shape[0]]
        est = {j: np.array([poses[j][0], poses[j][1], 0.0]) for j in live}
        matched = [j for j in live if self.have[j]]
        if matched:
            fine = m.scan_match([(j, est[j], filtered[j].filtered) for j in matched], o.real_time_scan_matcher_options, o.ceres_scan_matcher_options)
            for j, r in zip(matched, fine):
                est[j] = r.pose_estimate
        out, inserts = [None] * len(rds), []
        for j in live:
            e, theta = est[j], float(poses[j][2])
            qw, qz = math.cos(theta / 2), math.sin(theta / 2)
            aw, az = math.cos(0.5 * e[2]), math.sin(0.5 * e[2])
            out[j] = np.array([e[0], e[1], MB.yaw_of_quaternion_f64(aw * qw - az * qz, aw * qz + az * qw)])
            ha = f32(f32(0.5) * f32(e[2]))
            yaw2 = MB.yaw_of_quaternion_f32(math.cos(float(ha)), math.sin(float(ha)))
            origin = MB.rigid2f_apply((0.0, 0.0), MB.yaw_of_quaternion_f32(qw, qz), np.asarray(rds[j].origin, f32).reshape(1, 2))
            origin = MB.rigid2f_apply((e[0], e[1]), yaw2, origin)[0]
            if not self.have[j]:
                res = float(f32(o.resolution))
                m.SetGrid(j, np.zeros((100, 100), np.uint16), res, (float(origin[0]) + 50 * res, float(origin[1]) + 50 * res))
                self.have[j] = True
            inserts.append((j, origin, MB.rigid2f_apply((e[0], e[1]), yaw2, filtered[j].returns), MB.rigid2f_apply((e[0], e[1]), yaw2, filtered[j].misses)))
        assert not any(m.insert(inserts, o.range_data_inserter_options))
        return out

    def grid(self, j):
        return self.m.GetGrid(j), self.m.GetLimits(j)


def step(leg, B, ticks, warmup):
    """One leg at one size in this process -> {"rate": scans/s, "digest": poses of the timed ticks and final grids of the first and the last member}."""
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    from reflector_ekf_slam_amd.map_builder import FleetMapBuilder, MapBuilderOptions
    base, o = make_scans(), MapBuilderOptions()
    h, dt = hashlib.sha256(), 0.0
    if leg == "fleet":
        fb = FleetMapBuilder(B, o, max_points=N_RETURNS, max_cells=MAX_CELLS)
    elif leg == "handles":
        handles = [GridFrontEnd(max_points=N_RETURNS, max_cells=MAX_CELLS, max_candidates=1 << 16) for _ in range(B)]
    else:
        pc = PythonComposition(B, o)
    for k in range(warmup + ticks):
        scans = [base[b % N_POSES][k % N_VIEWS] for b in range(B)]
        rds, poses = [s[0] for s in scans], [s[1] for s in scans]
        t0 = time.perf_counter()
        if leg == "fleet":
            res = [None if r is None else r.local_pose for r in fb.AddRangeData([float(k)] * B, rds, poses)]
        elif leg == "handles":
            res = []
            for g, rd, pose in zip(handles, rds, poses):
                status, local_pose, _ = g.AddRangeData(o, rd.origin, rd.returns, rd.misses, pose)
                res.append(local_pose if status == 0 else None)
        else:
            res = pc.tick(rds, poses)
        t1 = time.perf_counter()
        assert all(r is not None for r in res)
        if k >= warmup:
            dt += t1 - t0
            for r in (res[0], res[-1]):
                h.update(np.asarray(r, np.float64).tobytes())
    shapes = []
    for b in (0, B - 1):
        if leg == "fleet":
            cells, limits = fb.grid(b)
        elif leg == "handles":
            limits = handles[b].GetLimits()
            handles[b]._grid_shape = (limits[1], limits[0])
            cells = handles[b].GetGrid()
        else:
            cells, limits = pc.grid(b)
        h.update(np.asarray(limits, np.float64).tobytes())
        h.update(np.ascontiguousarray(cells, np.uint16).tobytes())
        shapes.append([int(limits[0]), int(limits[1])])
    counts = list(fb._fleet.last_call_counts()) if leg == "fleet" else None
    return {"rate": B * ticks / dt, "digest": h.hexdigest(), "grids": shapes, "launches_syncs": counts}


def stats(rates):
    r = sorted(rates)
    return {"min": r[0], "median": float(np.median(r)), "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds one (size, repetition, leg) may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", nargs=2, metavar=("LEG", "B"), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args.step[0], int(args.step[1]), args.ticks, args.warmup)))
        return

    result = {"workload": f"B members, one scan of {N_RETURNS} returns and {N_MISSES} misses per member per tick ({N_POSES} positions, {N_VIEWS} noisy "
                          f"scans of each; member b stands at position b mod {N_POSES}), MapBuilder::AddRangeData at the default options, maps "
                          f"built by the {args.warmup} warm-up ticks",
              "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps, "unit": "scans/s (aggregate, one GPU, one host thread)"}
    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    for leg in LEGS:
        result[leg] = {}
    for B in sorted(set(args.sizes)):
        rates = {leg: [] for leg in LEGS}
        for _ in range(args.reps):
            seen = {}
            for leg in LEGS:                                        # the legs alternate; each step is a process of its own
                cmd = [sys.executable, os.path.abspath(__file__), "--step", leg, str(B), "--ticks", str(args.ticks), "--warmup", str(args.warmup)]
                t0 = time.perf_counter()
                try:
                    done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    sys.exit(f"step {leg} B={B} ran out of its {args.step_timeout:.0f} s: nothing more is started")
                if done.returncode != 0:
                    sys.stderr.write(done.stderr[-2000:])
                    sys.exit(f"step {leg} B={B} ended with status {done.returncode}: nothing more is started")
                seen[leg] = json.loads(done.stdout.strip().splitlines()[-1])
                rates[leg].append(seen[leg]["rate"])
                sys.stderr.write(f"B={B} {leg}: {seen[leg]['rate']:.0f} scans/s, the step took {time.perf_counter() - t0:.1f} s\n")
            assert seen["fleet"]["digest"] == seen["handles"]["digest"] == seen["python"]["digest"], (B, seen)   # the same poses and grids, bit for bit
            result["grids_first_and_last_member"] = seen["fleet"]["grids"]
            result.setdefault("launches_syncs_last_tick", {})[str(B)] = seen["fleet"]["launches_syncs"]
        for leg in LEGS:
            result[leg][str(B)] = dict(stats(rates[leg]), us_per_tick=1e6 * B / float(np.median(rates[leg])))
        for other in LEGS[1:]:
            result.setdefault(f"fleet_min_over_{other}_max", {})[str(B)] = result["fleet"][str(B)]["min"] / result[other][str(B)]["max"]
            result.setdefault(f"speedup_over_{other}_claimed", {})[str(B)] = bool(result["fleet"][str(B)]["min"] > result[other][str(B)]["max"])
        result["sizes"] = sorted(int(k) for k in result["fleet"])
        if args.out:                                                # (a size that is done is kept whatever happens to a later one)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
