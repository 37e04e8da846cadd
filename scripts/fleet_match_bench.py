"""Fleet scan matching, measured: B robots localising in one shared occupancy map, one 400-point scan per robot per tick,

* ``batch``:        one ScanMatchFleet.match per tick (ONE launch of kgb_match, one workgroup per scan and rotated scan, the arg-max
  over a scan's rotated scans by its last workgroup);
* ``batch_launch``: the same with the arg-max in a second launch (rgrid_batch_set_reduction): the other form of the reduction;
* ``packed``:       the batch with the scan records packed once outside the timed region (the C calls alone: what a C++ host pays);
* ``handles``:      the same scans through B GridFrontEnd handles, round robin on this thread, each with its own copy of the map --
  the only way to serve a fleet without the batch.

All legs run in the same process, alternating, --reps repetitions each; every repetition warms up and then times --ticks ticks with
the host clock around calls that each end in a synchronisation (collect / the handle's own wait).  Prints ONE JSON line (and
writes it to --out): scans/s as min / median / max, us per tick, the host time of submit before its launch (initial rotations,
search parameters, rotation tables, packing; median per tick), and the SHA-256 of the sources it was measured on.

  python scripts/fleet_match_bench.py --out profiles/fleet_match_bench.json
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

SOURCES = ["include/rgrid.h", "reflector_ekf_slam_amd/csrc/rgrid_batch.hip", "reflector_ekf_slam_amd/csrc/rgrid.hip",
           "reflector_ekf_slam_amd/csrc/rgrid_dev.h", "reflector_ekf_slam_amd/fleet_match.py", "reflector_ekf_slam_amd/grid.py",
           "scripts/fleet_match_bench.py"]
N_POSES = 16          # distinct poses (scans); member b of tick k sees scan (b + k) % N_POSES
N_POINTS = 400
RES, HALF = 0.05, 12.0


def room_map():
    """A 480 x 480 probability grid at 0.05 m: an elliptic outer wall and four pillars occupied, the inside free, a band along
    the border unknown.  -> (cells uint16 (ny, nx), max_xy, occupied points in the map frame)."""
    rng = np.random.default_rng(3)
    n = int(round(2 * HALF / RES))
    cells = np.full((n, n), 30000, np.uint16)
    cells[:8, :] = 0; cells[-8:, :] = 0; cells[:, :8] = 0; cells[:, -8:] = 0
    th = np.linspace(0, 2 * math.pi, 6000, endpoint=False)
    occ = [np.stack([9.0 * np.cos(th), 6.5 * np.sin(th)], 1)]
    for cx, cy in ((2.0, 1.5), (-3.5, 2.5), (4.0, -3.0), (-1.0, -4.0)):
        occ.append(np.stack([cx + 0.35 * np.cos(th[::10]), cy + 0.35 * np.sin(th[::10])], 1))
    occ = np.concatenate(occ)
    ix = np.rint((HALF - occ[:, 1]) / RES - 0.5).astype(int)
    iy = np.rint((HALF - occ[:, 0]) / RES - 0.5).astype(int)
    cells[iy, ix] = rng.integers(1200, 2600, occ.shape[0]).astype(np.uint16)
    return cells, (HALF, HALF), occ


def make_scans(occ):
    """N_POSES (initial pose, points in the tracking frame): the occupied points seen from a pose, the initial estimate nearby."""
    rng = np.random.default_rng(4200)
    out = []
    for _ in range(N_POSES):
        pose = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(-math.pi, math.pi)])
        p = occ[np.sort(rng.choice(occ.shape[0], size=N_POINTS, replace=False))]
        c, s = math.cos(pose[2]), math.sin(pose[2])
        dx, dy = p[:, 0] - pose[0], p[:, 1] - pose[1]
        loc = (np.stack([c * dx + s * dy, -s * dx + c * dy], 1) + rng.normal(0, 0.01, (N_POINTS, 2))).astype(np.float32)
        init = pose + np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), math.radians(rng.uniform(-5, 5))])
        out.append((init, np.ascontiguousarray(loc)))
    return out


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
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    cells, max_xy, occ = room_map()
    base = make_scans(occ)
    total = args.warmup + args.ticks
    legs = ("batch", "batch_launch", "packed", "handles")
    result = {"workload": f"B members, one {N_POINTS}-point scan per member per tick against ONE shared {cells.shape[1]} x {cells.shape[0]} map at "
                          f"{RES} m ({N_POSES} distinct poses, member b of tick k sees pose (b + k) mod {N_POSES}), default matcher options",
              "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps, "unit": "scans/s (aggregate, one GPU, one host thread)"}
    for leg in legs:
        result[leg] = {}

    for B in sorted(set(args.batch_sizes) | set(args.handle_sizes)):
        fm = handles = None
        if B in args.batch_sizes:
            fm = M.ScanMatchFleet(max_scans=B, max_points=N_POINTS, num_grids=1, max_cells=cells.size, max_rotations=256)
            fm.SetGrid(0, cells, RES, max_xy)
            packed = [M.ScanMatchFleet.pack([(0,) + base[(b + k) % N_POSES] for b in range(B)]) for k in range(N_POSES)]
        if B in args.handle_sizes:
            handles = [GridFrontEnd(max_points=N_POINTS, max_cells=cells.size, max_candidates=1 << 16) for _ in range(B)]
            for g in handles:
                g.SetGrid(cells, RES, max_xy)
        rates = {leg: [] for leg in legs}
        prepare = []
        ref = None
        for _ in range(args.reps):
            for leg in legs:
                if leg == "handles" and handles is None:
                    continue
                if leg != "handles" and fm is None:
                    continue
                if leg != "handles":
                    fm.set_reduction(M.REDUCE_LAUNCH if leg == "batch_launch" else M.REDUCE_ARRIVAL)
                dt = 0.0
                for k in range(total):
                    scans = [(0,) + base[(b + k) % N_POSES] for b in range(B)]
                    if leg == "handles":
                        t0 = time.perf_counter()
                        out = [g.Match(s[1], s[2]) for g, s in zip(handles, scans)]
                        t1 = time.perf_counter()
                    elif leg == "packed":
                        t0 = time.perf_counter()
                        rc = fm.submit_packed_code(packed[k % N_POSES])
                        out = fm.collect()
                        t1 = time.perf_counter()
                        assert rc == 0
                    else:
                        t0 = time.perf_counter()
                        out = fm.match(scans)
                        t1 = time.perf_counter()
                    if leg != "handles":
                        assert all(r.status == 0 for r in out)
                        if k >= args.warmup and leg == "batch":
                            prepare.append(fm.last_prepare_seconds())
                    if k == 0:                                      # every leg computes the same thing
                        sig = [(r.score, tuple(r.pose_estimate), r.best) for r in out]
                        assert ref is None or sig == ref
                        ref = sig
                    if k >= args.warmup:
                        dt += t1 - t0
                rates[leg].append(B * args.ticks / dt)
        for leg in legs:
            if rates[leg]:
                result[leg][str(B)] = dict(stats(rates[leg]), us_per_tick=1e6 * B / float(np.median(rates[leg])))
        if prepare:
            result["batch"][str(B)]["submit_host_us_per_tick"] = 1e6 * float(np.median(prepare))
        if fm is not None:
            fm.close()
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
