"""Fleet map insertion, measured: B robots, each building its OWN 480 x 480 map at 0.05 m, one 3600-return scan per robot per tick,

* ``batch``:   one ScanMatchFleet.insert per tick (ONE launch of kgb_insert, one workgroup per scan; the maps stay in the batch
  handle's resident slots);
* ``packed``:  the batch with the scan records packed once outside the timed region (the C calls alone: what a C++ host pays);
* ``handles``: the same scans through B GridFrontEnd handles (GrowAsNeeded + Insert), round robin on this thread -- the only way to
  build a fleet's maps without the batch.

All legs run in the same process, alternating, --reps repetitions each; every repetition starts from unknown maps, warms up and then
times --ticks ticks with the host clock around calls that each end in a synchronisation.  After every repetition the first and the
last member's map of the batch must equal the handles' bit for bit.  Prints ONE JSON line (and writes it to --out): scans/s as
min / median / max, us per tick, and the SHA-256 of the sources it was measured on.  A speed-up is claimed only where the batch's
minimum exceeds the handles' maximum.

  python scripts/fleet_insert_bench.py --out profiles/fleet_insert_bench.json
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
           "scripts/fleet_insert_bench.py"]
N_POSES = 16          # distinct scans; member b of tick k inserts scan (b + k) % N_POSES
N_RETURNS = 3600
RES, HALF, N_CELLS = 0.05, 12.0, 480


def make_scans():
    """N_POSES (origin, returns in the map frame): an elliptic outer wall and four pillars seen from a pose inside."""
    rng = np.random.default_rng(4300)
    th = np.linspace(0, 2 * math.pi, 6000, endpoint=False)
    occ = [np.stack([9.0 * np.cos(th), 6.5 * np.sin(th)], 1)]
    for cx, cy in ((2.0, 1.5), (-3.5, 2.5), (4.0, -3.0), (-1.0, -4.0)):
        occ.append(np.stack([cx + 0.35 * np.cos(th[::10]), cy + 0.35 * np.sin(th[::10])], 1))
    occ = np.concatenate(occ)
    out = []
    for _ in range(N_POSES):
        origin = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3)], np.float32)
        p = occ[np.sort(rng.choice(occ.shape[0], size=N_RETURNS, replace=False))] + rng.normal(0, 0.01, (N_RETURNS, 2))
        out.append((origin, np.ascontiguousarray(p, dtype=np.float32)))
    return out


def stats(rates):
    r = sorted(rates)
    return {"min": r[0], "median": float(np.median(r)), "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    base = make_scans()
    empty = np.zeros((N_CELLS, N_CELLS), np.uint16)
    max_xy = (HALF, HALF)
    total = args.warmup + args.ticks
    legs = ("batch", "packed", "handles")
    result = {"workload": f"B members, each with its own {N_CELLS} x {N_CELLS} map at {RES} m, one {N_RETURNS}-return scan per member per tick "
                          f"({N_POSES} distinct scans, member b of tick k inserts scan (b + k) mod {N_POSES}), default inserter options, no misses",
              "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps, "unit": "scans/s (aggregate, one GPU, one host thread)"}
    for leg in legs:
        result[leg] = {}

    for B in sorted(set(args.sizes)):
        fm = M.ScanMatchFleet(max_scans=B, max_points=N_RETURNS, num_grids=B, max_cells=empty.size, max_rotations=1)
        packed = [M.ScanMatchFleet.pack_insert([(b,) + base[(b + k) % N_POSES] + (None,) for b in range(B)]) for k in range(N_POSES)]
        handles = [GridFrontEnd(max_points=N_RETURNS, max_cells=empty.size, max_candidates=1 << 10) for _ in range(B)]
        rates = {leg: [] for leg in legs}
        for _ in range(args.reps):
            maps = {}
            for leg in legs:
                if leg == "handles":
                    for g in handles:
                        g.SetGrid(empty, RES, max_xy)
                else:
                    for b in range(B):
                        fm.SetGrid(b, empty, RES, max_xy)
                dt = 0.0
                for k in range(total):
                    scans = [(b,) + base[(b + k) % N_POSES] + (None,) for b in range(B)]
                    if leg == "handles":
                        t0 = time.perf_counter()
                        for g, s in zip(handles, scans):
                            g.Insert(s[1], s[2])
                        t1 = time.perf_counter()
                    elif leg == "packed":
                        t0 = time.perf_counter()
                        rc = fm.submit_insert_packed_code(packed[k % N_POSES])
                        status = fm.collect_insert()
                        t1 = time.perf_counter()
                        assert rc == 0 and not any(status)
                    else:
                        t0 = time.perf_counter()
                        status = fm.insert(scans)
                        t1 = time.perf_counter()
                        assert not any(status)
                    if k >= args.warmup:
                        dt += t1 - t0
                rates[leg].append(B * args.ticks / dt)
                maps[leg] = [handles[b].GetGrid() if leg == "handles" else fm.GetGrid(b) for b in (0, B - 1)]
            for leg in legs[:2]:                                    # every leg builds the same maps
                assert all(np.array_equal(a, h) for a, h in zip(maps[leg], maps["handles"])), leg
        for leg in legs:
            result[leg][str(B)] = dict(stats(rates[leg]), us_per_tick=1e6 * B / float(np.median(rates[leg])))
        result.setdefault("batch_min_over_handles_max", {})[str(B)] = result["batch"][str(B)]["min"] / result["handles"][str(B)]["max"]
        result.setdefault("speedup_claimed", {})[str(B)] = bool(result["batch"][str(B)]["min"] > result["handles"][str(B)]["max"])
        fm.close()
        for g in handles:
            g.close()

    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
