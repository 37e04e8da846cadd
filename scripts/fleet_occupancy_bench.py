"""Fleet occupancy grid, measured: B robots, each with its OWN 480 x 480 map at 0.05 m built by ScanMatchFleet.insert from the scans of
scripts/fleet_insert_bench.py; one call gives the occupancy grid of every robot (Node::PublishMap up to the message fields),

* ``batch``:   one ScanMatchFleet.occupancy_grids per call (ONE launch of kgb_occupancy, one workgroup per slot, one wait; the maps
  stay in the batch handle's resident slots);
* ``handles``: (a) the same grids in B GridFrontEnd handles, OccupancyGrid() each, round robin on this thread;
* ``today``:   (b) what a user of the fleet did before this call existed: ScanMatchFleet.draw_textures and the painting in numpy on
  the host (tests/witness/occupancy_witness.py: composite, turn, frame, rounding rule, message order).

All legs run in the same process, alternating, --reps repetitions each; every repetition warms up and then times --calls calls with
the host clock.  In every repetition the first and the last member's grid must be the same bytes, origin and box in all three legs.
Prints ONE JSON line (and writes it to --out): grids/s as min / median / max, us per call, and the SHA-256 of the sources it was
measured on.  A speed-up is claimed only where the batch's minimum exceeds the other leg's maximum.

  python scripts/fleet_occupancy_bench.py --out profiles/fleet_occupancy_bench.json
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.fleet_insert_bench import HALF, N_CELLS, N_POSES, N_RETURNS, RES, make_scans, stats  # noqa: E402

SOURCES = ["include/rgrid.h", "reflector_ekf_slam_amd/csrc/rgrid_batch.hip", "reflector_ekf_slam_amd/csrc/rgrid.hip",
           "reflector_ekf_slam_amd/csrc/rgrid_dev.h", "reflector_ekf_slam_amd/fleet_match.py", "reflector_ekf_slam_amd/grid.py",
           "scripts/fleet_occupancy_bench.py", "scripts/fleet_insert_bench.py", "tests/witness/occupancy_witness.py"]
N_INSERTS = 6         # scans inserted into every member's map before it is painted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)          # (the `today` leg paints B maps in numpy per call)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    from tests.witness import occupancy_witness as W
    base = make_scans()
    empty = np.zeros((N_CELLS, N_CELLS), np.uint16)
    total = args.warmup + args.calls
    legs = ("batch", "handles", "today")
    result = {"workload": f"B members, each with its own {N_CELLS} x {N_CELLS} map at {RES} m holding {N_INSERTS} inserted {N_RETURNS}-return scans "
                          f"(member b inserts scans b .. b + {N_INSERTS - 1} mod {N_POSES} of scripts/fleet_insert_bench.py); one call gives every "
                          "member's occupancy grid (mode 0)",
              "calls": args.calls, "warmup": args.warmup, "reps": args.reps, "unit": "grids/s (aggregate, one GPU, one host thread)",
              "kernel": "kgb_occupancy: one workgroup of 512 threads per slot, 64 x 64 byte tiles through LDS (pitch 72), the byte table read "
                        "through L2, 256 of the 512 threads store; other tile shapes, a wider store side, more than one workgroup per slot and "
                        "the table in LDS were not tried"}
    for leg in legs:
        result[leg] = {}

    for B in sorted(set(args.sizes)):
        fm = M.ScanMatchFleet(max_scans=B, max_points=N_RETURNS, num_grids=B, max_cells=empty.size, max_rotations=1)
        for b in range(B):
            fm.SetGrid(b, empty, RES, (HALF, HALF))
        for k in range(N_INSERTS):
            assert not any(fm.insert([(b,) + base[(b + k) % N_POSES] + (None,) for b in range(B)]))
        handles = [GridFrontEnd(max_points=N_RETURNS, max_cells=empty.size, max_candidates=1 << 10) for _ in range(B)]
        for b, g in enumerate(handles):
            lim = fm.GetLimits(b)
            g.SetGrid(fm.GetGrid(b), lim[2], (lim[3], lim[4]))
        ids = list(range(B))
        origins = [(float(np.float32(0.01 * b)), float(np.float32(-0.02 * b))) for b in range(B)]
        rates = {leg: [] for leg in legs}
        for _ in range(args.reps):
            ends = {}
            for leg in legs:
                dt = 0.0
                for k in range(total):
                    t0 = time.perf_counter()
                    if leg == "handles":
                        got = [g.OccupancyGrid(o) for g, o in zip(handles, origins)]
                        got = [(g.data, g.origin, g.box) for g in (got[0], got[-1])]
                    elif leg == "today":
                        got = []
                        for tex, o in zip(fm.draw_textures(ids), origins):
                            data, origin = W.occupancy(W.paint(tuple(tex), RES, o), RES)
                            got.append((data, origin, tex.box))
                        got = [got[0], got[-1]]
                    else:
                        got = fm.occupancy_grids(ids, origins)
                        got = [(g.data, g.origin, g.box) for g in (got[0], got[-1])]
                    t1 = time.perf_counter()
                    ends[leg] = got
                    if k >= args.warmup:
                        dt += t1 - t0
                rates[leg].append(B * args.calls / dt)
            for leg in legs[1:]:                                    # every leg gives the same grids
                for a, h in zip(ends["batch"], ends[leg]):
                    assert tuple(a[1]) == tuple(h[1]) and tuple(a[2]) == tuple(h[2]) and np.array_equal(a[0], h[0]), leg
        for leg in legs:
            result[leg][str(B)] = dict(stats(rates[leg]), us_per_call=1e6 * B / float(np.median(rates[leg])))
        for leg in legs[1:]:
            result.setdefault(f"batch_min_over_{leg}_max", {})[str(B)] = result["batch"][str(B)]["min"] / result[leg][str(B)]["max"]
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
