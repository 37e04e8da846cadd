"""Fleet scan matching with the refinement (MapBuilder::ScanMatch for a batch), measured: B robots localising in one shared
occupancy map, one 400-point scan per robot per tick -- the map and the scans of scripts/fleet_match_bench.py, default options.

* ``scan_match``:   one ScanMatchFleet.scan_match per tick: the match's launch and the refinement's back to back on the handle's
  stream, ONE synchronisation;
* ``match_refine``: ScanMatchFleet.match, then ScanMatchFleet.refine from its poses: two submits, two synchronisations;
* ``refine``:       ScanMatchFleet.refine alone (start poses taken from a match outside the timed region);
* ``handles``:      the same scans through B GridFrontEnd handles, round robin on this thread, each doing Match then RefineMatch
  on its own copy of the map -- the only way to serve a fleet without the batch.

All legs run in the same process, alternating, --reps repetitions each; every repetition warms up and then times --ticks ticks with
the host clock around calls that each end in a synchronisation.  Every leg's refined poses are compared bit for bit with the
first leg's.  Prints ONE JSON line (and writes it to --out): scans/s as min / median / max, us per tick, the host time of submit
before its launches (median per tick), whether the speed-up condition holds (scan_match's minimum above handles' maximum at 64),
and the SHA-256 of the sources it was measured on.

  python scripts/fleet_scan_match_bench.py --out profiles/fleet_scan_match_bench.json
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

from scripts.fleet_match_bench import N_POINTS, N_POSES, RES, make_scans, room_map, stats  # noqa: E402

SOURCES = ["include/rgrid.h", "reflector_ekf_slam_amd/csrc/rgrid_batch.hip", "reflector_ekf_slam_amd/csrc/rgrid.hip",
           "reflector_ekf_slam_amd/csrc/rgrid_dev.h", "reflector_ekf_slam_amd/csrc/rgrid_refine_dev.h",
           "reflector_ekf_slam_amd/fleet_match.py", "reflector_ekf_slam_amd/grid.py", "scripts/fleet_match_bench.py",
           "scripts/fleet_scan_match_bench.py"]
LEGS = ("scan_match", "match_refine", "refine", "handles")


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
    result = {"workload": f"B members, one {N_POINTS}-point scan per member per tick against ONE shared {cells.shape[1]} x {cells.shape[0]} map at "
                          f"{RES} m ({N_POSES} distinct poses, member b of tick k sees pose (b + k) mod {N_POSES}), default matcher and "
                          "refinement options; every scan is matched and then refined from the matched pose",
              "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps, "unit": "scans/s (aggregate, one GPU, one host thread)"}
    for leg in LEGS:
        result[leg] = {}

    for B in sorted(set(args.batch_sizes) | set(args.handle_sizes)):
        fm = handles = None
        if B in args.batch_sizes:
            fm = M.ScanMatchFleet(max_scans=B, max_points=N_POINTS, num_grids=1, max_cells=cells.size, max_rotations=256)
            fm.SetGrid(0, cells, RES, max_xy)
            # the start poses of the `refine` leg: each distinct scan's matched pose (at most B scans per call: the handle holds B)
            coarse = [r.pose_estimate for j in range(0, N_POSES, B) for r in fm.match([(0,) + s for s in base[j:j + B]])]
        if B in args.handle_sizes:
            handles = [GridFrontEnd(max_points=N_POINTS, max_cells=cells.size, max_candidates=1 << 16) for _ in range(B)]
            for g in handles:
                g.SetGrid(cells, RES, max_xy)
        rates = {leg: [] for leg in LEGS}
        prepare = {leg: [] for leg in LEGS}
        ref = None
        for _ in range(args.reps):
            for leg in LEGS:
                if (leg == "handles" and handles is None) or (leg != "handles" and fm is None):
                    continue
                dt = 0.0
                for k in range(total):
                    scans = [(0,) + base[(b + k) % N_POSES] for b in range(B)]
                    if leg == "handles":
                        t0 = time.perf_counter()
                        fine = []
                        for g, s in zip(handles, scans):
                            c = g.Match(s[1], s[2])
                            fine.append(g.RefineMatch(s[1][:2], c.pose_estimate, s[2]))
                        t1 = time.perf_counter()
                    elif leg == "scan_match":
                        t0 = time.perf_counter()
                        out = fm.scan_match(scans)
                        t1 = time.perf_counter()
                        fine = [r.fine for r in out]
                        host = fm.last_prepare_seconds()
                    elif leg == "match_refine":
                        t0 = time.perf_counter()
                        out = fm.match(scans)
                        host = fm.last_prepare_seconds()
                        fine = fm.refine([(0, s[1][:2], r.pose_estimate, s[2]) for s, r in zip(scans, out)])
                        t1 = time.perf_counter()
                        host += fm.last_prepare_seconds()
                    else:
                        rscans = [(0, s[1][:2], coarse[(b + k) % N_POSES], s[2]) for b, s in enumerate(scans)]
                        t0 = time.perf_counter()
                        fine = fm.refine(rscans)
                        t1 = time.perf_counter()
                        host = fm.last_prepare_seconds()
                    if leg != "handles":
                        assert all(r.status == 0 for r in fine)
                        if k >= args.warmup:
                            prepare[leg].append(host)
                    if k == 0:                                      # every leg computes the same thing
                        sig = [(r.pose_estimate.tobytes(), r.final_cost, r.iterations, r.termination) for r in fine]
                        assert ref is None or sig == ref, leg
                        ref = sig
                    if k >= args.warmup:
                        dt += t1 - t0
                rates[leg].append(B * args.ticks / dt)
        for leg in LEGS:
            if rates[leg]:
                result[leg][str(B)] = dict(stats(rates[leg]), us_per_tick=1e6 * B / float(np.median(rates[leg])))
                if prepare[leg]:
                    result[leg][str(B)]["submit_host_us_per_tick"] = 1e6 * float(np.median(prepare[leg]))
        if fm is not None:
            fm.close()
        for g in handles or []:
            g.close()

    a, b, h = result["scan_match"], result["match_refine"], result["handles"]
    if "64" in a and "64" in h:
        result["scan_match64_min_over_handles64_max"] = a["64"]["min"] / h["64"]["max"]
        result["speedup_claimed"] = bool(a["64"]["min"] > h["64"]["max"])
    result["scan_match_median_over_match_refine_median"] = {B: a[B]["median"] / b[B]["median"] for B in a if B in b}
    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
