"""What handing a fleet's state over costs, measured: B members at n = 259 (the built maps of scripts/fleet_bench.py, 128 reflectors
each, ld = 272) and at n = 67 (the leading 32 reflectors of the same states, in a fleet of the same capacity), through

* ``snapshot``:  ``fleet.snapshot()`` of all members -- a size call, one buffer, ONE launch of k_fleet_pack, one copy of the payload;
* ``get_state``: the only route there was before, on the same build and the same fleet: ``fleet.get_state(i)`` per member (a
                 synchronisation, an ld x n copy and the host's mirror loop each);
* ``restore``:   ``fleet.restore(snap)`` of that snapshot -- one copy to the device, ONE launch of k_fleet_unpack;
* ``set_state``: ``fleet.set_state(i, t, mu, sigma)`` per member, from dense matrices held ready (which restores neither the flags nor
                 the zeros beyond n).

All legs run in the same process, alternating, --reps repetitions each; a repetition times a loop of calls with the host clock (every
call ends in a synchronisation) and reports us per call.  Prints ONE JSON line and writes it to --out.

  python scripts/fleet_snapshot_bench.py --out profiles/fleet_snapshot_bench.json
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
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

SOURCES = ["include/rfleet.h", "reflector_ekf_slam_amd/csrc/fleet_dev.h", "reflector_ekf_slam_amd/csrc/fleet_host.h", "reflector_ekf_slam_amd/csrc/fleet_snapshot.h",
           "reflector_ekf_slam_amd/csrc/fleet_snapshot.hip", "reflector_ekf_slam_amd/csrc/rfleet_api.hip", "reflector_ekf_slam_amd/fleet.py",
           "scripts/fleet_snapshot_bench.py"]
N_SEEDS = 8
DIMS = (259, 67)
LEGS = ("snapshot", "get_state", "restore", "set_state")


def stats(us):
    s = sorted(us)
    return {"min": s[0], "median": float(np.median(s)), "max": s[-1]}


def timed(call, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    return 1e6 * (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fleet-sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--members-per-rep", type=int, default=1024, help="member states moved per leg and repetition (calls = this / B, at least 3)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import fleet_bench
    from reflector_ekf_slam_amd import ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd import session as S
    sessions, snaps, _ = fleet_bench.build_maps(1)
    result = {"workload": "B members of a fleet of max_landmarks = 128 (ld = 272), states of scripts/fleet_bench.py's built maps (seeds 7000 + i "
                          "mod 8): n = 259, and their leading 67 x 67 part",
              "unit": "us per call (host clock around calls that end in a synchronisation); a get_state / set_state call is all B members",
              "reps": args.reps, "dims": {}}

    for n in DIMS:
        rec = {leg: {} for leg in LEGS}
        rec.update(calls_per_rep={}, blob_bytes={}, get_state_min_over_snapshot_max={}, set_state_min_over_restore_max={},
                   snapshot_is_faster={}, restore_is_faster={})
        for B in args.fleet_sizes:
            fl = ReflectorEKFSLAMFleet([S.options_for(sessions[b % N_SEEDS]) for b in range(B)], max_landmarks=128)
            dense = [(snaps[b % N_SEEDS].time, np.ascontiguousarray(snaps[b % N_SEEDS].mu[:n]),
                      np.ascontiguousarray(snaps[b % N_SEEDS].sigma[:n, :n])) for b in range(B)]
            for b, (t, mu, sg) in enumerate(dense):
                fl.set_state(b, t, mu, sg)
            assert (fl.n() == n).all()
            snap = fl.snapshot()

            def get_all():
                return [fl.get_state(b) for b in range(B)]

            def set_all():
                for b, (t, mu, sg) in enumerate(dense):
                    fl.set_state(b, t, mu, sg)

            want = get_all()                                 # the two routes hand over the same bits
            for g in (0, B - 1):
                assert np.array_equal(snap.mu(g), want[g].mu) and np.array_equal(snap.sigma(g), want[g].sigma)
            fl.restore(snap)
            back = get_all()
            assert all(np.array_equal(a.mu, b.mu) and np.array_equal(a.sigma, b.sigma) for a, b in zip(want, back))
            calls = max(3, args.members_per_rep // B)
            legs = {"snapshot": fl.snapshot, "get_state": get_all, "restore": lambda: fl.restore(snap), "set_state": set_all}
            for call in legs.values():                       # warm every leg (the staging buffer is allocated here)
                call()
            us = {leg: [] for leg in LEGS}
            for _ in range(args.reps):
                for leg in LEGS:
                    us[leg].append(timed(legs[leg], calls))
            fl.close()
            key = str(B)
            for leg in LEGS:
                rec[leg][key] = stats(us[leg])
            rec["calls_per_rep"][key] = calls
            rec["blob_bytes"][key] = int(snap.blob.size)
            rec["get_state_min_over_snapshot_max"][key] = rec["get_state"][key]["min"] / rec["snapshot"][key]["max"]
            rec["set_state_min_over_restore_max"][key] = rec["set_state"][key]["min"] / rec["restore"][key]["max"]
            rec["snapshot_is_faster"][key] = bool(rec["snapshot"][key]["max"] < rec["get_state"][key]["min"])
            rec["restore_is_faster"][key] = bool(rec["restore"][key]["max"] < rec["set_state"][key]["min"])
        result["dims"][str(n)] = rec

    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
