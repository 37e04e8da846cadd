"""What a pose log after every message costs a fleet host, measured: B C2-sized members at capacity (128 reflectors each, the world
of scripts/fleet_bench.py); a tick is five odometry messages and one steady-state scan per member (6 B messages), handed over

* ``untracked_submit_sync``:      one ``submit`` per tick, then ``sync()`` -- no pose log at all: the floor;
* ``tracked_submit_take_track``:  tracking on, one ``submit`` per tick (ONE launch of k_fleet_step_track, which writes a record per
                                  message), then ``take_track()`` -- every member's pose after every message;
* ``submit_poses_per_message``:   the only route there was before the pose track, on the same build and the same fleet: one
                                  ``submit`` per message rank (the members' first odometry messages, their second ones, ..., their
                                  scans: six launches) with ``poses()`` behind each (six synchronisations).

All legs run in the same process, alternating, --reps repetitions each; every repetition restarts from the same built maps
(set_state), warms up and then times --ticks ticks with the host clock around work that ends in a synchronisation, and reports us
per tick.  Prints ONE JSON line and writes it to --out, with the SHA-256 of the fleet sources it was measured on.

  python scripts/fleet_track_bench.py --out profiles/fleet_track_bench.json
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

SOURCES = ["include/rfleet.h", "reflector_ekf_slam_amd/csrc/fleet_dev.h", "reflector_ekf_slam_amd/csrc/fleet_host.h", "reflector_ekf_slam_amd/csrc/fleet_kernels.hip",
           "reflector_ekf_slam_amd/csrc/rfleet_api.hip", "reflector_ekf_slam_amd/fleet.py", "scripts/fleet_track_bench.py"]
N_SEEDS = 8
N_ODOM = 5


def stats(us):
    s = sorted(us)
    return {"min": s[0], "median": float(np.median(s)), "max": s[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fleet-sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import fleet_bench
    from reflector_ekf_slam_amd import ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd import session as S
    total = args.warmup + args.ticks
    sessions, snaps, steady = fleet_bench.build_maps(total)
    result = {"workload": "B members, each SessionConfig(n_landmarks=128, obs_per_scan=16), seeds 7000 + i mod 8, maps built (n = 259); a "
                          f"tick is {N_ODOM} odometry messages and one steady-state scan per member",
              "unit": "us per tick (host clock around work that ends in a synchronisation)", "reps": args.reps, "ticks": args.ticks,
              "warmup": args.warmup, "messages_per_tick_per_member": N_ODOM + 1, "untracked_submit_sync": {},
              "tracked_submit_take_track": {}, "submit_poses_per_message": {}, "per_message_min_over_tracked_max": {},
              "tracked_median_over_untracked_median": {}, "tracked_is_a_speed_up_over_per_message": {}, "records_per_take": {}}

    for B in args.fleet_sizes:
        fl = ReflectorEKFSLAMFleet([S.options_for(sessions[b % N_SEEDS]) for b in range(B)], max_landmarks=128)

        def messages(k, b):
            """Member b's messages of tick k: N_ODOM odometry messages spread over the interval in front of its scan, then the scan."""
            sc = steady[b % N_SEEDS]
            t1 = sc[k][0]
            t0 = sc[k - 1][0] if k else snaps[b % N_SEEDS].time
            # (the steady-state scans are taken standing still: the odometer reports noise of alternating sign, which does not drift)
            od = [(b, 0, t0 + (t1 - t0) * (j + 1) / (N_ODOM + 1), (0.01 * (-1) ** (k * N_ODOM + j), 0.0, 0.005 * (-1) ** (k * N_ODOM + j)), None)
                  for j in range(N_ODOM)]
            return od + [(b, 1, t1, (0.0, 0.0, 0.0), sc[k][1])]

        per_member = [[messages(k, b) for b in range(B)] for k in range(total)]
        packed_tick = [fl.pack([ev for msgs in per_member[k] for ev in msgs]) for k in range(total)]
        packed_rank = [[fl.pack([msgs[j] for msgs in per_member[k]]) for j in range(N_ODOM + 1)] for k in range(total)]
        taken = []

        def restart():
            fl.sync()
            for b in range(B):
                st = snaps[b % N_SEEDS]
                fl.set_state(b, st.time, st.mu, st.sigma, vt=np.zeros(3))

        def tick_untracked(k):
            fl.submit_packed(packed_tick[k])
            fl.sync()

        def tick_tracked(k):
            fl.submit_packed(packed_tick[k])
            taken.append(sum(len(t) for t in fl.take_track()))

        def tick_per_message(k):
            for p in packed_rank[k]:
                fl.submit_packed(p)
                fl.poses()

        ra, rb, rc = [], [], []
        for _ in range(args.reps):
            for leg, acc, tracked in ((tick_untracked, ra, False), (tick_tracked, rb, True), (tick_per_message, rc, False)):
                restart()
                fl.track(tracked)
                for k in range(args.warmup):
                    leg(k)
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    leg(k)
                acc.append(1e6 * (time.perf_counter() - t0) / args.ticks)
        assert (fl.n() == 259).all() and not fl.flags().any()
        assert set(taken) == {B * (N_ODOM + 1)}, sorted(set(taken))
        fl.close()
        key = str(B)
        result["untracked_submit_sync"][key], result["tracked_submit_take_track"][key], result["submit_poses_per_message"][key] = stats(ra), stats(rb), stats(rc)
        result["per_message_min_over_tracked_max"][key] = min(rc) / max(rb)
        result["tracked_median_over_untracked_median"][key] = float(np.median(rb)) / float(np.median(ra))
        result["tracked_is_a_speed_up_over_per_message"][key] = bool(max(rb) < min(rc))
        result["records_per_take"][key] = B * (N_ODOM + 1)

    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
