"""Wide scans in the fleet, measured: B C2-sized sessions (128 reflectors, maps built) advanced one WIDE scan per member per tick,
at K = 48 observations (two block steps of k_fleet_step_wide) and K = 96 (three),

* ``fleet``:   one rfleet_submit per tick on a fleet with wide scans switched on (ONE launch of k_fleet_step_wide);
* ``handles``: the same scans through B ReflectorEKFSLAM handles (max_landmarks=128, auto_grow=False), which take wide scans
  themselves, fed round-robin from this thread -- the only way to serve such robots without wide scans in the fleet.

The protocol is scripts/fleet_bench.py's: both legs in the same process, alternating, --reps repetitions each; every repetition
restarts from the same built maps (set_state), warms up and then times --ticks ticks with the host clock around work that ends in a
synchronisation.  The scans are taken from each session's final pose with the range gate opened so that the K nearest of its 128
reflectors are in view; all of them are in the state, so every observation is matched and nothing is appended.  Prints ONE JSON
line (and writes it to --out): updates/s (min / median / max), us per tick, the fleet's minimum over the handles' maximum at each
size (below 1: the handles were faster), the largest |mu - handles' mu| at the end, and the SHA-256 of the sources it was measured on.

  python scripts/fleet_wide_bench.py --out profiles/fleet_wide_bench.json
"""
from __future__ import annotations

import argparse
import dataclasses
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
           "reflector_ekf_slam_amd/csrc/fleet_wide.hip", "reflector_ekf_slam_amd/csrc/rfleet_api.hip", "reflector_ekf_slam_amd/fleet.py",
           "scripts/fleet_wide_bench.py"]
WIDTHS = (48, 96)
OPEN_RANGE = 100.0            # metres: every reflector of a 128-reflector session is inside


def wide_scans_of(session, K, n):
    from reflector_ekf_slam_amd import synth
    cfg = dataclasses.replace(session.config, obs_per_scan=K, range_max=OPEN_RANGE)
    scans = synth.steady_state_scans(dataclasses.replace(session, config=cfg), n)
    assert all(c.shape == (K, 2) for _, c in scans), (K, scans[0][1].shape)
    return scans


def stats(rates):
    r = sorted(rates)
    return {"min": r[0], "median": float(np.median(r)), "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import fleet_bench as FB
    from reflector_ekf_slam_amd import ReflectorEKFSLAM, ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd import session as S
    total = args.warmup + args.ticks
    N = FB.N_SEEDS
    sessions, snaps, _ = FB.build_maps(1)
    result = {"workload": "B members, each SessionConfig(n_landmarks=128), seeds 7000 + i mod 8; maps built (n = 259), then one scan of the K "
                          "nearest reflectors per member per tick, all matched", "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps,
              "unit": "updates/s (aggregate, one GPU, one host thread)", "widths": {}}
    for K in WIDTHS:
        steady = [wide_scans_of(s, K, total) for s in sessions]
        rec = {"blocks": (K + 31) // 32, "fleet": {}, "handles": {}, "fleet_min_over_handles_max": {}, "fleet_is_a_speed_up_over_handles": {},
               "max_abs_mu_diff": {}}
        for B in sorted(args.sizes):
            fl = ReflectorEKFSLAMFleet([S.options_for(sessions[b % N]) for b in range(B)], max_landmarks=128, wide_scans=True)
            packed = [fl.pack([(b, 1, steady[b % N][k][0], (0.0, 0.0, 0.0), steady[b % N][k][1]) for b in range(B)]) for k in range(total)]
            handles = [ReflectorEKFSLAM(S.options_for(sessions[b % N]), max_landmarks=128, device=0, auto_grow=False) for b in range(B)]
            rf, rh = [], []
            for _ in range(args.reps):
                for b in range(B):
                    st = snaps[b % N]
                    fl.set_state(b, st.time, st.mu, st.sigma)
                for k in range(args.warmup):
                    fl.submit_packed(packed[k])
                fl.sync()
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    fl.submit_packed(packed[k])
                fl.sync()
                rf.append(B * args.ticks / (time.perf_counter() - t0))
                for b, g in enumerate(handles):
                    st = snaps[b % N]
                    g.set_state(st.time, st.mu, st.sigma)
                    g.sync()
                for k in range(args.warmup):
                    for b, g in enumerate(handles):
                        g.handle_observation(*steady[b % N][k])
                for g in handles:
                    g.sync()
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    for b, g in enumerate(handles):
                        g.handle_observation(*steady[b % N][k])
                for g in handles:
                    g.sync()
                rh.append(B * args.ticks / (time.perf_counter() - t0))
            launches, scans = fl.wide_counts()
            assert launches == args.reps * total and scans == launches * B, (launches, scans)
            m = fl.last_match(0)
            assert m.state_obs_match_ids.shape[0] == K and m.new_ids.shape[0] == 0, (K, m.state_obs_match_ids.shape, m.new_ids.shape)
            rec["fleet"][str(B)] = dict(stats(rf), us_per_tick=1e6 * B / float(np.median(rf)), flags_any=bool(fl.flags().any()))
            rec["handles"][str(B)] = dict(stats(rh), us_per_tick=1e6 * B / float(np.median(rh)))
            rec["fleet_min_over_handles_max"][str(B)] = min(rf) / max(rh)
            rec["fleet_is_a_speed_up_over_handles"][str(B)] = bool(min(rf) > max(rh))
            rec["max_abs_mu_diff"][str(B)] = max(float(np.abs(fl.get_state(b, want_sigma=False).mu - handles[b].mu()).max()) for b in range(B))
            fl.close()
            for g in handles:
                g.close()
        result["widths"][str(K)] = rec
    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
