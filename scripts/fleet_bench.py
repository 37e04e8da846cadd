"""Fleet serving, measured: B C2-sized sessions advanced one scan per tick,

* ``fleet``:   one rfleet_submit per tick (ONE launch of k_fleet_step, one workgroup per member);
* ``handles``: the same scans through B ReflectorEKFSLAM handles (max_landmarks=128, auto_grow=False) fed round-robin from
  this thread -- what bench.py's multi_session does and the only way to serve a fleet without the fleet filter.

* ``fleet_pose_fix`` (opt-in, --pose-fix; B = 64 and 256): the fleet leg with an absolute pose fix on every scan (the
  USE_GPS deployment: three more rows on each member's update), next to the plain fleet leg of the same size.

* ``fleet_map`` (opt-in, --map; B = 64 and 256): C2-sized members (capacity 128) that LOCALISE against one shared 128-point
  pre-loaded map (rfleet_set_map): every member starts with n = 3 at seed 7000's pose, every scan's 16 reflectors are in the map
  (the map is that session's built map, weights 0.01 I as in tests/golden/map_L24_obs8.npz), next to the plain fleet leg of the
  same size; and ``handles_map``: the same scans through 64 ReflectorEKFSLAM handles with ``set_map``.

All legs run in the same process, alternating, --reps repetitions each; every repetition restarts from the same built maps
(set_state), warms up and then times --ticks ticks with the host clock around work that ends in a synchronisation.  Prints
ONE JSON line (and writes it to --out) with the aggregate updates/s (min / median / max), us per tick, the largest
|mu - handles' mu| per member at the end, and the SHA-256 of the fleet sources it was measured on.

  python scripts/fleet_bench.py --pose-fix --map --out profiles/fleet_bench.json
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/fleet_bench.py --only-fleet 256 --reps 1     (k_fleet_step's own time)
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

SOURCES = ["include/rfleet.h", "reflector_ekf_slam_amd/csrc/fleet_dev.h", "reflector_ekf_slam_amd/csrc/fleet_host.h", "reflector_ekf_slam_amd/csrc/fleet_kernels.hip",
           "reflector_ekf_slam_amd/csrc/rfleet_api.hip", "reflector_ekf_slam_amd/fleet.py", "scripts/fleet_bench.py"]
N_SEEDS = 8
POSE_FIX_SIZES = (64, 256)
MAP_SIZES = (64, 256)
MAP_HANDLES = 64
MAP_WEIGHT = 0.01
FIX_SIGMA = (0.05, 0.05, 0.017)


def build_maps(ticks_total):
    """The eight sessions' maps, built by an eight-member fleet (whole sessions), and their steady-state scans."""
    from reflector_ekf_slam_amd import ReflectorEKFSLAMFleet, synth
    from reflector_ekf_slam_amd import session as S
    sessions = [synth.make_session(synth.SessionConfig(f"fleet_c2_{i}", 128, 16, synth.DIFF, seed=7000 + i)) for i in range(N_SEEDS)]
    fl = ReflectorEKFSLAMFleet([S.options_for(s) for s in sessions], max_landmarks=128)
    pos, first = [0] * N_SEEDS, [True] * N_SEEDS
    while any(pos[i] < sessions[i].n_events for i in range(N_SEEDS)):
        batch = []
        for i, s in enumerate(sessions):
            while pos[i] < s.n_events:
                e = pos[i]
                pos[i] += 1
                if s.ev_type[e] == synth.EV_ODOM:
                    batch.append((i, 0, float(s.ev_time[e]), tuple(float(v) for v in s.odom[e]), None))
                elif first[i]:
                    first[i] = False
                else:
                    batch.append((i, 1, float(s.ev_time[e]), (0.0, 0.0, 0.0), s.obs_of(e)))
                    break
        fl.submit(batch)
    snaps = []
    for i in range(N_SEEDS):
        st = fl.get_state(i)
        assert st.mu.shape[0] == 259, st.mu.shape
        snaps.append(st)
    assert not fl.flags().any()
    fl.close()
    steady = [synth.steady_state_scans(s, ticks_total) for s in sessions]
    return sessions, snaps, steady


def make_fixes(sessions, snaps, steady, total):
    """One fix per seed and tick, as a scan matcher started from PredictState would hand it back: the pose predict_poses gives
    at the scan's time plus seeded noise, drawn on a run of the eight maps that applies them."""
    from reflector_ekf_slam_amd import ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd import session as S
    fl = ReflectorEKFSLAMFleet([S.options_for(s) for s in sessions], max_landmarks=128)
    for i, st in enumerate(snaps):
        fl.set_state(i, st.time, st.mu, st.sigma)
    rng = np.random.default_rng(7900)
    fixes = []
    for k in range(total):
        mu, _ = fl.predict_poses([steady[i][k][0] for i in range(N_SEEDS)])
        fx = mu + rng.normal(size=mu.shape) * FIX_SIGMA
        fixes.append(fx)
        fl.submit([(i, 1, steady[i][k][0], (0.0, 0.0, 0.0), steady[i][k][1], tuple(fx[i])) for i in range(N_SEEDS)])
    assert not fl.flags().any()
    fl.close()
    return fixes


def stats(rates):
    r = sorted(rates)
    return {"min": r[0], "median": float(np.median(r)), "max": r[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fleet-sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--handle-sizes", type=int, nargs="*", default=[4, 64])
    ap.add_argument("--only-fleet", type=int, default=0, help="run the fleet leg at this size only (profiling runs)")
    ap.add_argument("--pose-fix", action="store_true", help="add the fleet leg with a pose fix on every scan (B = 64, 256)")
    ap.add_argument("--map", action="store_true", help="add the leg that localises against one shared 128-point map (B = 64, 256; 64 handles)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.only_fleet:
        args.fleet_sizes, args.handle_sizes = [args.only_fleet], []

    from reflector_ekf_slam_amd import ReflectorEKFSLAM, ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd import session as S
    total = args.warmup + args.ticks
    sessions, snaps, steady = build_maps(total)
    result = {"workload": "B members, each SessionConfig(n_landmarks=128, obs_per_scan=16), seeds 7000 + i mod 8; maps built, then one "
                          "steady-state scan per member per tick", "ticks": args.ticks, "warmup": args.warmup, "reps": args.reps,
              "unit": "updates/s (aggregate, one GPU, one host thread)", "fleet": {}, "handles": {}, "max_abs_mu_diff": {}}
    fixes = None
    if args.pose_fix:
        fixes = make_fixes(sessions, snaps, steady, total)
        result["fleet_pose_fix"] = {}

    map_xy = map_cov = None
    if args.map:
        map_xy = np.ascontiguousarray(snaps[0].mu[3:].reshape(-1, 2), np.float32)         # seed 7000's built map: 128 points
        map_cov = np.tile(np.array([MAP_WEIGHT, 0.0, 0.0, MAP_WEIGHT]), (map_xy.shape[0], 1))
        result["fleet_map"], result["handles_map"] = {}, {}
        result["fleet_map_workload"] = (f"B members at n = 3 (seed 7000's pose and pose block), one shared {map_xy.shape[0]}-point map, weights "
                                        f"{MAP_WEIGHT} I, seed 7000's steady-state scans (16 reflectors each, all in the map)")

    def start_localising(set_state, st):
        set_state(st.time, st.mu[:3].copy(), np.ascontiguousarray(st.sigma[:3, :3]))

    for B in sorted(set(args.fleet_sizes) | set(args.handle_sizes)):
        fl = handles = flm = hmap = None
        packed_map = None
        if args.map and B in MAP_SIZES and B in args.fleet_sizes:
            flm = ReflectorEKFSLAMFleet([S.options_for(sessions[0]) for _ in range(B)], max_landmarks=128)
            flm.set_map(map_xy, map_cov)
            packed_map = [flm.pack([(b, 1, steady[0][k][0], (0.0, 0.0, 0.0), steady[0][k][1]) for b in range(B)]) for k in range(total)]
            if B == MAP_HANDLES:
                hmap = [ReflectorEKFSLAM(S.options_for(sessions[0]), max_landmarks=128, device=0, auto_grow=False) for _ in range(B)]
                for g in hmap:
                    g.set_map(map_xy, map_cov)
        if B in args.fleet_sizes:
            fl = ReflectorEKFSLAMFleet([S.options_for(sessions[b % N_SEEDS]) for b in range(B)], max_landmarks=128)
            packed = [fl.pack([(b, 1, steady[b % N_SEEDS][k][0], (0.0, 0.0, 0.0), steady[b % N_SEEDS][k][1]) for b in range(B)])
                      for k in range(total)]
        packed_fix = None
        if fl is not None and fixes is not None and B in POSE_FIX_SIZES:
            packed_fix = [fl.pack([(b, 1, steady[b % N_SEEDS][k][0], (0.0, 0.0, 0.0), steady[b % N_SEEDS][k][1], tuple(fixes[k][b % N_SEEDS]))
                                   for b in range(B)]) for k in range(total)]
        if B in args.handle_sizes:
            handles = [ReflectorEKFSLAM(S.options_for(sessions[b % N_SEEDS]), max_landmarks=128, device=0, auto_grow=False) for b in range(B)]
        rf, rh, rp, rm, rhm = [], [], [], [], []
        for _ in range(args.reps):
            if flm is not None:
                for b in range(B):
                    start_localising(lambda *a: flm.set_state(b, *a), snaps[0])
                for k in range(args.warmup):
                    flm.submit_packed(packed_map[k])
                flm.sync()
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    flm.submit_packed(packed_map[k])
                flm.sync()
                rm.append(B * args.ticks / (time.perf_counter() - t0))
            if hmap is not None:
                for g in hmap:
                    start_localising(g.set_state, snaps[0])
                    g.sync()
                for k in range(args.warmup):
                    for g in hmap:
                        g.handle_observation(*steady[0][k])
                for g in hmap:
                    g.sync()
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    for g in hmap:
                        g.handle_observation(*steady[0][k])
                for g in hmap:
                    g.sync()
                rhm.append(B * args.ticks / (time.perf_counter() - t0))
            if packed_fix is not None:                       # (first: the fleet's final state is the plain leg's)
                for b in range(B):
                    st = snaps[b % N_SEEDS]
                    fl.set_state(b, st.time, st.mu, st.sigma)
                for k in range(args.warmup):
                    fl.submit_packed(packed_fix[k])
                fl.sync()
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    fl.submit_packed(packed_fix[k])
                fl.sync()
                rp.append(B * args.ticks / (time.perf_counter() - t0))
            if fl is not None:
                for b in range(B):
                    st = snaps[b % N_SEEDS]
                    fl.set_state(b, st.time, st.mu, st.sigma)
                for k in range(args.warmup):
                    fl.submit_packed(packed[k])
                fl.sync()
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    fl.submit_packed(packed[k])
                fl.sync()
                rf.append(B * args.ticks / (time.perf_counter() - t0))
            if handles is not None:
                for b, g in enumerate(handles):
                    st = snaps[b % N_SEEDS]
                    g.set_state(st.time, st.mu, st.sigma)
                    g.sync()
                for k in range(args.warmup):
                    for b, g in enumerate(handles):
                        g.handle_observation(*steady[b % N_SEEDS][k])
                for g in handles:
                    g.sync()
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    for b, g in enumerate(handles):
                        g.handle_observation(*steady[b % N_SEEDS][k])
                for g in handles:
                    g.sync()
                rh.append(B * args.ticks / (time.perf_counter() - t0))
        if fl is not None:
            result["fleet"][str(B)] = dict(stats(rf), us_per_tick=1e6 * B / float(np.median(rf)), flags_any=bool(fl.flags().any()))
        if packed_fix is not None:
            us_fix, us_plain = 1e6 * B / float(np.median(rp)), 1e6 * B / float(np.median(rf))
            result["fleet_pose_fix"][str(B)] = dict(stats(rp), us_per_tick=us_fix, extra_us_per_tick_over_plain=us_fix - us_plain,
                                                    flags_any=bool(fl.flags().any()))
        if flm is not None:
            n_end = flm.n()
            result["fleet_map"][str(B)] = dict(stats(rm), us_per_tick=1e6 * B / float(np.median(rm)), flags_any=bool(flm.flags().any()),
                                               n_max_at_end=int(n_end.max()), map_pairs_last_scan=int(flm.last_match(0).map_obs_match_ids.shape[0]))
            if fl is not None:
                result["fleet_map"][str(B)]["us_per_tick_minus_plain"] = 1e6 * B / float(np.median(rm)) - 1e6 * B / float(np.median(rf))
        if hmap is not None:
            result["handles_map"][str(B)] = dict(stats(rhm), us_per_tick=1e6 * B / float(np.median(rhm)))
            result["fleet_map"][str(B)]["max_abs_mu_diff_to_handles"] = max(
                float(np.abs(flm.get_state(b, want_sigma=False).mu - hmap[b].mu()).max()) for b in range(B))
            result["fleet_map_min_over_handles_map_max"] = min(rm) / max(rhm)
            result["fleet_map_is_a_speed_up_over_handles"] = bool(min(rm) > max(rhm))
        if handles is not None:
            result["handles"][str(B)] = dict(stats(rh), us_per_tick=1e6 * B / float(np.median(rh)))
        if fl is not None and handles is not None:
            result["max_abs_mu_diff"][str(B)] = max(float(np.abs(fl.get_state(b, want_sigma=False).mu - handles[b].mu()).max())
                                                    for b in range(B))
        if fl is not None:
            fl.close()
        for g in (handles or []) + (hmap or []):
            g.close()
        if flm is not None:
            flm.close()

    f, h = result["fleet"], result["handles"]
    if "64" in f and "64" in h:
        result["fleet64_min_over_handles64_max"] = f["64"]["min"] / h["64"]["max"]
    if "64" in f and "256" in f:
        result["fleet256_median_over_fleet64_median"] = f["256"]["median"] / f["64"]["median"]
    if "256" in f and h:
        result["fleet256_median_over_best_handles_median"] = f["256"]["median"] / max(v["median"] for v in h.values())
    result["_sources_sha256"] = {rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
