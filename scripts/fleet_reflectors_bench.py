"""What publishing costs a fleet host, measured: the reflectors of B C2-sized members at capacity (128 reflectors each, the world
of scripts/fleet_bench.py), read

* ``batch_ellipses``: ``fleet.marker_ellipses()`` of all members -- ONE launch of k_fleet_reflectors and one synchronisation;
* ``batch_all``:      ellipses, positions and blocks together (``fleet.reflectors(ellipses, xy, cov)``), the same launch;
* ``baseline``:       the only route there was before rfleet_get_reflectors, on the same build and the same fleet:
                      ``fleet.get_state(i)`` per member (a synchronisation, an ld x n copy and the host's mirror loop each) plus
                      the ellipse arithmetic in numpy on the host;

and one tick of ``submit`` followed by ``sync()`` against one followed by ``marker_ellipses()`` (the node publishes after every
scan).  All legs run in the same process, alternating, --reps repetitions each; a repetition times a loop of calls that each end
in a synchronisation with the host clock, and reports us per call.  Prints ONE JSON line and writes it to --out.

  python scripts/fleet_reflectors_bench.py --out profiles/fleet_reflectors_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

EPS = 2.220446049250313e-16
N_SEEDS = 8


def host_ellipses(state):
    """k_ellipses' arithmetic (src/ros_node.cc:750-765) on the host, vectorised over a state's reflectors: -> [L, 5]."""
    n = state.mu.shape[0]
    idx = np.arange(3, n, 2)
    a, c, d = state.sigma[idx, idx], state.sigma[idx + 1, idx], state.sigma[idx + 1, idx + 1]
    with np.errstate(all="ignore"):
        p = 0.5 * (a - d)
        z = np.sqrt(np.abs(p * p + c * c))
        pz = np.where(p >= 0.0, p + z, p - z)
        d0 = d + pz
        d1 = np.where(pz != 0.0, d - c * c / np.where(pz != 0.0, pz, 1.0), d0)
        small = np.abs(c) <= EPS * (np.abs(a) + np.abs(d))
        d0, d1 = np.where(small, a, d0), np.where(small, d, d1)
        vx, vy = np.where(small, 1.0, pz), np.where(small, 0.0, c)
        return np.stack([state.mu[idx], state.mu[idx + 1], np.arctan2(vy, vx), 2.0 * np.sqrt(d0 * 5.991), 2.0 * np.sqrt(d1 * 5.991)], -1)


def stats(us):
    s = sorted(us)
    return {"min": s[0], "median": float(np.median(s)), "max": s[-1]}


def timed(call, calls):
    """us per call of `calls` calls, each of which ends in a synchronisation."""
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    return 1e6 * (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fleet-sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--batch-calls", type=int, default=1000)
    ap.add_argument("--baseline-members", type=int, default=2048, help="get_state calls per baseline repetition (calls = this / B)")
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import fleet_bench
    from reflector_ekf_slam_amd import ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd import session as S
    total = args.warmup + args.ticks
    sessions, snaps, steady = fleet_bench.build_maps(total)
    result = {"workload": "B members, each SessionConfig(n_landmarks=128, obs_per_scan=16), seeds 7000 + i mod 8, maps built: 128 "
                          "reflectors per member (n = 259, ld = 272)", "unit": "us per call (host clock around calls that end in a synchronisation)",
              "reps": args.reps, "batch_calls_per_rep": args.batch_calls, "ticks": args.ticks, "warmup": args.warmup,
              "batch_ellipses": {}, "batch_all": {}, "baseline": {}, "baseline_calls_per_rep": {}, "tick_submit_sync": {},
              "tick_submit_marker_ellipses": {}, "max_abs_diff_batch_vs_baseline": {}}

    for B in args.fleet_sizes:
        fl = ReflectorEKFSLAMFleet([S.options_for(sessions[b % N_SEEDS]) for b in range(B)], max_landmarks=128)
        packed = [fl.pack([(b, 1, steady[b % N_SEEDS][k][0], (0.0, 0.0, 0.0), steady[b % N_SEEDS][k][1]) for b in range(B)])
                  for k in range(total)]

        def restart():
            for b in range(B):
                st = snaps[b % N_SEEDS]
                fl.set_state(b, st.time, st.mu, st.sigma)

        def baseline():
            return [host_ellipses(fl.get_state(b)) for b in range(B)]

        def tick_sync(k):
            fl.submit_packed(packed[k])
            fl.sync()

        def tick_publish(k):
            fl.submit_packed(packed[k])
            fl.marker_ellipses()

        restart()
        got, want = fl.marker_ellipses(), baseline()
        assert [g.shape for g in got] == [(128, 5)] * B
        result["max_abs_diff_batch_vs_baseline"][str(B)] = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
        base_calls = max(3, args.baseline_members // B)
        for _ in range(3):                                   # warm every shape the timed windows use
            fl.marker_ellipses()
            fl.reflectors(ellipses=True, xy=True, cov=True)
        re_, ra, rb, ts, tp = [], [], [], [], []
        for _ in range(args.reps):
            re_.append(timed(fl.marker_ellipses, args.batch_calls))
            ra.append(timed(lambda: fl.reflectors(ellipses=True, xy=True, cov=True), args.batch_calls))
            rb.append(timed(baseline, base_calls))
            for leg, acc in ((tick_sync, ts), (tick_publish, tp)):
                restart()
                for k in range(args.warmup):
                    leg(k)
                t0 = time.perf_counter()
                for k in range(args.warmup, total):
                    leg(k)
                acc.append(1e6 * (time.perf_counter() - t0) / args.ticks)
        assert (fl.n() == 259).all()
        fl.close()
        key = str(B)
        result["batch_ellipses"][key], result["batch_all"][key], result["baseline"][key] = stats(re_), stats(ra), stats(rb)
        result["baseline_calls_per_rep"][key] = base_calls
        result["tick_submit_sync"][key], result["tick_submit_marker_ellipses"][key] = stats(ts), stats(tp)

    if "64" in result["baseline"]:
        b, e, a = result["baseline"]["64"], result["batch_ellipses"]["64"], result["batch_all"]["64"]
        result["baseline64_min_over_batch_ellipses64_max"] = b["min"] / e["max"]
        result["baseline64_min_over_batch_all64_max"] = b["min"] / a["max"]
        result["batch_is_a_speed_up_over_get_state"] = bool(e["max"] < b["min"] and a["max"] < b["min"])
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
