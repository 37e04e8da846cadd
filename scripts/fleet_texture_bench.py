"""Fleet texture export, measured: B robots, each with its OWN 480 x 480 map at 0.05 m built by ScanMatchFleet.insert from the scans
of scripts/fleet_insert_bench.py; one call draws the submap texture of every robot (MapBuilder::ToSubmapTexture),

* ``batch``:   one ScanMatchFleet.draw_textures per call (ONE launch of kgb_texture, one workgroup per slot, one wait; the maps stay in
  the batch handle's resident slots);
* ``packed``:  the two C calls alone with the slot list and the result buffers made once outside the timed region (what a C++ host
  pays); its time is split in two by the buffer protocol -- a first collect without room waits for the launch and returns the boxes
  (the DEVICE part: submit, kernel, its writes over the link, the wait), the second one copies the textures out (the COPY part);
* ``handles``: the same grids in B GridFrontEnd handles, DrawTexture() each, round robin on this thread -- the only way to get a
  fleet's textures without the batch short of GetGrid and a crop on the host.

All legs run in the same process, alternating, --reps repetitions each; every repetition warms up and then times --calls calls with
the host clock.  In every repetition the first and the last member's texture of the batch must equal the handles' byte for byte.
Prints ONE JSON line (and writes it to --out): textures/s as min / median / max, us per call, and the SHA-256 of the sources it was
measured on.  A speed-up is claimed only where the batch's minimum exceeds the handles' maximum.

  python scripts/fleet_texture_bench.py --out profiles/fleet_texture_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
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
           "scripts/fleet_texture_bench.py", "scripts/fleet_insert_bench.py"]
N_INSERTS = 6         # scans inserted into every member's map before it is drawn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    L = M._texture_lib()
    base = make_scans()
    empty = np.zeros((N_CELLS, N_CELLS), np.uint16)
    total = args.warmup + args.calls
    legs = ("batch", "packed", "handles")
    result = {"workload": f"B members, each with its own {N_CELLS} x {N_CELLS} map at {RES} m holding {N_INSERTS} inserted {N_RETURNS}-return scans "
                          f"(member b inserts scans b .. b + {N_INSERTS - 1} mod {N_POSES} of scripts/fleet_insert_bench.py); one call draws every member's texture",
              "calls": args.calls, "warmup": args.warmup, "reps": args.reps, "unit": "textures/s (aggregate, one GPU, one host thread)",
              "kernel": "kgb_texture: one workgroup of 512 threads per slot, the byte-pair table read through L2; more than one workgroup "
                        "per slot and the table in LDS were not tried"}
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
        ids = np.arange(B, dtype=np.int32)
        boxes, sm, offs = np.zeros((B, 4), np.int32), np.zeros((B, 2)), np.zeros(B, dtype=C.c_long)
        out = np.zeros(2 * empty.size * B, np.uint8)
        rates = {leg: [] for leg in legs}
        device_us, copy_us, tex_bytes = [], [], 0
        for _ in range(args.reps):
            ends = {}
            for leg in legs:
                dt = dev = cp = 0.0
                for k in range(total):
                    if leg == "handles":
                        t0 = time.perf_counter()
                        tex = [g.DrawTexture() for g in handles]
                        t1 = time.perf_counter()
                        ends[leg] = [tex[0], tex[-1]]
                    elif leg == "packed":
                        t0 = time.perf_counter()
                        rc0 = L.rgrid_batch_texture_submit(fm._h, ids.ctypes.data, B)
                        rc1 = L.rgrid_batch_texture_collect(fm._h, boxes.ctypes.data, sm.ctypes.data, offs.ctypes.data, None, 0)
                        tm = time.perf_counter()
                        rc2 = L.rgrid_batch_texture_collect(fm._h, boxes.ctypes.data, sm.ctypes.data, offs.ctypes.data, out.ctypes.data, out.size)
                        t1 = time.perf_counter()
                        assert (rc0, rc1, rc2) == (0, M.RGRID_ERR_BUFFER, 0)
                        if k >= args.warmup:
                            dev += tm - t0
                            cp += t1 - tm
                        tex_bytes = int(2 * (boxes[:, 2].astype(np.int64) * boxes[:, 3]).sum())
                    else:
                        t0 = time.perf_counter()
                        tex = fm.draw_textures(ids)
                        t1 = time.perf_counter()
                        ends[leg] = [tuple(tex[0]), tuple(tex[-1])]
                    if k >= args.warmup:
                        dt += t1 - t0
                rates[leg].append(B * args.calls / dt)
                if leg == "packed":
                    device_us.append(1e6 * dev / args.calls)
                    copy_us.append(1e6 * cp / args.calls)
                    last = int(offs[B - 1])
                    ends[leg] = [(out[:2 * boxes[0, 2] * boxes[0, 3]].reshape(boxes[0, 3], boxes[0, 2], 2), tuple(boxes[0]), tuple(sm[0])),
                                 (out[last:last + 2 * boxes[B - 1, 2] * boxes[B - 1, 3]].reshape(boxes[B - 1, 3], boxes[B - 1, 2], 2),
                                  tuple(boxes[B - 1]), tuple(sm[B - 1]))]
            for leg in legs[:2]:                                    # every leg draws the same textures
                for a, h in zip(ends[leg], ends["handles"]):
                    assert tuple(int(v) for v in a[1]) == tuple(h[1]) and tuple(float(v) for v in a[2]) == tuple(h[2]) and np.array_equal(a[0], h[0]), leg
        for leg in legs:
            result[leg][str(B)] = dict(stats(rates[leg]), us_per_call=1e6 * B / float(np.median(rates[leg])))
        result["packed"][str(B)].update(device_us=stats(device_us), copy_us=stats(copy_us), texture_bytes_per_call=tex_bytes)
        result.setdefault("batch_min_over_handles_max", {})[str(B)] = result["batch"][str(B)]["min"] / result["handles"][str(B)]["max"]
        result.setdefault("packed_min_over_handles_max", {})[str(B)] = result["packed"][str(B)]["min"] / result["handles"][str(B)]["max"]
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
