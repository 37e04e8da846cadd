"""The fleet detectors' host text (csrc/det_batch_host.h: check_members, the 2D submit's validate / plan_tables / pack_scans and
fill_angle_table, the 3D submit's validate / pack_clouds, the range-data plan, fill_link and the collect rule), built host-only and run
without a GPU (tests/cpp/det_batch_host.cpp), against a second, independent text of the rules as include/rdet.h, include/rlink.h and the
headers of csrc/det2d_batch.hip / det3d_batch.hip document them, written below with numpy.  Everything is compared exactly: floats by
their bits, records by their bytes (the program packs into heap buffers of exactly the size the handle allocates, pre-filled with 0xA5,
so the padding is part of the comparison)."""
from __future__ import annotations

import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, BAD_SCAN, CAPACITY, BUFFER = 0, -1, -3, -4, -5   # include/rdet.h
MAX_CENTERS, TABLES, MAX_BEAMS, RANGE_TILE, MAX_BRIGHT, CLOUD_TILE = 256, 8, 8192, 512, 5120, 64

ODOM = np.dtype([(n, "<f8") for n in ("time", "px", "py", "yaw", "vx", "vy", "wz")])
REC2 = np.dtype([("intensity_min", "<f8"), ("min_length", "<f8"), ("length_error", "<f8"), ("first_point_time", "<f8"), ("point_delta_t", "<f8"),
                 ("front", ODOM), ("back", ODOM), ("n_odom", "<i4"), ("opt_range_min", "<f4"), ("opt_range_max", "<f4"), ("msg_range_min", "<f4"),
                 ("msg_range_max", "<f4"), ("angle_increment", "<f4"), ("N", "<i4"), ("is_circle", "<i4"), ("member", "<i4"), ("table", "<i4"),
                 ("run", "<i4"), ("s2b_x", "<f4"), ("s2b_y", "<f4"), ("s2b_a", "<f4"), ("s2b_c", "<f4"), ("s2b_s", "<f4")], align=True)
REC3 = np.dtype([("intensity_min", "<f8"), ("stamp", "<f8"), ("member", "<i4"), ("N", "<i4"), ("slot", "<i4"), ("pad", "<i4"), ("sx", "<f4"),
                 ("sy", "<f4"), ("cs", "<f4"), ("sn", "<f4")], align=True)
RANGE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("n", "<i4"), ("pad", "<i4")], align=True)
assert (REC2.itemsize, REC3.itemsize, RANGE.itemsize) == (216, 48, 24)

_libm = ctypes.CDLL("libm.so.6")
for _f in (_libm.cosf, _libm.sinf):
    _f.restype, _f.argtypes = ctypes.c_float, [ctypes.c_float]


def cosf(v):
    return np.float32(_libm.cosf(ctypes.c_float(float(v))))


def sinf(v):
    return np.float32(_libm.sinf(ctypes.c_float(float(v))))


def from_bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def h(v):
    return float(v).hex()


PI32 = np.float32(math.pi)


def scan(member, N=8, stamp=100.0, amin=-PI32, amax=PI32, inc=None, scan_time=0.1, rmin=0.1, rmax=30.0, rnull=False, inull=False):
    """One rdet2d_scan; the float fields are float32 as the struct's are."""
    inc = np.float32(2 * math.pi / max(N, 1)) if inc is None else inc
    return dict(member=member, stamp=float(stamp), amin=np.float32(amin), amax=np.float32(amax), inc=np.float32(inc), scan_time=np.float32(scan_time),
                rmin=np.float32(rmin), rmax=np.float32(rmax), N=N, rnull=rnull, inull=inull)


def scan_line(s):
    return "%d %s %s %d %d %d" % (s["member"], h(s["stamp"]), " ".join("%08x" % bits(s[k]) for k in ("amin", "amax", "inc", "scan_time", "rmin", "rmax")),
                                  s["N"], s["rnull"], s["inull"])


# ---- the second text -------------------------------------------------------------------------------------------------------------
def first_bad(lst, B):
    """The first entry that names no member or one named before it (rdet.h: "a member out of range or listed twice")."""
    for g, m in enumerate(lst):
        if not 0 <= m < B or m in lst[:g]:
            return g
    return len(lst)


def validate2(scans, B, max_beams):
    """rdet2d_batch_submit's refusals: the first offending scan in call order decides the code."""
    named = set()
    for s in scans:
        if not 0 <= s["member"] < B or s["member"] in named or s["N"] < 0 or (s["N"] > 0 and (s["rnull"] or s["inull"])):
            return INVALID
        named.add(s["member"])
        if s["N"] > max_beams or s["N"] > MAX_BEAMS:
            return CAPACITY
    return OK


def validate3(clouds, B, max_points):
    named = set()
    for c in clouds:
        if not 0 <= c["member"] < B or c["member"] in named or c["N"] < 0 or (c["N"] > 0 and c["null"]):
            return INVALID
        named.add(c["member"])
        if c["N"] > max_points:
            return CAPACITY
    return OK


def malformed(s):
    """rdet.h: range_min < 0, range_max <= range_min, angle_increment < 0 with angle_max <= angle_min."""
    return bool(s["rmin"] < 0 or s["rmax"] <= s["rmin"] or (s["inc"] < 0 and s["amax"] <= s["amin"]))


class Cache:
    """The cached beam-angle tables: one per lidar (N and the BITS of angle_min and angle_increment), least recently used replaced."""
    def __init__(self):
        self.tab = [dict(key=(-1, 0, 0), used=0) for _ in range(TABLES)]
        self.n = 0

    def plan(self, scans):
        self.n += 1
        key = lambda s: (s["N"], bits(s["amin"]), bits(s["inc"]))
        runs = [s["N"] != 0 and not malformed(s) for s in scans]
        find = lambda k: next((t for t in range(TABLES) if self.tab[t]["key"] == k), None)
        for s, r in zip(scans, runs):                         # what this call needs and already has is not replaced by it
            if r and find(key(s)) is not None:
                self.tab[find(key(s))]["used"] = self.n
        out = []
        for s, r in zip(scans, runs):
            if not r:
                out.append((0, 0, 0))
                continue
            t = find(key(s))
            if t is not None:
                self.tab[t]["used"] = self.n
                out.append((t, 0, 1))
                continue
            lru = min(range(TABLES), key=lambda t: (self.tab[t]["used"], t))
            if self.tab[lru]["used"] == self.n:               # every cached table is this call's: the member's own slot, not kept
                out.append((TABLES + s["member"], 1, 0))
            else:
                self.tab[lru] = dict(key=key(s), used=self.n)
                out.append((lru, 1, 1))
        return out

    def state(self):
        return [(t["key"][0], t["key"][1], t["key"][2], t["used"]) for t in self.tab]


def pack2(members, scans):
    """Steps 2 and 3 of an accepted rdet2d_batch_submit on a fresh cache -> (n_run, per scan (member, stamp, status, runs, table plan,
    record bytes), per member (last_n_returns, the odometry times left))."""
    members = [dict(m, odom=list(m["odom"])) for m in members]
    use = Cache().plan(scans)
    rows = []
    for s, u in zip(scans, use):
        M = members[s["member"]]
        r = np.zeros((), REC2)
        r["member"] = s["member"]
        status, runs = OK, 0
        if malformed(s):
            status = BAD_SCAN                                  # (the member keeps its odometry and its range data)
        elif s["N"] == 0:
            M["last_n_returns"] = 0
        else:
            runs = 1
            r["run"], r["N"], r["table"] = 1, s["N"], u[0]
            r["intensity_min"], r["min_length"], r["length_error"] = M["opt"][:3]
            r["opt_range_min"], r["opt_range_max"] = np.float32(M["opt"][3]), np.float32(M["opt"][4])
            r["msg_range_min"], r["msg_range_max"], r["angle_increment"] = s["rmin"], s["rmax"], s["inc"]
            with np.errstate(all="ignore"):
                r["point_delta_t"] = np.float64(s["scan_time"] / np.float32(s["N"]))      # float / float, then widened
                first = np.float64(s["stamp"]) - np.float64(s["scan_time"])
                r["is_circle"] = 1 if (np.float64(s["amax"] - s["amin"]) - 2 * math.pi) < 1e-6 else 0   # float - float, then double
            r["first_point_time"] = first
            a = np.float32(M["s2b"][2])
            r["s2b_x"], r["s2b_y"], r["s2b_a"], r["s2b_c"], r["s2b_s"] = np.float32(M["s2b"][0]), np.float32(M["s2b"][1]), a, cosf(a), sinf(a)
            while len(M["odom"]) > 1 and M["odom"][0][0] < first:                         # TrimDataByTime: at least one sample stays
                M["odom"].pop(0)
            r["n_odom"] = min(len(M["odom"]), 2)
            if M["odom"]:
                r["front"], r["back"] = np.array(tuple(M["odom"][0]), ODOM), np.array(tuple(M["odom"][-1]), ODOM)
        rows.append((s["member"], s["stamp"], status, runs, u, r.tobytes()))
    return sum(r[3] for r in rows), rows, [(M["last_n_returns"], [o[0] for o in M["odom"]]) for M in members]


def pack3(members, clouds):
    """An accepted rdet3d_batch_submit: records compacted over the clouds with points, slot = the cloud's index; the launch's LDS holds
    the largest N rounded up to whole 64-node tiles, at most 5120."""
    recs = []
    for i, c in enumerate(clouds):
        if c["N"] == 0:
            continue
        M = members[c["member"]]
        r = np.zeros((), REC3)
        r["intensity_min"], r["stamp"], r["member"], r["N"], r["slot"] = M["intensity_min"], c["stamp"], c["member"], c["N"], i
        a = np.float32(M["s2b"][2])
        r["sx"], r["sy"], r["cs"], r["sn"] = np.float32(M["s2b"][0]), np.float32(M["s2b"][1]), cosf(a), sinf(a)
        recs.append(r.tobytes())
    n_max = max([c["N"] for c in clouds] + [0])
    cap = min(-(-n_max // CLOUD_TILE) * CLOUD_TILE, MAX_BRIGHT)
    return len(recs), cap, [(c["member"], c["stamp"], int(c["N"] > 0)) for c in clouds], recs


def range_plan(B, max_beams, lst, last_n):
    """get_range_data_all's plan: the listed members' rows one behind the other; a record's pairs lie on the DESTINATION's 16-byte grid,
    so a record behind an odd offset has one slot in front and costs ceil((n + lead) / 512) workgroups, an empty member none."""
    order = list(range(B)) if lst is None else lst
    counts = [min(max(last_n[m], 0), max_beams) for m in order]
    recs, wgs, at = [], [], 0
    for m, n in zip(order, counts):
        if n == 0:
            continue
        wgs += [(len(recs), t) for t in range(-(-(n + (at & 1)) // RANGE_TILE))]
        recs.append(np.array((m * max_beams, at, n, 0), RANGE).tobytes())
        at += n
    return sum(counts), -(-(max_beams + 1) // RANGE_TILE), -(-24 * B // 256) * 256, counts, recs, wgs


def collect_rule(entries, max_centers):
    """rdet.h: the host's status stands; an entry without a workgroup has K = 0; a record's err is the status, K = 0; more centres than
    max_centers (capped at RDET_MAX_CENTERS) is RDET_ERR_BUFFER, K = 0."""
    cap = min(max_centers, MAX_CENTERS)
    out = []
    for i, (host_status, runs, K, err) in enumerate(entries):
        if not runs:
            out.append((host_status, 0, 0, []))
        elif err:
            out.append((err, 0, 1, []))
        elif K > cap:
            out.append((BUFFER, 0, 1, []))
        else:
            out.append((host_status, K, 1, [v for k in range(K) for v in (float(1000 * i + k), -float(1000 * i + k))]))
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
MB = 5
MEMBERS = {"all": (MB, None), "all_but_one": (MB - 1, None), "one_too_many": (MB + 1, None), "none_listed": (0, []), "some": (3, [2, 0, 3]),
           "all_backwards": (MB, [4, 3, 2, 1, 0]), "first_negative": (3, [-1, 0, 1]), "first_is_B": (3, [MB, 0, 1]), "middle_twice": (4, [0, 2, 0, 3]),
           "middle_negative": (4, [1, 0, -3, 2]), "last_is_B": (4, [0, 1, 2, MB]), "last_twice": (MB, [4, 3, 2, 1, 4]),
           "more_than_B": (MB + 1, [0, 1, 2, 3, 4, 0]), "more_than_B_outside": (MB + 1, [0, 1, 2, 3, 4, 5])}

VB, VMAX = 4, 16
VALIDATE2 = {
    "accepted_permuted": ([scan(3), scan(0, N=16), scan(2, N=0), scan(1, N=1)], VMAX, OK),
    "nothing": ([], VMAX, OK),
    "null_buffers_without_beams": ([scan(1, N=0, rnull=True, inull=True), scan(0)], VMAX, OK),
    "too_long_then_bad_member": ([scan(0, N=17), scan(9)], VMAX, CAPACITY),
    "bad_member_then_too_long": ([scan(9), scan(0, N=17)], VMAX, INVALID),
    "too_long_then_twice": ([scan(1), scan(0, N=17), scan(1)], VMAX, CAPACITY),
    "twice_then_too_long": ([scan(1), scan(1), scan(0, N=17)], VMAX, INVALID),
    "too_long_and_null": ([scan(0, N=17, rnull=True)], VMAX, INVALID),
    "N_negative": ([scan(0), scan(1, N=-1)], VMAX, INVALID),
    "null_ranges": ([scan(0), scan(1, rnull=True)], VMAX, INVALID),
    "null_intensities": ([scan(0, inull=True)], VMAX, INVALID),
    "first_negative": ([scan(-1), scan(0), scan(1)], VMAX, INVALID),
    "middle_twice": ([scan(0), scan(1), scan(1), scan(2)], VMAX, INVALID),
    "last_is_B": ([scan(0), scan(1), scan(2), scan(VB)], VMAX, INVALID),
    "more_than_B": ([scan(0), scan(1), scan(2), scan(3), scan(0)], VMAX, INVALID),
    "8192_beams": ([scan(0, N=8192)], 9000, OK),
    "8193_beams": ([scan(0, N=8193)], 9000, CAPACITY),
}
cloud = lambda member, N=8, stamp=50.0, null=False: dict(member=member, N=N, stamp=float(stamp), null=null)
VALIDATE3 = {
    "accepted_permuted": ([cloud(2), cloud(0, N=16), cloud(3, N=0, null=True)], VMAX, OK),
    "too_long_then_bad_member": ([cloud(0, N=17), cloud(-2)], VMAX, CAPACITY),
    "bad_member_then_too_long": ([cloud(VB), cloud(0, N=17)], VMAX, INVALID),
    "N_negative": ([cloud(0, N=-1)], VMAX, INVALID),
    "null_cloud": ([cloud(0), cloud(1, null=True)], VMAX, INVALID),
    "middle_twice": ([cloud(0), cloud(2), cloud(2), cloud(1)], VMAX, INVALID),
    "last_twice": ([cloud(0), cloud(1), cloud(0)], VMAX, INVALID),
}

lidar = lambda k, member, **kw: scan(member, **{"N": 4 + k, **kw})     # lidar k: its own beam count
NAN_A, NAN_B = from_bits(0x7FC00001), from_bits(0x7FC00002)
TABLE_SEQUENCES = {
    # 8 lidars fill the cache; a hit; a 9th evicts the least recently used (table 0: lidar 3's was used since); the evicted lidar comes
    # back as a miss; a call that needs a cached lidar LATER than its miss keeps that lidar's table
    "fill_hit_evict": [[lidar(k, k) for k in range(8)], [lidar(3, 0)], [lidar(8, 5)], [lidar(0, 2)], [lidar(9, 0), lidar(2, 1)]],
    # 9 lidars in one call: the last one goes to its member's own slot, and is a miss again in the next call
    "nine_in_one_call": [[lidar(k, 8 - k) for k in range(9)], [lidar(8, 3)]],
    # the cache full of this call's tables and the missing lidar FIRST in the call
    "nine_the_missing_one_first": [[lidar(k, k) for k in range(8)], [lidar(8, 8)] + [lidar(k, k) for k in range(8)] + [lidar(8, 9)]],
    "zero_signs_and_nans": [[scan(0, amin=0.0), scan(1, amin=-0.0), scan(2, amin=0.0)], [scan(0, inc=NAN_A), scan(1, inc=NAN_A), scan(2, inc=NAN_B)]],
    "no_table_for_nothing": [[lidar(0, 0)], [lidar(1, 0, rmin=-1.0), lidar(2, 1, N=0), lidar(3, 2, rmax=0.05), lidar(4, 3, inc=-0.1, amin=1.0, amax=1.0)],
                             [lidar(0, 1)]],
}

od = lambda t: (t, 1.0 + t, -2.0 - t, 0.25 * t, 0.5, -0.125, 0.03125)
member2 = lambda k, odom=(), last=7: dict(opt=(30.0 + k, 0.2 + 0.01 * k, 0.05, 0.5 + k, 25.0 - k), s2b=(0.1 * k, -0.2 * k, 0.3 * k - 1.0), odom=[od(t) for t in odom],
                                          last_n_returns=last + k)
TWO_PI32 = np.float32(2 * math.pi)
UNDER, OVER = np.nextafter(TWO_PI32, np.float32(9)), np.nextafter(np.nextafter(TWO_PI32, np.float32(9)), np.float32(9))
SUBMIT2 = {
    # stamp 100, scan_time 0.1f: first_point_time is just under 99.9
    "trim": ([member2(0), member2(1, [99.0]), member2(2, [99.0, 99.95]), member2(3, [99.95, 100.0]), member2(4, [99.0, 99.5, 99.8, 99.95, 100.0]),
              member2(5, [90.0, 91.0, 92.0, 93.0, 94.0]), member2(6, [99.95, 99.96, 99.97, 99.98, 99.99]), member2(7, [99.0, 99.5])],
             [scan(k, N=3 + k) for k in (4, 0, 7, 1, 6, 2, 5, 3)]),
    "delta_t_and_circle": ([member2(k) for k in range(4)], [scan(0, N=3), scan(1, N=7, amin=0.0, amax=UNDER), scan(2, N=8, amin=0.0, amax=OVER),
                                                            scan(3, N=5, amin=0.0, amax=NAN_A, scan_time=0.025)]),
    "malformed_and_empty": ([member2(k, [99.0, 99.5, 99.95]) for k in range(5)],
                            [scan(0, rmin=-0.5), scan(1, N=0), scan(2, rmax=0.1), scan(3, inc=-0.01, amin=1.0, amax=0.5), scan(4, inc=-0.01, amin=-1.0, amax=0.5)]),
    "one_lidar_for_all": ([member2(k, [99.95]) for k in range(12)], [scan(k, N=6, stamp=100.0 + k) for k in range(12)]),
}

member3 = lambda k: dict(intensity_min=100.0 + k, s2b=(0.5 * k, 1.0 - k, 0.7 * k - 2.0))
SUBMIT3 = {
    "compacted": (16, [cloud(3, N=5, stamp=7.5), cloud(0, N=0), cloud(1, N=16, stamp=8.5), cloud(2, N=0, null=True), cloud(4, N=1)], 64),
    "cap_64": (100, [cloud(0, N=64), cloud(1, N=63)], 64),
    "cap_65": (100, [cloud(1, N=0), cloud(0, N=65)], 128),
    "cap_5120": (6000, [cloud(2, N=5120), cloud(0, N=5057)], 5120),
    "cap_5121": (6000, [cloud(2, N=5121), cloud(1, N=2)], 5120),
    "nothing_runs": (16, [cloud(0, N=0), cloud(4, N=0)], 0),
    "no_cloud": (16, [], 0),
}

EDGE = (0, 1, 511, 512, 513, 1023, 1024, 1025)
RANGE_CASES = {"%s_offset_%d" % (("even", "odd")[p], n): (2, 1100, None, [2 - p, n]) for p in (0, 1) for n in EDGE}
RANGE_CASES.update({
    "zero_between": (3, 1100, None, [513, 0, 5]),
    "all_edges_in_one_call": (8, 1100, None, list(EDGE)),
    "permuted_list": (6, 600, [4, 0, 5, 2], [3, 77, 512, 0, 513, 600]),
    "clamped": (4, 600, None, [601, -1, 9000, 600]),
    "nothing_to_copy": (3, 600, [2, 0], [0, 5, 0]),
    "empty_list": (3, 600, [], [1, 2, 3]),
    "twelve_members": (12, 700, [11, 3, 7, 0], [1 + 59 * k for k in range(12)]),
})
RANGE_REFUSED = {"twice": (3, 600, [1, 1], [1, 2, 3]), "outside": (3, 600, [0, 3], [1, 2, 3])}

#            host status, runs, K, err
COLLECT = {"each_branch": ([(OK, 1, 3, 0), (BAD_SCAN, 0, 5, 0), (OK, 0, 2, 0), (OK, 1, 9, CAPACITY), (OK, 1, 5, 0), (OK, 1, 4, 0), (OK, 1, 0, 0)], 4),
           "no_room": ([(OK, 1, 0, 0), (OK, 1, 1, 0), (OK, 0, 1, 0)], 0),
           "all_256": ([(OK, 1, 256, 0), (OK, 1, 255, 0)], MAX_CENTERS),
           "above_256": ([(OK, 1, 256, 0), (OK, 1, 257, 0), (OK, 1, 300, 0), (OK, 1, 301, 0)], 300),
           "nothing": ([], 8)}
#               count, status, K, centers, max_centers
COLLECT_ARGS = [((2, 1, 1, 1, 4), 1), ((2, 1, 1, 0, 0), 1), ((0, 0, 0, 0, 0), 1), ((0, 0, 0, 0, 7), 1), ((2, 1, 1, 0, 1), 0), ((2, 0, 1, 1, 4), 0),
                ((2, 1, 0, 1, 4), 0), ((2, 1, 1, 1, -1), 0), ((0, 1, 1, 1, -1), 0)]
LINK = [(7, 11.5, OK, 1), (2, 12.5, BAD_SCAN, 0), (0, 13.5, OK, 0), (5, 14.5, OK, 1)]


# ---- the program's answers -------------------------------------------------------------------------------------------------------
def member2_lines(m):
    o = m["opt"]
    head = "%s %s %s %08x %08x %s %d %d" % (h(o[0]), h(o[1]), h(o[2]), bits(o[3]), bits(o[4]), " ".join(h(v) for v in m["s2b"]), m["last_n_returns"], len(m["odom"]))
    return [head] + [" ".join(h(v) for v in s) for s in m["odom"]]


def records():
    """-> [(key, the record's text, its parser)] in the order they are written."""
    out = []
    ints = lambda line: [int(v) for v in line.split()[1:]]
    for name, (count, lst) in MEMBERS.items():
        out.append((("members", name), "members %d %d %d %s" % (MB, count, lst is not None, " ".join(map(str, lst or []))), lambda L: tuple(ints(L.pop(0)))))
    for name, (scans, max_beams, _) in VALIDATE2.items():
        out.append((("validate2", name), "\n".join(["validate2 %d %d %d" % (VB, max_beams, len(scans))] + [scan_line(s) for s in scans]), lambda L: tuple(ints(L.pop(0)))))
    for name, (clouds, max_points, _) in VALIDATE3.items():
        text = ["validate3 %d %d %d" % (VB, max_points, len(clouds))] + ["%d %d %d" % (c["member"], c["N"], c["null"]) for c in clouds]
        out.append((("validate3", name), "\n".join(text), lambda L: tuple(ints(L.pop(0)))))
    for name, calls in TABLE_SEQUENCES.items():
        def parse(L, calls=calls):
            got = []
            for scans in calls:
                n = ints(L.pop(0))[0]
                use = [tuple(int(v) for v in L.pop(0).split()) for _ in scans]
                state = [L.pop(0).split() for _ in range(TABLES)]
                got.append((n, use, [(int(t[0]), int(t[1], 16), int(t[2], 16), int(t[3])) for t in state]))
            return got
        text = ["tables %d" % len(calls)]
        for scans in calls:
            text += ["%d" % len(scans)] + [scan_line(s) for s in scans]
        out.append((("tables", name), "\n".join(text), parse))
    for name, (members, scans) in SUBMIT2.items():
        def parse(L, members=members, scans=scans):
            rc = ints(L.pop(0))[0]
            if rc != OK:
                return rc, None
            n_run, rows = ints(L.pop(0))[0], []
            for _ in scans:
                t = L.pop(0).split()
                rows.append((int(t[0]), float.fromhex(t[1]), int(t[2]), int(t[3]), (int(t[4]), int(t[5]), int(t[6])), bytes.fromhex(t[7])))
            left = []
            for _ in members:
                t = L.pop(0).split()
                left.append((int(t[0]), [float.fromhex(v) for v in t[2:]]))
                assert int(t[1]) == len(t) - 2
            return rc, (n_run, rows, left)
        text = ["submit2 %d %d" % (len(members), len(scans))]
        for m in members:
            text += member2_lines(m)
        out.append((("submit2", name), "\n".join(text + [scan_line(s) for s in scans]), parse))
    for name, (max_points, clouds, _) in SUBMIT3.items():
        def parse(L, clouds=clouds):
            rc = ints(L.pop(0))[0]
            n_run, cap = (int(v) for v in L.pop(0).split())
            subs = []
            for _ in clouds:
                t = L.pop(0).split()
                subs.append((int(t[0]), float.fromhex(t[1]), int(t[2])))
            return rc, n_run, cap, subs, [bytes.fromhex(L.pop(0)) for _ in range(n_run)]
        text = ["submit3 %d %d %d" % (5, max_points, len(clouds))] + ["%s %s" % (h(member3(k)["intensity_min"]), " ".join(h(v) for v in member3(k)["s2b"])) for k in range(5)]
        out.append((("submit3", name), "\n".join(text + ["%d %s %d %d" % (c["member"], h(c["stamp"]), c["N"], c["null"]) for c in clouds]), parse))
    for name, (B, max_beams, lst, last_n) in {**RANGE_CASES, **RANGE_REFUSED}.items():
        def parse(L):
            if not ints(L.pop(0))[0]:
                return None
            total, tiles, off = (int(v) for v in L.pop(0).split())
            counts, recs, wgs = ints(L.pop(0)), L.pop(0).split()[1:], L.pop(0).split()[1:]
            assert int(recs[0]) == len(recs) - 1 and int(wgs[0]) == len(wgs) - 1
            return total, tiles, off, counts, [bytes.fromhex(r) for r in recs[1:]], [tuple(int(v) for v in w.split(":")) for w in wgs[1:]]
        text = "range %d %d %d %d %s\n%s" % (B, max_beams, B if lst is None else len(lst), lst is not None, " ".join(map(str, lst or [])), " ".join(map(str, last_n)))
        out.append((("range", name), text, parse))
    for name, (entries, max_centers) in COLLECT.items():
        def parse(L, entries=entries):
            rows = []
            for _ in entries:
                t = L.pop(0).split()
                rows.append((int(t[0]), int(t[1]), int(t[2]), [float.fromhex(v) for v in t[3:]]))
            return rows, ints(L.pop(0))[0]
        out.append((("collect", name), "\n".join(["collect %d %d" % (len(entries), max_centers)] + ["%d %d %d %d" % e for e in entries]), parse))
    for args, _ in COLLECT_ARGS:
        out.append((("collect_args", args), "collect_args %d %d %d %d %d" % args, lambda L: ints(L.pop(0))[0]))
    out.append((("link", 0), "\n".join(["link 3 %d" % len(LINK)] + ["%d %s %d %d" % (m, h(t), st, r) for m, t, st, r in LINK]), lambda L: L.pop(0).split()[1:]))
    for name, (a0, inc, N, stride) in ANGLES.items():
        out.append((("angles", name), "angles %08x %08x %d %d" % (bits(a0), bits(inc), N, stride), lambda L: [int(v, 16) for v in L.pop(0).split()[1:]]))
    return out


ANGLES = {"a_third_of_a_degree": (-PI32, np.float32(math.pi / 540), 8, 11), "backwards": (np.float32(2.0), np.float32(-0.3), 5, 5), "one_beam": (np.float32(0.1), NAN_A, 1, 4)}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """tests/cpp/det_batch_host.cpp, built host-only, run once over every record of this file: key -> the parsed answer."""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    tmp = tmp_path_factory.mktemp("det_batch_host")
    exe, path = str(tmp / "det_batch_host"), str(tmp / "cases.txt")
    r = subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "det_batch_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = records()
    with open(path, "w") as f:
        f.write("\n".join(text for _, text, _ in recs) + "\n")
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    out = {key: parse(lines) for key, _, parse in recs}
    assert not lines
    return out


@pytest.mark.parametrize("name", sorted(MEMBERS))
def test_members_named_once_and_a_clean_scratch(answers, name):
    count, lst = MEMBERS[name]
    ok, bad, zero, next_ok = answers[("members", name)]
    want_bad = -1 if lst is None else first_bad(lst, MB)
    assert bad == want_bad
    assert ok == int(count == MB if lst is None else (count <= MB and want_bad == len(lst)))
    assert zero == 1 and next_ok == 1                          # whatever the call was, and wherever it was refused
    assert len(lst or []) <= 12


def test_the_member_lists_are_the_ones_they_claim_to_be():
    bad = {n: first_bad(l, MB) for n, (c, l) in MEMBERS.items() if l is not None}
    assert bad["first_negative"] == bad["first_is_B"] == 0 and bad["middle_twice"] == bad["middle_negative"] == 2
    assert bad["last_is_B"] == 3 and bad["last_twice"] == 4 and bad["more_than_B"] == bad["more_than_B_outside"] == MB     # the last entry each
    assert all(bad[n] == len(MEMBERS[n][1]) for n in ("none_listed", "some", "all_backwards"))


@pytest.mark.parametrize("name", sorted(VALIDATE2))
def test_2d_submit_refusals_and_their_order(answers, name):
    scans, max_beams, code = VALIDATE2[name]
    assert validate2(scans, VB, max_beams) == code
    assert answers[("validate2", name)] == (code, 1, OK)      # the code; the scratch all zero; the next call accepted


@pytest.mark.parametrize("name", sorted(VALIDATE3))
def test_3d_submit_refusals_and_their_order(answers, name):
    clouds, max_points, code = VALIDATE3[name]
    assert validate3(clouds, VB, max_points) == code
    assert answers[("validate3", name)] == (code, 1, OK)


@pytest.mark.parametrize("name", sorted(TABLE_SEQUENCES))
def test_the_table_cache_through_a_sequence_of_calls(answers, name):
    cache = Cache()
    for scans, (n, use, state) in zip(TABLE_SEQUENCES[name], answers[("tables", name)]):
        assert len(scans) <= 12 and validate2(scans, 12, MAX_BEAMS) == OK
        want = cache.plan(scans)
        assert n == cache.n and use == want and state == cache.state()


def test_the_table_sequences_are_the_ones_they_claim_to_be(answers):
    use = lambda name, call: answers[("tables", name)][call][1]
    keys = lambda name, call: [t[0] for t in answers[("tables", name)][call][2]]
    assert use("fill_hit_evict", 0) == [(k, 1, 1) for k in range(8)] and use("fill_hit_evict", 1) == [(3, 0, 1)]
    assert use("fill_hit_evict", 2) == [(0, 1, 1)] and keys("fill_hit_evict", 2) == [12, 5, 6, 7, 8, 9, 10, 11]       # lidar 0's table went
    assert use("fill_hit_evict", 3) == [(1, 1, 1)]                                                                      # ... and lidar 0 is a miss
    assert use("fill_hit_evict", 4) == [(4, 1, 1), (2, 0, 1)] and keys("fill_hit_evict", 4)[2] == 6                      # table 2 was the oldest and stays
    assert use("nine_in_one_call", 0) == [(k, 1, 1) for k in range(8)] + [(TABLES + 0, 1, 0)] and 12 not in keys("nine_in_one_call", 0)
    assert use("nine_in_one_call", 1) == [(0, 1, 1)]
    assert use("nine_the_missing_one_first", 1)[0] == (TABLES + 8, 1, 0) and use("nine_the_missing_one_first", 1)[-1] == (TABLES + 9, 1, 0)
    assert use("nine_the_missing_one_first", 1)[1:-1] == [(k, 0, 1) for k in range(8)]
    assert use("zero_signs_and_nans", 0) == [(0, 1, 1), (1, 1, 1), (0, 0, 1)] and use("zero_signs_and_nans", 1) == [(2, 1, 1), (2, 0, 1), (3, 1, 1)]
    before, after = answers[("tables", "no_table_for_nothing")][0][2], answers[("tables", "no_table_for_nothing")][1][2]
    assert use("no_table_for_nothing", 1) == [(0, 0, 0)] * 4 and before == after and use("no_table_for_nothing", 2) == [(0, 0, 1)]
    assert [malformed(s) for s in TABLE_SEQUENCES["no_table_for_nothing"][1]] == [True, False, True, True] and TABLE_SEQUENCES["no_table_for_nothing"][1][1]["N"] == 0


@pytest.mark.parametrize("name", sorted(ANGLES))
def test_a_beam_angle_table(answers, name):
    a0, inc, N, stride = ANGLES[name]
    angle, want = np.float32(a0), []
    with np.errstate(all="ignore"):
        for _ in range(N):                                     # the float32 accumulation, not angle_min + k * increment
            want.append(angle)
            angle = np.float32(angle + inc)
    assert answers[("angles", name)] == [bits(v) for v in want] + [bits(cosf(v)) for v in want] + [bits(sinf(v)) for v in want]


@pytest.mark.parametrize("name", sorted(SUBMIT2))
def test_an_accepted_2d_submit_packs_the_documented_records(answers, name):
    members, scans = SUBMIT2[name]
    assert len(members) <= 12 and max(s["N"] for s in scans) <= 16 and validate2(scans, len(members), MAX_BEAMS) == OK
    rc, got = answers[("submit2", name)]
    n_run, rows, left = pack2(members, scans)
    assert rc == OK and got[0] == n_run
    for g, w in zip(got[1], rows):
        assert g[:5] == w[:5] and g[5] == w[5], (g[:5], w[:5], np.frombuffer(g[5], REC2), np.frombuffer(w[5], REC2))
    assert got[2] == left


def test_the_2d_submits_are_the_ones_they_claim_to_be(answers):
    rec = lambda name, i: np.frombuffer(answers[("submit2", name)][1][1][i][5], REC2)[0]
    left = lambda name: answers[("submit2", name)][1][2]
    first = 100.0 - float(np.float32(0.1))
    # the trim: scans were given for members 4, 0, 7, 1, 6, 2, 5, 3
    assert [rec("trim", i)["member"] for i in range(8)] == [4, 0, 7, 1, 6, 2, 5, 3]
    assert [rec("trim", i)["n_odom"] for i in range(8)] == [2, 0, 1, 1, 2, 1, 1, 2]
    assert [len(t) for _, t in left("trim")] == [0, 1, 1, 2, 2, 1, 5, 1]
    assert left("trim")[1][1] == [99.0] and left("trim")[5][1] == [94.0] and left("trim")[5][1][0] < first             # all older: one is kept
    assert left("trim")[4][1] == [99.95, 100.0] and left("trim")[7][1] == [99.5] and left("trim")[2][1] == [99.95]
    r = rec("trim", 4)                                                                                                  # member 6: nothing is older
    assert (r["front"]["time"], r["back"]["time"]) == (99.95, 99.99) and r["front"]["px"] == 1.0 + 99.95 and r["back"]["wz"] == 0.03125
    assert rec("trim", 1)["front"]["time"] == 0.0 and rec("trim", 2)["front"].tobytes() == rec("trim", 2)["back"].tobytes()
    # point_delta_t: the quotient is taken in float32
    r = rec("delta_t_and_circle", 0)
    assert r["point_delta_t"] == float(np.float32(0.1) / np.float32(3)) != float(np.float32(0.1)) / 3 and r["first_point_time"] == first
    assert float(UNDER) - 2 * math.pi < 1e-6 < float(OVER) - 2 * math.pi and bits(OVER) - bits(UNDER) == 1
    assert [rec("delta_t_and_circle", i)["is_circle"] for i in range(4)] == [1, 1, 0, 0]
    # a malformed scan trims nothing and leaves last_n_returns; N == 0 zeroes it and trims nothing either
    rows = answers[("submit2", "malformed_and_empty")][1][1]
    assert [(r[2], r[3]) for r in rows] == [(BAD_SCAN, 0), (OK, 0), (BAD_SCAN, 0), (BAD_SCAN, 0), (OK, 1)]
    assert [n for n, _ in left("malformed_and_empty")] == [7, 0, 9, 10, 11] and [len(t) for _, t in left("malformed_and_empty")] == [3, 3, 3, 3, 1]
    assert all(rows[i][5] == np.array((0,) * 5 + ((0,) * 7,) * 2 + (0,) * 8 + (i,) + (0,) * 7, REC2).tobytes() for i in range(4))
    assert answers[("submit2", "one_lidar_for_all")][1][0] == 12 and [r[4] for r in answers[("submit2", "one_lidar_for_all")][1][1]] == [(0, 1, 1)] + [(0, 0, 1)] * 11


@pytest.mark.parametrize("name", sorted(SUBMIT3))
def test_an_accepted_3d_submit_packs_the_documented_records(answers, name):
    max_points, clouds, cap = SUBMIT3[name]
    assert validate3(clouds, 5, max_points) == OK and len(clouds) <= 12
    want = pack3([member3(k) for k in range(5)], clouds)
    assert want[1] == cap
    assert answers[("submit3", name)] == (OK,) + want


def test_the_3d_submits_are_the_ones_they_claim_to_be(answers):
    recs = np.frombuffer(b"".join(answers[("submit3", "compacted")][4]), REC3)
    assert recs["slot"].tolist() == [0, 2, 4] and recs["member"].tolist() == [3, 1, 4] and recs["N"].tolist() == [5, 16, 1] and recs["stamp"].tolist() == [7.5, 8.5, 50.0]
    assert [s[2] for s in answers[("submit3", "compacted")][3]] == [1, 0, 1, 0, 1]
    assert answers[("submit3", "nothing_runs")][1:3] == (0, 0)


@pytest.mark.parametrize("name", sorted(RANGE_CASES))
def test_the_range_data_plan(answers, name):
    B, max_beams, lst, last_n = RANGE_CASES[name]
    assert B <= 12 and first_bad(lst or [], B) == len(lst or [])
    total, tiles, off, counts, recs, wgs = want = range_plan(B, max_beams, lst, last_n)
    assert answers[("range", name)] == want
    assert len(wgs) <= tiles * B and 24 * B <= off and off % 256 == 0        # the plan fits what the handle allocates for it
    rows = np.frombuffer(b"".join(recs), RANGE)
    assert rows["n"].sum() == total == sum(counts) and (rows["n"] > 0).all()
    assert rows["dst_off"].tolist() == np.cumsum(np.concatenate([[0], rows["n"]]))[:-1].tolist()
    for r, row in enumerate(rows):                            # every slot of every record is some workgroup's, once
        t = sorted(tile for rec, tile in wgs if rec == r)
        lead = int(row["dst_off"]) & 1
        assert t == list(range(len(t))) and (len(t) - 1) * RANGE_TILE < row["n"] + lead <= len(t) * RANGE_TILE


def test_the_range_cases_are_the_ones_they_claim_to_be(answers):
    wg = lambda name: len(answers[("range", name)][5])
    assert [wg("even_offset_%d" % n) - 1 for n in EDGE] == [0, 1, 1, 1, 2, 2, 2, 3]       # (one workgroup is the member's in front)
    assert [wg("odd_offset_%d" % n) - 1 for n in EDGE] == [0, 1, 1, 2, 2, 2, 3, 3]        # the slot in front costs 512 and 1024 one more
    assert answers[("range", "zero_between")][5] == [(0, 0), (0, 1), (1, 0)] and answers[("range", "zero_between")][3] == [513, 0, 5]
    assert np.frombuffer(b"".join(answers[("range", "zero_between")][4]), RANGE)["src_off"].tolist() == [0, 2200]
    assert answers[("range", "clamped")][3] == [600, 0, 600, 600] and answers[("range", "permuted_list")][3] == [513, 3, 600, 512]
    assert answers[("range", "nothing_to_copy")][0] == 0 and answers[("range", "nothing_to_copy")][5] == [] and answers[("range", "empty_list")][3] == []
    assert all(answers[("range", name)] is None for name in RANGE_REFUSED)


@pytest.mark.parametrize("name", sorted(COLLECT))
def test_the_collect_rule(answers, name):
    entries, max_centers = COLLECT[name]
    rows, untouched = answers[("collect", name)]
    assert rows == collect_rule(entries, max_centers) and untouched == 1


def test_collect_cases_and_arguments(answers):
    status = lambda name: [r[:2] for r in answers[("collect", name)][0]]
    assert status("each_branch") == [(OK, 3), (BAD_SCAN, 0), (OK, 0), (CAPACITY, 0), (BUFFER, 0), (OK, 4), (OK, 0)]
    assert status("no_room") == [(OK, 0), (BUFFER, 0), (OK, 0)] and status("all_256") == [(OK, 256), (OK, 255)]
    assert status("above_256") == [(OK, 256), (BUFFER, 0), (BUFFER, 0), (BUFFER, 0)]        # 300 asked for: 256 it is
    assert [answers[("collect_args", args)] for args, _ in COLLECT_ARGS] == [want for _, want in COLLECT_ARGS]


def test_fill_link(answers):
    t = answers[("link", 0)]
    i = t.index("records")
    #                  count device  the four host arrays   stride  K  err centres pairs  records/ready consumed
    assert t[:i] == ["4", "3", "1", "1", "1", "1", "2064", "0", "8", "16", str(MAX_CENTERS), "1", "1"]
    assert [int(v) for v in t[i + 1:]] == [0, -1, -1, 3, 77, 77]                            # record = i for an entry that runs, else -1
