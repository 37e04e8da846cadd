"""Cases of the fleet range-data tests (tests/test_fleet_range_data_gpu.py runs them on the GPU, tests/test_fleet_range_data_cpu.py
holds them to their stated conditions under the oracle alone), in the ``(members, ticks)`` form of tests/fleet_detect_cases.py.

A scan's number of valid beams -- the rows GetRangeData has after it -- is made exactly k by putting the other beams outside the
message's [range_min, range_max], half of them below and half above."""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from tests.detect_cases import S2B, odom_stream
from tests.fleet_detect_cases import member

TILE = 512            # RDET2DB_RANGE_TILE of csrc/det2d_batch.hip: the rows (16 bytes a lane, 256 lanes) of one workgroup
MAX_BEAMS = 8192

# rows per member of the edge handle, in member order: an odd count in front of the largest one (its rows start 8 bytes off a 16-byte
# boundary and take one workgroup more), both sides of 256 and of the tile, empty members between odd and even ones
EDGE_COUNTS = (1, 8192, 0, 255, 256, 257, 0, 511, 512, 513, 3, 1023, 1024, 1025, 2)
PERMUTED = (9, 1, 14, 0, 7, 2, 12, 5)      # a subset out of order: odd counts in front of 8192 (again), of 512 and of 1024; an empty member inside
MANY = 300


def scan_with_valid(k, n_beams, seed, stamp=5.0):
    """A LaserScan of ``n_beams`` beams of which exactly ``k`` lie inside the message's range limits."""
    assert 0 <= k <= n_beams
    rng = np.random.default_rng(seed)
    inc = np.float32(2.0 * math.pi / max(n_beams, 1))
    amin = np.float32(-math.pi)
    r = np.full(n_beams, 40.0, np.float32)                         # above range_max
    r[::2] = 0.01                                                  # below range_min
    idx = np.sort(rng.choice(n_beams, size=k, replace=False)) if k else np.zeros(0, np.int64)
    r[idx] = rng.uniform(1.0, 8.0, size=k).astype(np.float32)
    it = np.where(rng.random(n_beams) < 0.1, 200.0, 50.0).astype(np.float32)
    return NS(stamp=stamp, angle_min=float(amin), angle_max=float(amin + inc * max(n_beams - 1, 0)), angle_increment=float(inc),
              scan_time=0.1, range_min=0.05, range_max=30.0, ranges=r, intensities=it)


def beams_for(k):
    """The beams of the scan that leaves k rows: more than k (the compaction has something to skip) up to the handle's limit."""
    return min(MAX_BEAMS, k + 37 + k // 3)


def _s2b(m):
    return (S2B[0] + 0.01 * m, -0.02 * m, 0.1 * (m % 5))           # every member its own origin


def edge_case():
    """-> (members, ticks): one tick, member m's scan leaves EDGE_COUNTS[m] rows; odd members have odometry (their rows are de-skewed
    along a moving pose)."""
    members = [member(_s2b(m)) for m in range(len(EDGE_COUNTS))]
    scans = [(m, scan_with_valid(k, beams_for(k), 100 + m)) for m, k in enumerate(EDGE_COUNTS)]
    odom = {m: odom_stream(5.0 - 0.3, 5.0 + 0.05, v=0.6 + 0.05 * m, w=0.2) for m in range(1, len(EDGE_COUNTS), 2)}
    return members, [dict(odom=odom, scans=scans)]


HISTORY_COUNTS = (700, 301, 64, 5)


def history_case():
    """-> (members, ticks): four members, two ticks.  Tick 1: everybody.  Tick 2: member 0 sits out (keeps its 700 rows), member 1
    has a scan of no beams (0 rows), member 2 a malformed message (keeps its 64 rows), member 3 a new scan (9 rows)."""
    from tests.fleet_detect_cases import malformed
    members = [member(_s2b(m)) for m in range(4)]
    t1 = [(m, scan_with_valid(k, beams_for(k), 200 + m)) for m, k in enumerate(HISTORY_COUNTS)]
    empty = scan_with_valid(0, 0, 1, stamp=5.1)
    t2 = [(1, empty), (2, malformed(scan_with_valid(33, 90, 210, stamp=5.1), 1)), (3, scan_with_valid(9, 40, 211, stamp=5.1))]
    odom = {0: odom_stream(4.7, 5.05), 2: odom_stream(4.7, 5.05, v=0.4, w=-0.3)}
    return members, [dict(odom=odom, scans=t1), dict(odom={3: odom_stream(5.06, 5.15)}, scans=t2)]


HISTORY_AFTER = (700, 0, 64, 9)


def many_counts():
    """The rows of MANY members (max_beams 64): every count 0 .. 64 several times, odd and even mixed."""
    return [(7 * m + 3) % 65 for m in range(MANY)]


def many_case():
    members = [member(_s2b(m % 11)) for m in range(MANY)]
    scans = [(m, scan_with_valid(k, 64, 300 + m, stamp=5.0 + 0.001 * m)) for m, k in enumerate(many_counts())]
    return members, [dict(odom={}, scans=scans)]


def expected_rows(members, ticks):
    """-> per tick, per member: the rows GetRangeData has after the tick, by one OracleDetect2D per member that was fed the same
    odometry.  A member that is not in a tick keeps its rows, as does one whose message is malformed (the oracle refuses it); a scan
    of no beams leaves none (include/rdet.h)."""
    from oracle.binding import OracleDetect2D
    orc = [OracleDetect2D(sensor_to_base_link=m["s2b"], **m["opts"]) for m in members]
    rows = [np.zeros((0, 2), np.float32) for _ in members]
    out = []
    for tick in ticks:
        for m, stream in tick["odom"].items():
            for o in stream:
                orc[m].handle_odometry(*o)
        for m, sc in tick["scans"]:
            if sc.ranges.shape[0] == 0:
                rows[m] = np.zeros((0, 2), np.float32)
                continue
            try:
                orc[m].handle_scan(sc)
            except ValueError:
                continue
            rows[m] = orc[m].returns()
        out.append(list(rows))
    for o in orc:
        o.close()
    return out


def workgroups(counts):
    """The workgroups rdet2d_batch_get_range_data_all's one launch has for these counts, in order: a member with n rows behind
    ``at`` rows costs ceil((n + at % 2) / TILE), an empty one none."""
    at = total = 0
    for n in counts:
        if n:
            total += (n + (at & 1) + TILE - 1) // TILE
        at += n
    return total
