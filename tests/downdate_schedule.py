"""The tile schedule of the covariance downdate (dd_body, csrc/ekf_kernels.hip), restated in Python and shared by
tests/test_downdate_schedule_cpu.py (the bookkeeping), tests/ekf_range_cases.py (which state size gives which range form) and
tests/test_ekf_ranges_gpu.py (which workgroup held a tile).  The HIP code is the product; this mirrors its index arithmetic --
host: downdate_schedule / launch_downdate_any / rekf_launch_scan / rekf_scan_launch_fits, device: the classA / tri_IJ / cursor
logic -- and reads the constants the arithmetic uses from the source."""
import math
import os
import re

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reflector_ekf_slam_amd", "csrc", "ekf_kernels.hip")


def _defines(*names):
    with open(_SRC) as f:
        text = f.read()
    out = []
    for name in names:
        m = re.findall(r"^#define\s+%s\s+(\d+)\s*$" % name, text, re.M)
        assert len(m) == 1, (name, m)
        out.append(int(m[0]))
    return out


DT, DD_WG_PER_CU, FRONT_MB, REKF_SCAN_MIN_DD_WGS, MID_ROWS = _defines("DT", "DD_WG_PER_CU", "FRONT_MB", "REKF_SCAN_MIN_DD_WGS", "MID_ROWS")
AHEAD = 1                                   # REKF_DD_AHEAD's default: tile pos + 1 is loaded while tile pos is computed
DD_RUN = 3                                  # tiles per class-B item of the queue


def tiles_of(n):
    return (n + DT - 1) // DT


def host_plan(T, slots=256):
    """downdate_schedule (csrc/ekf_kernels.hip): (grid, lo, x, sub) -- class-B workgroups take lo tiles, the first x one more."""
    room = slots - T if slots - T > 1 else 1
    nB = (T - 1) * (T - 2) // 2
    sub = 2
    if (nB + room - 1) // room < 3:
        sub = 1
        nB = T * (T - 1) // 2
    lo, x = nB // room, nB % room
    grid = T + (room if lo > 0 else x)
    if grid >= 64:
        grid = (grid + 7) & ~7
    return grid, lo, x, sub


def kernel_plan(T, grid):
    """What k_downdate2 derives itself when the host only has a bound of n (dd_sub = 0)."""
    room = grid - T if grid - T > 1 else 1
    nB = (T - 1) * (T - 2) // 2
    sub = 2
    if (nB + room - 1) // room < 3:
        sub = 1
        nB = T * (T - 1) // 2
    return nB // room, nB % room, sub


def renumbered(grid, block):
    """The workgroup number w a block takes: an XCD's workgroups take consecutive ranges."""
    if grid >= 8 and grid % 8 == 0:
        return (block & 7) * (grid >> 3) + (block >> 3)
    return block


def seed_column(TT, t0):
    """The column the cursor starts at: the kernel's closed form, in float32 as it evaluates it (one sqrtf)."""
    f = np.float32
    bq = f(2.0) * f(TT) + f(1.0)
    arg = max(f(bq * bq - f(8.0) * f(t0)), f(0.0))
    Jg = int(f(f(bq - np.sqrt(f(arg))) * f(0.5)))
    return max(0, min(TT - 1, Jg))


def device_tiles(T, grid, lo, x, sub, block):
    """Tiles of workgroup `block`, in processing order."""
    w = block
    if grid >= 8 and grid % 8 == 0:
        w = (block & 7) * (grid >> 3) + (block >> 3)          # an XCD's workgroups take consecutive ranges
    if w < T:                                                  # class A
        tiles = []
        if sub == 2 and w + 1 < T:
            tiles.append((w + 1, w))
        tiles.append((w, w))
        return tiles
    TT = T - sub
    nB = (T - sub + 1) * (T - sub) // 2
    wq = w - T
    t0 = wq * lo + min(wq, x)
    t1 = t0 + lo + (1 if wq < x else 0)
    t0, t1 = min(t0, nB), min(t1, nB)
    if t0 >= t1:
        return []
    # cursor seeded by the closed form, then walked (tri_IJ)
    bq = 2.0 * TT + 1.0
    Jg = int((bq - math.sqrt(max(bq * bq - 8.0 * t0, 0.0))) * 0.5)
    Jg = max(0, min(TT - 1, Jg))
    cur_J, cur_c0 = Jg, Jg * TT - (Jg * (Jg - 1)) // 2
    out = []
    for tt in range(t0, t1):
        while cur_J + 1 < TT and tt >= cur_c0 + (TT - cur_J):
            cur_c0 += TT - cur_J
            cur_J += 1
        while cur_J > 0 and tt < cur_c0:
            cur_J -= 1
            cur_c0 -= TT - cur_J
        out.append((cur_J + (tt - cur_c0) + sub, cur_J))
    return out


def queue_items(T, run=DD_RUN):
    """The work items of the downdate ROLE inside k_mid's grid (dd_body<KC, true>, round 5): items 0 .. T-1 are class A (the tile below
    diagonal tile w, then that tile), then runs of `run` tiles of the triangle I >= J + 2, column by column; whoever is free takes the
    next item from RekfCtl::dd_queue."""
    nB = (T - 1) * (T - 2) // 2
    n_items = T + (nB + run - 1) // run
    items = []
    for it in range(n_items):
        if it < T:
            items.append(device_tiles(T, T + 1, 0, 0, 2, it) if False else ([(it + 1, it)] if it + 1 < T else []) + [(it, it)])
        else:
            t0, t1 = run * (it - T), min(run * (it - T) + run, nB)
            TT = T - 2
            out = []
            for tt in range(t0, t1):
                J = 0
                c0 = 0
                while tt >= c0 + (TT - J):
                    c0 += TT - J
                    J += 1
                out.append((J + (tt - c0) + 2, J))
            items.append(out)
    return items


# ---- the launches ------------------------------------------------------------------------------------------------------------
def slots_of(n_cu, n_front=0):
    """launch_downdate_any: the workgroups the static schedule plans for; n_front = 0: k_downdate2, n_front = K of the next scan:
    k_dd_front, whose front end takes min(K, FRONT_MB) workgroups (at least one) out of the schedule."""
    if n_front:
        n_front = min(max(n_front, 1), FRONT_MB)
    return max(n_cu * DD_WG_PER_CU - n_front, 8)


def role_wgs(n_cu, n, K_front):
    """rekf_launch_scan / rekf_scan_launch_fits: -> (workgroups of the downdate role inside k_mid's grid, its items, whether the host
    takes the one-launch form at all).  K_front: observations of the scan whose speculative front end rides behind the mid role
    (0: the host holds no next scan; for its decision the host takes the scan's own K as the bound).  Every role workgroup asks
    the queue until it is handed a number past the last item, so the queue ends at items + workgroups (rekf_debug_counters [24])."""
    n_mid = (n + MID_ROWS - 1) // MID_ROWS
    dd_first = (n_mid + max(K_front, 0) + 7) & ~7
    fits = dd_first + REKF_SCAN_MIN_DD_WGS <= n_cu and dd_first < 0x1000
    T = tiles_of(n)
    items = T + ((T - 1) * (T - 2) // 2 + DD_RUN - 1) // DD_RUN
    return min(max(n_cu - dd_first, 8), items), items, fits


# ---- what a static schedule is made of ---------------------------------------------------------------------------------------
def schedule(T, slots, derived=False):
    """-> (grid, lo, x, sub) as the launch runs it: the host's plan, or (derived) what the kernel makes of the host's grid."""
    grid, lo, x, sub = host_plan(T, slots)
    if derived:
        lo, x, sub = kernel_plan(T, grid)
    return grid, lo, x, sub


def forms(T, slots, derived=False):
    """The facts of a static schedule the range cases are chosen by.  -> dict:
    sub; lengths: the set of class-B range lengths; classA: the set of class-A tile counts; renumbered: the grid is renumbered per XCD
    non-trivially; cross: class-B ranges that cross a column; col0_mixed: those that hold a column-0 tile and a tile of another
    column; off_seed: those whose first look-up moves the cursor off its sqrt seed."""
    grid, lo, x, sub = schedule(T, slots, derived)
    out = dict(sub=sub, lengths=set(), classA=set(), renumbered=grid >= 16 and grid % 8 == 0, cross=0, col0_mixed=0, off_seed=0, grid=grid)
    TT = T - sub
    for b in range(grid):
        tl = device_tiles(T, grid, lo, x, sub, b)
        if not tl:
            continue
        if renumbered(grid, b) < T:
            out["classA"].add(len(tl))
            continue
        out["lengths"].add(len(tl))
        cols = {J for _, J in tl}
        out["cross"] += len(cols) > 1
        out["col0_mixed"] += 0 in cols and len(cols) > 1
        wq = renumbered(grid, b) - T
        out["off_seed"] += seed_column(TT, wq * lo + min(wq, x)) != tl[0][1]
    return out


FORMS = ("sub1_range2", "sub1_range3", "sub2_range3", "sub2_range4", "sub2_range5")


def form_of(T, slots, derived=False):
    """The named form of a static schedule: sub and the longest class-B range (None: no form the range cases name)."""
    f = forms(T, slots, derived)
    if not f["lengths"]:
        return None
    longest = max(f["lengths"])
    name = f"sub{f['sub']}_range{longest}"
    if name == "sub2_range3" and not (f["lengths"] == {2, 3} and 2 in f["classA"]):
        return None
    return name if name in FORMS else None


def smallest_T(form, slots, T_max=64):
    """The smallest tile count whose static schedule on `slots` workgroups has the named form; None when none up to T_max has."""
    assert form in FORMS, form
    for T in range(1, T_max + 1):
        if form_of(T, slots) == form:
            return T
    return None


def holder(T, slots, tile, derived=False):
    """-> (block, position in its range, the range) of the workgroup that holds `tile` in a static schedule."""
    grid, lo, x, sub = schedule(T, slots, derived)
    for b in range(grid):
        tl = device_tiles(T, grid, lo, x, sub, b)
        if tile in tl:
            return b, tl.index(tile), tl
    raise KeyError(tile)
