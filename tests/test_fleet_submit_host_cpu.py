"""The steps of rfleet_submit that need no HIP call (csrc/fleet_host.h: submit_validate, submit_plan, submit_layout, submit_pack) and
members_named_once, built host-only and run without a GPU (tests/cpp/fleet_submit_host.cpp), against a second, independent text of
the segment's layout as csrc/fleet_dev.h and csrc/rfleet_api.hip document it:

    members[G] | ev_begin[G + 1] | FleetEvent[E] | fix[3 n_fix] | obs[2 n_obs]      each part at the next 16-byte boundary,
    16 bytes of slack behind obs, and for a tracked submit | FleetTrackRec[E] at the next 128-byte boundary

written below with numpy structured arrays.  The program packs into a heap buffer of exactly `need` bytes filled with 0xA5, so the
padding is part of the comparison."""
from __future__ import annotations

import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4
ODOM, SCAN = 0, 1
OK, INVALID, TOO_MANY_OBS = 0, -1, -3                         # REKF_OK, REKF_ERR_INVALID, REKF_ERR_TOO_MANY_OBS of include/rekf.h
NONE, NARROW, NARROW_MAP, WIDE = 0, 1, 2, 3                   # fleet_host.h's LastRec
FILL = 0xA5
EVENT = np.dtype([("dt", "<f8"), ("vt", "<f8", 3), ("kind", "<i4"), ("K", "<i4"), ("obs_off", "<i4"), ("fix_off", "<i4")])
assert EVENT.itemsize == 48
NAN, INF = float("nan"), float("inf")


def odom(member, t, v=(0.5, 0.0, 0.1), fix=None):
    return dict(member=member, kind=ODOM, t=t, v=v, K=0, fix=fix, xy=None, xy_null=False)


def scan(member, t, K, fix=None, xy_null=False, kind=SCAN, seed=0):
    xy = (np.arange(2 * max(K, 0), dtype=np.float32) * np.float32(0.125) + np.float32(member + 10 * seed + t)).astype(np.float32)
    return dict(member=member, kind=kind, t=t, v=(0.0, 0.0, 0.0), K=K, fix=fix, xy=xy, xy_null=xy_null)


def fleet(use_imu=(0, 1, 0, 0), map_use=(0, 0, 0, 0), M_map=0, wide=False):
    """The handle's side of a submit: per member use_imu, the mirror (time, vt) and the map switch."""
    return dict(use_imu=use_imu, time=[10.0, 20.0, 30.0, 40.0], vt=[(0.25 * b, 0.0, -0.125 * b) for b in range(B)], map_use=map_use,
                M_map=M_map, wide=wide)


# ---- the second text -------------------------------------------------------------------------------------------------------------
def validate(fl, events):
    max_obs = 256 if fl["wide"] else 32
    for e in events:
        if not 0 <= e["member"] < B or e["kind"] not in (ODOM, SCAN):
            return INVALID
        if e["kind"] == SCAN:
            if e["K"] < 0:
                return INVALID
            if e["K"] > max_obs:
                return TOO_MANY_OBS
            if e["K"] > 0 and e["xy_null"]:
                return INVALID
            if e["fix"] is not None and not all(math.isfinite(v) for v in e["fix"]):
                return INVALID
        elif e["fix"] is not None:
            return INVALID
    return OK


def a16(v):
    return (v + 15) & ~15


def expected(fl, events, tracked):
    """-> what the program must print for an accepted call: plan, counts, the next mirror, offsets, the segment's bytes, the meta."""
    time, vt = list(fl["time"]), [list(v) for v in fl["vt"]]
    kept, cnt, scanned = [], [0] * B, []                      # kept: (event, dropped, dt, velocity) in call order
    for e in events:
        b = e["member"]
        if e["kind"] == ODOM:
            if fl["use_imu"][b] or e["t"] < time[b]:
                if tracked:
                    kept.append((e, 1, 0.0, (0.0, 0.0, 0.0)))
                    cnt[b] += 1
                continue
            vt[b] = list(e["v"])
        else:
            scanned.append(b)
        kept.append((e, 0, e["t"] - time[b], tuple(vt[b])))
        time[b] = e["t"]
        cnt[b] += 1
    scans = [e for e, dr, _, _ in kept if e["kind"] == SCAN]
    E, G = len(kept), sum(c > 0 for c in cnt)
    n_obs, n_fix, n_wide = sum(e["K"] for e in scans), sum(e["fix"] is not None for e in scans), sum(e["K"] > 32 for e in scans)
    with_map = any(cnt[b] > 0 and fl["M_map"] > 0 and fl["map_use"][b] for b in range(B))
    rec = WIDE if n_wide else NARROW_MAP if (with_map or tracked) else NARROW
    # the parts: observations and fixes in CALL order, the events grouped by member (stable)
    rows, obs, fixes = [], [], []
    for e, dr, dt, v in kept:
        if dr:
            rows.append((e["member"], (0.0, (0.0, 0.0, 0.0), 2, 0, len(obs), -1)))
            continue
        is_scan = e["kind"] == SCAN
        fix_off = -1
        if is_scan and e["fix"] is not None:
            fix_off = len(fixes)
            fixes += list(e["fix"])
        rows.append((e["member"], (dt, v, 1 if is_scan else 0, e["K"] if is_scan else 0, len(obs), fix_off)))
        if is_scan:
            obs += e["xy"].tolist()
    members = np.array([b for b in range(B) if cnt[b]], "<i4")
    ev_begin = np.concatenate([[0], np.cumsum([cnt[b] for b in members])]).astype("<i4")
    grouped = np.array([r for b in members for m, r in rows if m == b], EVENT)
    metas = [(e["t"], e["member"], e["kind"], e["K"] if e["kind"] == SCAN else 0, dr) for b in members for e, dr, _, _ in kept if e["member"] == b]
    off_mem = 0
    off_beg = a16(off_mem + 4 * G)
    off_ev = a16(off_beg + 4 * (G + 1))
    off_fix = a16(off_ev + 48 * E)
    off_obs = a16(off_fix + 8 * len(fixes))
    need = a16(off_obs + 4 * len(obs) + 16)
    off_track = (need + 127) & ~127
    if tracked:
        need = off_track + 128 * E
    seg = np.full(need, FILL, np.uint8)
    for off, part in ((off_mem, members), (off_beg, ev_begin), (off_ev, grouped), (off_fix, np.array(fixes, "<f8")), (off_obs, np.array(obs, "<f4"))):
        raw = np.frombuffer(part.tobytes(), np.uint8)
        seg[off: off + raw.size] = raw
    return dict(plan=(E, G, n_obs, n_fix, n_wide, int(with_map), rec), cnt=cnt, scanned=scanned, next=(time, [x for v in vt for x in v]),
                layout=(off_mem, off_beg, off_ev, off_fix, off_obs, off_track, need), seg=seg.tobytes(), meta=metas if tracked else [])


# ---- the cases -------------------------------------------------------------------------------------------------------------------
FIX = (0.02, -0.03, 0.01)
ACCEPTED = {
    "interleaved": (fleet(), [scan(2, 30.1, 3), odom(0, 10.1), scan(2, 30.2, 1), scan(3, 40.1, 2), odom(0, 10.2, (0.7, 0.0, 0.0)), scan(0, 10.3, 4),
                              odom(2, 30.3), scan(2, 30.4, 2), odom(3, 40.2), scan(0, 10.4, 1)]),
    "stale_odometry": (fleet(), [odom(0, 9.5, (9.0, 9.0, 9.0)), odom(0, 10.5), odom(2, 30.5), odom(2, 30.25, (8.0, 8.0, 8.0)), scan(2, 30.75, 2),
                                 odom(0, 10.5, (0.75, 0.0, 0.0))]),
    "use_imu": (fleet(), [odom(1, 20.5, (9.0, 9.0, 9.0)), scan(1, 20.75, 2), odom(1, 21.0), odom(3, 40.5), scan(1, 21.5, 1)]),
    "empty_scan": (fleet(), [scan(0, 10.5, 0), scan(3, 40.5, 2), scan(3, 40.75, 0, fix=FIX)]),
    "fix": (fleet(), [scan(3, 40.5, 2, fix=FIX), scan(0, 10.5, 3), scan(0, 10.75, 1, fix=(1.0, 2.0, -3.0)), odom(2, 30.5)]),
    "K32": (fleet(), [scan(1, 20.5, 32), scan(2, 30.5, 1)]),
    "K33_wide": (fleet(wide=True), [scan(2, 30.5, 1), scan(1, 20.5, 33, fix=FIX), odom(0, 10.5), scan(1, 20.75, 2)]),
    "all_dropped": (fleet(), [odom(1, 20.5), odom(0, 9.0), odom(1, 21.0), odom(2, 29.5)]),
    "on_the_map": (fleet(map_use=(0, 0, 1, 0), M_map=3), [scan(2, 30.5, 2), scan(0, 10.5, 1)]),
    "map_of_another_member": (fleet(map_use=(0, 0, 1, 0), M_map=3), [scan(3, 40.5, 2), odom(0, 10.5)]),
    "empty_map": (fleet(map_use=(1, 1, 1, 1), M_map=0), [scan(3, 40.5, 2)]),
}
REFUSED = {
    "member_4": (fleet(), [scan(0, 10.5, 1), scan(4, 1.0, 1)], INVALID),
    "member_negative": (fleet(), [odom(-1, 1.0)], INVALID),
    "kind_2": (fleet(), [odom(0, 10.5), scan(1, 20.5, 1, kind=2)], INVALID),
    "K_negative": (fleet(), [scan(1, 20.5, -1)], INVALID),
    "K33_wide_off": (fleet(), [scan(0, 10.5, 32), scan(1, 20.5, 33)], TOO_MANY_OBS),
    "K257_wide_on": (fleet(wide=True), [scan(0, 10.5, 256), scan(1, 20.5, 257)], TOO_MANY_OBS),
    "K33_null_xy": (fleet(), [scan(1, 20.5, 33, xy_null=True)], TOO_MANY_OBS),             # (the count is looked at before the pointer)
    "too_many_before_a_bad_member": (fleet(), [scan(1, 20.5, 33), scan(7, 1.0, 1)], TOO_MANY_OBS),
    "bad_member_before_too_many": (fleet(), [scan(7, 1.0, 1), scan(1, 20.5, 33)], INVALID),
    "null_xy": (fleet(), [scan(0, 10.5, 2), scan(1, 20.5, 2, xy_null=True)], INVALID),
    "fix_nan": (fleet(), [scan(0, 10.5, 2, fix=(0.0, NAN, 0.0))], INVALID),
    "fix_inf": (fleet(), [scan(0, 10.5, 0, fix=(0.0, 0.0, -INF))], INVALID),
    "fix_on_odometry": (fleet(), [scan(0, 10.5, 2, fix=FIX), odom(1, 20.5, fix=FIX)], INVALID),
}
MEMBERS = [((B, None), 1), ((B - 1, None), 0), ((B + 1, None), 0), ((0, None), 0), ((3, [2, 0, 3]), 1), ((B, [3, 2, 1, 0]), 1), ((0, []), 1),
           ((3, [2, 0, 2]), 0), ((2, [0, B]), 0), ((2, [-1, 0]), 0), ((B + 1, [0, 1, 2, 3, 0]), 0), ((B + 1, [0, 1, 2, 3, 4]), 0)]


def h(v):
    return float(v).hex()


def submit_record(fl, events, tracked):
    lines = ["submit %d %d %d %d %d" % (B, fl["wide"], tracked, fl["M_map"], len(events))]
    for b in range(B):
        lines.append("%d %s %s %d" % (fl["use_imu"][b], h(fl["time"][b]), " ".join(h(v) for v in fl["vt"][b]), fl["map_use"][b]))
    for e in events:
        fix = e["fix"] or (0.0, 0.0, 0.0)
        lines.append("%d %d %s %s %d %d %s %d" % (e["member"], e["kind"], h(e["t"]), " ".join(h(v) for v in e["v"]), e["K"], e["fix"] is not None,
                                                   " ".join(h(v) for v in fix), e["xy_null"]))
        if e["K"] > 0 and not e["xy_null"]:
            lines.append(" ".join(h(v) for v in e["xy"]))
    return "\n".join(lines) + "\n"


def parse_submit(lines):
    """One submit's answer off the front of `lines` -> a dict like expected()'s, with rc and the mirror."""
    out = {"rc": int(lines.pop(0).split()[1])}
    floats = lambda t: [float.fromhex(v) for v in t]
    t = lines.pop(0).split()
    assert t[0] == "mirror"
    out["mirror"] = (floats(t[1: 1 + B]), floats(t[1 + B:]))
    if out["rc"] != OK:
        return out
    out["plan"] = tuple(int(v) for v in lines.pop(0).split()[1:])
    out["cnt"] = [int(v) for v in lines.pop(0).split()[1:]]
    out["scanned"] = [int(v) for v in lines.pop(0).split()[1:]]
    t = lines.pop(0).split()
    out["next"] = (floats(t[1: 1 + B]), floats(t[1 + B:]))
    out["layout"] = tuple(int(v) for v in lines.pop(0).split()[1:])
    out["seg"] = bytes.fromhex(lines.pop(0).split()[1])
    n = int(lines.pop(0).split()[1])
    out["meta"] = []
    for _ in range(n):
        t = lines.pop(0).split()
        out["meta"].append((float.fromhex(t[0]),) + tuple(int(v) for v in t[1:]))
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """tests/cpp/fleet_submit_host.cpp, built host-only, run once over every record of this file: name -> the parsed answer."""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    tmp = tmp_path_factory.mktemp("fleet_submit_host")
    exe, path = str(tmp / "fleet_submit_host"), str(tmp / "cases.txt")
    r = subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "fleet_submit_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    names = []
    with open(path, "w") as f:
        for name, (fl, events) in ACCEPTED.items():
            for tracked in (0, 1):
                f.write(submit_record(fl, events, tracked))
                names.append((name, tracked))
        for name, (fl, events, _) in REFUSED.items():
            for tracked in (0, 1):
                f.write(submit_record(fl, events, tracked))
                names.append((name, tracked))
        for (count, lst), _ in MEMBERS:
            f.write("members %d %d %d %s\n" % (B, count, lst is not None, " ".join(str(m) for m in lst or [])))
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    out = {key: parse_submit(lines) for key in names}
    out["members"] = [int(line.split()[1]) for line in lines]
    assert len(out["members"]) == len(MEMBERS)
    return out


@pytest.mark.parametrize("tracked", [0, 1])
@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_an_accepted_call_packs_the_documented_bytes(answers, name, tracked):
    fl, events = ACCEPTED[name]
    assert validate(fl, events) == OK and len(events) <= 10
    got, want = answers[(name, tracked)], expected(fl, events, tracked)
    assert got["rc"] == OK
    assert got["mirror"] == (fl["time"], [x for v in fl["vt"] for x in v])                 # the plan works on a copy
    assert got["plan"] == want["plan"] and got["cnt"] == want["cnt"] and got["scanned"] == want["scanned"]
    assert got["next"] == want["next"]
    if want["plan"][0] == 0:                                  # every event dropped, untracked: rfleet_submit returns here, no launch
        assert name == "all_dropped" and not tracked and want["plan"][1] == 0 and got["next"] == got["mirror"]
        return
    assert got["layout"] == want["layout"]
    assert len(got["seg"]) == want["layout"][6] and got["seg"] == want["seg"]
    assert got["meta"] == want["meta"]


def test_the_cases_are_the_ones_they_claim_to_be(answers):
    plan = lambda name, tracked=0: answers[(name, tracked)]["plan"]
    assert plan("all_dropped") == (0, 0, 0, 0, 0, 0, NARROW) and plan("all_dropped", 1) == (4, 3, 0, 0, 0, 0, NARROW_MAP)
    kinds = np.frombuffer(answers[("all_dropped", 1)]["seg"], EVENT, 4, answers[("all_dropped", 1)]["layout"][2])["kind"]
    assert kinds.tolist() == [2, 2, 2, 2]
    assert plan("stale_odometry")[0] == 4 and plan("stale_odometry", 1)[0] == 6 and plan("use_imu")[0] == 3 and plan("use_imu", 1)[0] == 5
    assert plan("K32")[4:] == (0, 0, NARROW) and plan("K33_wide")[4:] == (1, 0, WIDE) and plan("K33_wide", 1)[6] == WIDE
    assert plan("on_the_map")[5:] == (1, NARROW_MAP) and plan("map_of_another_member")[5:] == (0, NARROW) and plan("empty_map")[5:] == (0, NARROW)
    assert plan("fix")[3] == 2 and plan("empty_scan")[2:4] == (2, 1) and plan("interleaved")[:2] == (10, 3)
    for name in ACCEPTED:                                     # tracked and untracked runs of the same input: the same front part
        a, b = answers[(name, 0)], answers[(name, 1)]
        if a["plan"][0] == b["plan"][0]:
            assert a["layout"][:6] == b["layout"][:6] and b["seg"][: a["layout"][6]] == a["seg"] and a["next"] == b["next"]
            assert b["layout"][6] == a["layout"][5] + 128 * a["plan"][0] and a["layout"][5] % 128 == 0
        assert a["next"] == b["next"]                         # (a dropped message moves nothing, tracked or not)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_a_refusal_has_its_code_and_leaves_the_mirror(answers, name):
    fl, events, code = REFUSED[name]
    assert validate(fl, events) == code
    for tracked in (0, 1):
        got = answers[(name, tracked)]
        assert got["rc"] == code and got["mirror"] == (fl["time"], [x for v in fl["vt"] for x in v])


def test_members_named_once(answers):
    assert answers["members"] == [want for _, want in MEMBERS]
