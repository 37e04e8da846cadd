"""What a linked submit (rfleet_submit_linked) does without a HIP call -- csrc/fleet_host.h's four steps given an rlink, and
csrc/fleet_link.h's taking rule, the text k_fleet_bind compiles for the device -- built host-only and run without a GPU
(tests/cpp/fleet_link_host.cpp), against a second, independent text of the rules as include/rfleet.h and csrc/fleet_host.h document
them:

    a linked scan (kind 2, K = the link's entry) whose entry has a record reserves 2 * max_obs floats of obs (max_obs 32, 256 on a wide
    fleet), is packed as a scan with K = 0 and gets a row {event, obs_off, record, slot} in | FleetBindRec[n_bind] at the next 16-byte
    boundary behind the segment; an entry with record -1 is packed as an empty scan; on a wide fleet a call with a bound scan takes the
    wide launch.

The program packs into a heap buffer of exactly `need` bytes filled with 0xA5, so the padding is part of the comparison."""
from __future__ import annotations

import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4
ODOM, SCAN, LINKED = 0, 1, 2
OK, INVALID, TOO_MANY_OBS, DET_CAPACITY = 0, -1, -3, -4
NARROW, NARROW_MAP, WIDE = 1, 2, 3                            # fleet_host.h's LastRec
FILL = 0xA5
EVENT = np.dtype([("dt", "<f8"), ("vt", "<f8", 3), ("kind", "<i4"), ("K", "<i4"), ("obs_off", "<i4"), ("fix_off", "<i4")])
BIND = np.dtype([("ev_at", "<i4"), ("obs_off", "<i4"), ("record", "<i4"), ("slot", "<i4")])
NAN = float("nan")
FIX = (0.02, -0.03, 0.01)


def odom(member, t, v=(0.5, 0.0, 0.1)):
    return dict(member=member, kind=ODOM, t=t, v=v, K=0, fix=None, xy=None)


def scan(member, t, K, fix=None):
    xy = (np.arange(2 * K, dtype=np.float32) * np.float32(0.125) + np.float32(member + t)).astype(np.float32)
    return dict(member=member, kind=SCAN, t=t, v=(0.0, 0.0, 0.0), K=K, fix=fix, xy=xy)


def linked(member, t, entry, fix=None):
    return dict(member=member, kind=LINKED, t=t, v=(0.0, 0.0, 0.0), K=entry, fix=fix, xy=None)


def fleet(wide=False, tracked=False, map_use=(0, 0, 0, 0), M_map=0, device=0):
    return dict(use_imu=(0, 1, 0, 0), time=[10.0, 20.0, 30.0, 40.0], vt=[(0.25 * b, 0.0, -0.125 * b) for b in range(B)], map_use=map_use,
                M_map=M_map, wide=wide, tracked=tracked, device=device)


def link(entries, device=0):
    """entries: [(member, stamp, host_status, record)]"""
    return dict(entries=entries, device=device)


LINK = link([(1, 20.5, 0, 0), (0, 10.5, 0, 1), (3, 40.5, 0, -1), (2, 30.5, -3, -1)])


# ---- the second text -------------------------------------------------------------------------------------------------------------
def take(K, err, max_centers, max_obs):
    if err != 0:
        return 0, err
    if K < 0 or K > max_centers:
        return 0, DET_CAPACITY
    if K > max_obs:
        return 0, TOO_MANY_OBS
    return K, 0


def validate(fl, events, lk):
    max_obs = 256 if fl["wide"] else 32
    used = set()
    for e in events:
        if not 0 <= e["member"] < B:
            return INVALID
        fix_ok = e["fix"] is None or all(math.isfinite(v) for v in e["fix"])
        if e["kind"] == LINKED:
            if lk is None or fl["tracked"] or lk["device"] != fl["device"]:
                return INVALID
            k = e["K"]
            if not 0 <= k < len(lk["entries"]) or k in used:
                return INVALID
            used.add(k)
            member, _, status, record = lk["entries"][k]
            if member != e["member"] or status != 0 or not -1 <= record < len(lk["entries"]) or not fix_ok:
                return INVALID
        elif e["kind"] == SCAN:
            if e["K"] < 0:
                return INVALID
            if e["K"] > max_obs:
                return TOO_MANY_OBS
            if not fix_ok:
                return INVALID
        elif e["kind"] != ODOM or e["fix"] is not None:
            return INVALID
    return OK


def a16(v):
    return (v + 15) & ~15


def expected(fl, events, lk):
    """-> what the program must print for an accepted untracked call."""
    max_obs = 256 if fl["wide"] else 32
    time, vt = list(fl["time"]), [list(v) for v in fl["vt"]]
    kept, cnt, scanned = [], [0] * B, []
    for e in events:
        b = e["member"]
        if e["kind"] == ODOM:
            if fl["use_imu"][b] or e["t"] < time[b]:
                continue
            vt[b] = list(e["v"])
        else:
            scanned.append(b)
        kept.append((e, e["t"] - time[b], tuple(vt[b])))
        time[b] = e["t"]
        cnt[b] += 1
    bound = lambda e: e["kind"] == LINKED and lk["entries"][e["K"]][3] >= 0
    E, G = len(kept), sum(c > 0 for c in cnt)
    n_obs = sum(e["K"] for e, _, _ in kept if e["kind"] == SCAN) + max_obs * sum(bound(e) for e, _, _ in kept)
    n_fix = sum(e["fix"] is not None for e, _, _ in kept)
    n_wide = sum(e["kind"] == SCAN and e["K"] > 32 for e, _, _ in kept)
    n_linked, n_bind = sum(e["kind"] == LINKED for e, _, _ in kept), sum(bound(e) for e, _, _ in kept)
    wide_launch = n_wide > 0 or (fl["wide"] and n_bind > 0)
    with_map = any(cnt[b] > 0 and fl["M_map"] > 0 and fl["map_use"][b] for b in range(B))
    rec = WIDE if wide_launch else NARROW_MAP if with_map else NARROW
    members = [b for b in range(B) if cnt[b]]
    begin = np.concatenate([[0], np.cumsum([cnt[b] for b in members])]).astype("<i4")
    at_of, nxt = {}, {b: int(begin[g]) for g, b in enumerate(members)}
    rows, obs, fixes, binds, known, slot = {}, [], [], [], [], 0
    for q, (e, dt, v) in enumerate(kept):                     # call order: observations, fixes, bind rows; events grouped by member
        at = nxt[e["member"]]
        nxt[e["member"]] += 1
        fix_off = -1
        if e["fix"] is not None:
            fix_off = len(fixes)
            fixes += list(e["fix"])
        off = len(obs)
        if e["kind"] == SCAN:
            rows[at] = (dt, v, 1, e["K"], off, fix_off)
            obs += e["xy"].tolist()
        elif e["kind"] == LINKED:
            rows[at] = (dt, v, 1, 0, off, fix_off)
            record = lk["entries"][e["K"]][3]
            known.append(int(record < 0))
            if record >= 0:
                binds.append((at, off, record, slot))
                obs += [None] * (2 * max_obs)                 # reserved: the program leaves its fill there
            slot += 1
        else:
            rows[at] = (dt, v, 0, 0, off, -1)
    off_mem = 0
    off_beg = a16(off_mem + 4 * G)
    off_ev = a16(off_beg + 4 * (G + 1))
    off_fix = a16(off_ev + 48 * E)
    off_obs = a16(off_fix + 8 * len(fixes))
    need = a16(off_obs + 4 * len(obs) + 16)
    off_track = (need + 127) & ~127
    off_bind = 0
    if n_bind:
        off_bind = a16(need)
        need = off_bind + 16 * n_bind
    seg = np.full(need, FILL, np.uint8)
    fill32 = np.frombuffer(bytes([FILL] * 4), "<f4")[0]
    parts = ((off_mem, np.array(members, "<i4")), (off_beg, begin), (off_ev, np.array([rows[a] for a in range(E)], EVENT)),
             (off_fix, np.array(fixes, "<f8")), (off_obs, np.array([fill32 if v is None else v for v in obs], "<f4")),
             (off_bind, np.array(binds, BIND)))
    for off, part in parts:
        raw = np.frombuffer(part.tobytes(), np.uint8)
        seg[off: off + raw.size] = raw
    return dict(plan=(E, G, n_obs, n_fix, n_wide, int(with_map), rec, n_linked, n_bind, max_obs, int(wide_launch)), cnt=cnt, scanned=scanned,
                next=(time, [x for v in vt for x in v]), layout=(off_mem, off_beg, off_ev, off_fix, off_obs, off_track, off_bind, need),
                seg=seg.tobytes(), known=known)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
MIXED = [scan(0, 10.1, 3), linked(1, 20.5, 0), odom(2, 30.1), scan(2, 30.2, 2), linked(3, 40.5, 2), linked(0, 10.5, 1, fix=FIX), scan(3, 40.6, 1),
         odom(0, 10.6), scan(1, 20.6, 2, fix=(1.0, 2.0, -3.0))]
UNLINKED = [scan(2, 30.1, 3), odom(0, 10.1), scan(2, 30.2, 1, fix=FIX), scan(3, 40.1, 2), odom(0, 10.2, (0.7, 0.0, 0.0)), scan(0, 10.3, 4)]
ACCEPTED = {
    "mixed_narrow": (fleet(), MIXED, LINK),
    "mixed_wide": (fleet(wide=True), MIXED, LINK),
    "no_record_on_a_wide_fleet": (fleet(wide=True), [scan(0, 10.1, 32), linked(3, 40.5, 2), scan(2, 30.1, 1)], LINK),
    "a_known_wide_scan_too": (fleet(wide=True), [scan(0, 10.1, 33), linked(1, 20.5, 0), scan(2, 30.1, 1)], LINK),
    "on_the_map": (fleet(map_use=(0, 1, 0, 0), M_map=3), [linked(1, 20.5, 0), scan(0, 10.5, 1)], LINK),
    "linked_only": (fleet(), [linked(0, 10.5, 1), linked(1, 20.5, 0)], LINK),
    "unlinked": (fleet(), UNLINKED, LINK),
    "unlinked_wide": (fleet(wide=True), UNLINKED + [scan(1, 20.5, 40)], LINK),
    "unlinked_without_a_link": (fleet(), UNLINKED, None),
}
REFUSED = {
    "entry_outside": (fleet(), [scan(0, 10.1, 2), linked(1, 20.5, 4)], LINK),
    "entry_negative": (fleet(), [linked(1, 20.5, -1)], LINK),
    "entry_twice": (fleet(), [linked(1, 20.5, 0), odom(0, 10.5), linked(1, 20.6, 0)], LINK),
    "wrong_member": (fleet(), [odom(0, 10.5), linked(2, 30.5, 0)], LINK),
    "host_status": (fleet(), [linked(2, 30.5, 3)], LINK),
    "another_device": (fleet(device=1), [linked(1, 20.5, 0)], LINK),
    "tracked": (fleet(tracked=True), [odom(0, 10.5), linked(1, 20.5, 0)], LINK),
    "no_link": (fleet(), [odom(0, 10.5), linked(1, 20.5, 0)], None),
    "fix_nan": (fleet(), [linked(1, 20.5, 0, fix=(0.0, NAN, 0.0))], LINK),
    "record_outside": (fleet(), [linked(1, 20.5, 0)], link([(1, 20.5, 0, 1)])),
    "too_many_behind_a_linked": (fleet(), [linked(1, 20.5, 0), scan(0, 10.5, 33)], LINK),
}
TAKES = [(K, err, 256, max_obs) for K in (-1, 0, 1, 32, 33, 256, 257) for err in (0, -4, -5) for max_obs in (32, 256)]


def h(v):
    return float(v).hex()


def submit_record(fl, events, lk, as_linked):
    n_link = -1 if lk is None else len(lk["entries"])
    lines = ["submit %d %d %d %d %d %d %d %d %d" % (B, fl["wide"], fl["tracked"], fl["M_map"], fl["device"], as_linked, n_link,
                                                    0 if lk is None else lk["device"], len(events))]
    for b in range(B):
        lines.append("%d %s %s %d" % (fl["use_imu"][b], h(fl["time"][b]), " ".join(h(v) for v in fl["vt"][b]), fl["map_use"][b]))
    for member, stamp, status, record in ([] if lk is None else lk["entries"]):
        lines.append("%d %s %d %d" % (member, h(stamp), status, record))
    for e in events:
        fix = e["fix"] or (0.0, 0.0, 0.0)
        lines.append("%d %d %s %s %d %d %s 0" % (e["member"], e["kind"], h(e["t"]), " ".join(h(v) for v in e["v"]), e["K"], e["fix"] is not None,
                                                 " ".join(h(v) for v in fix)))
        if e["kind"] == SCAN and e["K"] > 0:
            lines.append(" ".join(h(v) for v in e["xy"]))
    return "\n".join(lines) + "\n"


def parse_submit(lines):
    out = {"rc": int(lines.pop(0).split()[1])}
    floats = lambda t: [float.fromhex(v) for v in t]
    t = lines.pop(0).split()
    assert t[0] == "mirror"
    out["mirror"] = (floats(t[1: 1 + B]), floats(t[1 + B:]))
    if out["rc"] != OK:
        return out
    out["text"] = list(lines[:7])
    out["plan"] = tuple(int(v) for v in lines.pop(0).split()[1:])
    out["cnt"] = [int(v) for v in lines.pop(0).split()[1:]]
    out["scanned"] = [int(v) for v in lines.pop(0).split()[1:]]
    t = lines.pop(0).split()
    out["next"] = (floats(t[1: 1 + B]), floats(t[1 + B:]))
    out["layout"] = tuple(int(v) for v in lines.pop(0).split()[1:])
    out["seg"] = bytes.fromhex(lines.pop(0).split()[1])
    out["known"] = [int(v) for v in lines.pop(0).split()[1:]]
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """tests/cpp/fleet_link_host.cpp, built host-only, run once over every record of this file: name -> the parsed answer."""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    tmp = tmp_path_factory.mktemp("fleet_link_host")
    exe, path = str(tmp / "fleet_link_host"), str(tmp / "cases.txt")
    r = subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "fleet_link_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    names = []
    with open(path, "w") as f:
        for name, (fl, events, lk) in ACCEPTED.items():
            f.write(submit_record(fl, events, lk, 1))
            names.append(name)
        for name, (fl, events, lk) in REFUSED.items():
            f.write(submit_record(fl, events, lk, 1))
            names.append(name)
        for name in ("unlinked", "unlinked_wide"):            # the same calls as rfleet_submit makes them
            f.write(submit_record(*ACCEPTED[name][:2], None, 0))
            names.append(name + "/submit")
        f.write(submit_record(*REFUSED["no_link"][:2], None, 0))                           # rfleet_submit keeps refusing kind 2
        names.append("kind_2/submit")
        for t in TAKES:
            f.write("take %d %d %d %d\n" % t)
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    out = {key: parse_submit(lines) for key in names}
    out["takes"] = [tuple(int(v) for v in line.split()[1:]) for line in lines]
    assert len(out["takes"]) == len(TAKES)
    return out


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_an_accepted_call_plans_and_packs_the_documented_bytes(answers, name):
    fl, events, lk = ACCEPTED[name]
    assert validate(fl, events, lk) == OK
    got, want = answers[name], expected(fl, events, lk)
    assert got["rc"] == OK
    assert got["mirror"] == (fl["time"], [x for v in fl["vt"] for x in v])                 # the plan works on a copy
    assert got["plan"] == want["plan"] and got["cnt"] == want["cnt"] and got["scanned"] == want["scanned"]
    assert got["next"] == want["next"] and got["layout"] == want["layout"]
    assert len(got["seg"]) == want["layout"][7] and got["seg"] == want["seg"]
    assert got["known"] == want["known"]


def test_the_cases_are_the_ones_they_claim_to_be(answers):
    plan = lambda name: answers[name]["plan"]
    # reserved floats per bound scan, obs_off of the host scans behind them, the choice of the launch, who owns the records
    assert plan("mixed_narrow")[2] == 3 + 2 + 1 + 2 + 2 * 32 and plan("mixed_narrow")[6:] == (NARROW, 3, 2, 32, 0)
    assert plan("mixed_wide")[2] == 3 + 2 + 1 + 2 + 2 * 256 and plan("mixed_wide")[6:] == (WIDE, 3, 2, 256, 1) and plan("mixed_wide")[4] == 0
    a = answers["mixed_narrow"]
    ev = np.frombuffer(a["seg"], EVENT, a["plan"][0], a["layout"][2])
    binds = np.frombuffer(a["seg"], BIND, a["plan"][8], a["layout"][6])
    assert ev["kind"].tolist() == [1, 1, 0, 1, 1, 0, 1, 1, 1] and ev["K"].tolist() == [3, 0, 0, 0, 2, 0, 2, 0, 1]   # (grouped by member)
    assert ev["obs_off"].tolist() == [0, 74, 140, 6, 140, 70, 70, 74, 138]                 # 6 | 64 reserved | 4 | 64 reserved | 2 | 4
    assert binds.tolist() == [(3, 6, 0, 0), (1, 74, 1, 2)] and a["known"] == [0, 1, 0]
    assert a["layout"][7] == a["layout"][6] + 32 and a["layout"][6] % 16 == 0
    assert plan("no_record_on_a_wide_fleet")[6:] == (NARROW, 1, 0, 256, 0) and answers["no_record_on_a_wide_fleet"]["layout"][6] == 0
    assert plan("a_known_wide_scan_too")[4] == 1 and plan("a_known_wide_scan_too")[6:] == (WIDE, 1, 1, 256, 1)
    assert plan("on_the_map")[5:7] == (1, NARROW_MAP) and plan("linked_only")[:3] == (2, 2, 64)


def test_without_a_linked_event_the_call_is_rfleet_submit_byte_for_byte(answers):
    for name in ("unlinked", "unlinked_wide"):
        assert answers[name]["text"] == answers[name + "/submit"]["text"] and answers[name]["plan"][7:9] == (0, 0)
    assert answers["unlinked_without_a_link"]["text"] == answers["unlinked/submit"]["text"]
    assert answers["unlinked_wide"]["plan"][4] == 1 and answers["unlinked"]["layout"][6] == 0


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_a_refusal_is_invalid_and_moves_nothing(answers, name):
    fl, events, lk = REFUSED[name]
    want = TOO_MANY_OBS if name == "too_many_behind_a_linked" else INVALID
    assert validate(fl, events, lk) == want
    got = answers[name]
    assert got["rc"] == want and got["mirror"] == (fl["time"], [x for v in fl["vt"] for x in v])


def test_rfleet_submit_keeps_refusing_the_kind(answers):
    assert answers["kind_2/submit"]["rc"] == INVALID


def test_the_taking_rule_over_the_table(answers):
    assert len(TAKES) == 7 * 3 * 2
    assert answers["takes"] == [take(*t) for t in TAKES]
    table = dict(zip(TAKES, answers["takes"]))
    assert table[(33, 0, 256, 32)] == (0, TOO_MANY_OBS) and table[(33, 0, 256, 256)] == (33, 0) and table[(32, 0, 256, 32)] == (32, 0)
    assert table[(257, 0, 256, 256)] == (0, DET_CAPACITY) and table[(-1, 0, 256, 32)] == (0, DET_CAPACITY) and table[(256, 0, 256, 256)] == (256, 0)
    assert table[(1, -5, 256, 32)] == (0, -5) and table[(257, -4, 256, 32)] == (0, -4) and table[(0, 0, 256, 32)] == (0, 0)
