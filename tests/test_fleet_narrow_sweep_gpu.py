"""Fleet filter, the shape sweep of the three other narrow compiles on the GPU (-m gpu): k_fleet_step_fix against the joint pose
witness and k_fleet_step_map against the map witness on the tables of tests/fleet_narrow_sweep_cases.py, the plain sweep's 117 cases
through all three compiles (within fleet_cases.SUITE's bound of the witness and bit for bit what k_fleet_step leaves), both tables in
tracked fleets (k_fleet_step_track: record by record against an untracked twin), and eight map members in other call patterns.

No counter says which compile ran.  The host's choice is deterministic (track, else a member with events on a non-empty map, else a
fix in the submit, else plain), so each test arranges it and asserts what can be seen of it: a fix moved the state (the same run
without fixes gives other bits and misses the witness), a map member's record carries map pairs, track records exist.

Worst figures on an MI355X, as multiples of each suite's measured FP64 floor (bound: 16; printed by the tests, run with -s): fix
table sigma 0.84 x (nfix_L17_MM15_N6_diff_fix scan 0), mu 11.6 x (nfix_L61_MM24_N4_omni_fix; the rows-first two-step ORDER's own
round-off: the same two steps in FP64 numpy are 27 x off there, the joint solve 0.7 x); map table sigma 3.5 x, mu 7.4 x
(nmap_L11_MM16_N3_omni); the plain sweep under the three compiles sigma 1.20 x, mu 0.96 x of fleet_cases.SUITE's floor, and bit for
bit k_fleet_step's.  No kernel line had to change ("Shape sweep of the fix, map and track compiles")."""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as FM
from tests import fleet_narrow_sweep_cases as NC
from tests import fleet_track_cases as TC
from tests import fleet_wide_cases as WC
from tests.witness import fleet_witness as WT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not WT.available(), reason="numpy.longdouble has no 64-bit mantissa here")]


# ---- the two tables: fleets, references, one lockstep run each, kept for the tests behind ---------------------------------------------
def fix_fleet(cases, track=False):
    """A fleet without a map: a submit with a fix takes k_fleet_step_fix."""
    fl = H.make_fleet(cases)
    if track:
        fl.track(True)
    return fl


def map_fleet(cases, track=False):
    """A fleet on the standard map, narrow scans only: a submit with a member on the map takes k_fleet_step_map."""
    return WC.make_fleet(cases, wide=False, track=track)


TABLES = {"fix": NS(cases=NC.fix_cases, runs=NC.fix_runs, suite=NC.FIX_SUITE, fleet=fix_fleet, check=H.check_member),
          "map": NS(cases=NC.map_cases, runs=NC.map_runs, suite=NC.MAP_SUITE, fleet=map_fleet, check=FM.check_member)}


def witness_at(runs, case, k):
    """The suite's longdouble witness behind scan k of the case, computed once on the CPU side (fix_runs / map_runs)."""
    ref = runs[case.name][k][0][0]
    return NS(state=lambda: ref)


def tick(cases, k, with_fix=True):
    return [FC.fev(i, c.events[k], with_fix) for i, c in enumerate(cases)]


def lockstep(which, with_fix=True):
    """All cases of a table as members of ONE fleet, one submit per tick; with fixes every scan is checked as
    fleet_harness.run_lockstep / fleet_map_cases.run_lockstep check it (a miss is recorded and the run goes on).  -> the bits behind
    each tick, n, flags, the worst (sigma error, where), (mu error, where) as multiples of the floor, the misses."""
    t = TABLES[which]
    cases, runs = t.cases(), t.runs()
    fl = t.fleet(cases)
    out = NS(bits=[], worst_s=(0.0, ""), worst_m=(0.0, ""), misses=[])
    try:
        for k in range(2):
            fl.submit(tick(cases, k, with_fix))
            for i, c in enumerate(cases):
                if not with_fix:
                    continue
                try:
                    fs, fm = t.check(fl, i, c, k, witness_at(runs, c, k), t.suite)
                except AssertionError as err:
                    out.misses.append(str(err))
                    continue
                out.worst_s, out.worst_m = max(out.worst_s, (fs, f"{c.name} scan {k}")), max(out.worst_m, (fm, f"{c.name} scan {k}"))
            out.bits.append([FC.state_bits(fl, i) for i in range(len(cases))])
        out.n, out.flags = fl.n().copy(), fl.flags().copy()
    finally:
        fl.close()
    return out


_left = {}


def left(which):
    """What the lockstep run of a table left: run once, shared by the tests."""
    if which not in _left:
        _left[which] = lockstep(which)
    return _left[which]


def report(what, r, count):
    print(f"\nworst of {count} {what}: sigma {r.worst_s[0]:.2f} x the floor at {r.worst_s[1]}; mu {r.worst_m[0]:.2f} x at {r.worst_m[1]}")
    assert not r.misses, "\n".join(r.misses)
    assert 0 < r.worst_s[0] <= FC.GPU_FACTOR and 0 < r.worst_m[0] <= FC.GPU_FACTOR


# ---- 1. the fix table ------------------------------------------------------------------------------------------------------------------
def test_the_fix_table_against_the_joint_pose_witness():
    """Every case of the fix table in one fleet without a map, every submit with fixes (k_fleet_step_fix): lists, n, flags, exact
    symmetry and the bound against the JOINT pose witness behind both scans.  The same run without the fixes (k_fleet_step) leaves
    other bits in every member: the fixes did count."""
    cases = NC.fix_cases()
    r = left("fix")
    report("fix cases", r, len(cases))
    bare = lockstep("fix", with_fix=False)
    for i, c in enumerate(cases):
        assert len(c.expect[0][0]) > 0 and not FC.same_bits(r.bits[0][i], bare.bits[0][i]), (c.name, "the fix moved nothing")
        assert r.bits[0][i][0].shape == bare.bits[0][i][0].shape, c.name
    assert (r.n == bare.n).all()


# ---- 2. the map table ------------------------------------------------------------------------------------------------------------------
def test_the_map_table_against_the_map_witness():
    """Every case of the map table in one fleet on the standard map (k_fleet_step_map): fleet_map_cases.check_member behind both
    scans -- the three lists (every member on the map has map pairs in both records), n, flags, symmetry, the bound.  Without the
    fixes the members that had one hold other bits."""
    cases = NC.map_cases()
    assert {c.max_landmarks for c in cases} == {128} and all(len(c.expect[k][1]) >= 1 for c in cases if c.use for k in (0, 1))
    r = left("map")
    report("map cases", r, len(cases))
    bare = lockstep("map", with_fix=False)
    for i, c in enumerate(cases):
        assert FC.same_bits(r.bits[0][i], bare.bits[0][i]) == (not c.fixed), (c.name, "a fix moves the state, and nothing else does")


# ---- 3. the plain sweep through the other three compiles ---------------------------------------------------------------------------------
_plain = None


def plain_sweep():
    """fleet_cases.sweep_cases() in a default fleet (k_fleet_step): the bits, lists, n and flags behind each tick, and the longdouble
    witness's state behind each scan; once."""
    global _plain
    if _plain is None:
        cases = FC.sweep_cases()
        out = NS(bits=[], lists=[], n=[], flags=[], refs=[])
        fl = H.make_fleet(cases)
        try:
            for k in range(2):
                fl.submit(tick(cases, k))
                out.bits.append([FC.state_bits(fl, i) for i in range(len(cases))])
                out.lists.append([H.norm_match(fl.last_match(i)) for i in range(len(cases))])
                out.n.append(fl.n().copy())
                out.flags.append(fl.flags().copy())
        finally:
            fl.close()
        for c in cases:
            w = FC.witness_of(c)
            per = []
            for ev in FC.reference_events(c):
                FC.feed(w, ev)
                per.append(w.state())
            out.refs.append(per)
        _plain = out
    return _plain


@pytest.mark.parametrize("compile_", ["fix", "map", "track"])
def test_the_plain_sweep_through_the_other_compiles(compile_):
    """The 117 shapes that found k_fleet_step's own edge cases, beside one member with a fix in each submit (k_fleet_step_fix),
    beside one member on the map (k_fleet_step_map), and in a tracked fleet (k_fleet_step_track): behind each tick every member is
    within fleet_cases.SUITE's bound of the witness and holds the bits, lists, n and flags a default fleet leaves under k_fleet_step."""
    cases, plain = FC.sweep_cases(), plain_sweep()
    assert len(cases) == 117 and all(len(c.events) == 2 for c in cases)
    extra = {"fix": NC.fix_cases()[10], "map": next(c for c in NC.map_cases() if c.table == "map" and not c.fixed and c.NSn and c.N2), "track": None}[compile_]
    off = 0 if extra is None else 1
    fl = H.make_fleet(([extra] if off else []) + cases)
    worst_s, worst_m = (0.0, ""), (0.0, "")
    try:
        if compile_ == "map":
            fl.set_map(*WC.std_map(), members=[0])
        if compile_ == "track":
            fl.track(True)
        for k in range(2):
            fl.submit(([FC.fev(0, extra.events[k])] if off else []) + [FC.fev(off + i, c.events[k]) for i, c in enumerate(cases)])
            # what can be seen of the compile: the extra member's fix or map pairs took part
            if compile_ == "fix":
                assert extra.events[k][4] is not None
                H.check_member(fl, 0, extra, k, witness_at(NC.fix_runs(), extra, k), NC.FIX_SUITE)
            if compile_ == "map":
                assert len(extra.expect[k][1]) >= 1
                FM.check_member(fl, 0, extra, k, witness_at(NC.map_runs(), extra, k), NC.MAP_SUITE)
            for i, c in enumerate(cases):
                fs, fm = H.check_member(fl, off + i, c, k, NS(state=lambda i=i, k=k: plain.refs[i][k]), FC.SUITE)
                worst_s, worst_m = max(worst_s, (fs, f"{c.name} scan {k}")), max(worst_m, (fm, f"{c.name} scan {k}"))
                assert FC.same_bits(FC.state_bits(fl, off + i), plain.bits[k][i]), (compile_, c.name, k, "other bits than under k_fleet_step")
                got = H.norm_match(fl.last_match(off + i))
                assert all(np.array_equal(a, b) for a, b in zip(got, plain.lists[k][i])), (compile_, c.name, k)
            assert (fl.n()[off:] == plain.n[k]).all() and (fl.flags()[off:] == plain.flags[k]).all()
        if compile_ == "track":
            for i, tr in enumerate(fl.take_track()):
                assert tr.kind.tolist() == [FC.EV_SCAN, FC.EV_SCAN] and TC.last_record_is_the_slot(fl, tr, i), cases[i].name
                assert (tr.n_state[0], tr.n_new[0]) == tuple(len(x) for x in cases[i].expect[0]) and tr.n_map[0] == 0, cases[i].name
    finally:
        fl.close()
    print(f"\nplain sweep under the {compile_} compile: sigma {worst_s[0]:.2f} x the floor at {worst_s[1]}; mu {worst_m[0]:.2f} x at {worst_m[1]}")
    assert 0 < worst_s[0] <= FC.GPU_FACTOR and 0 < worst_m[0] <= FC.GPU_FACTOR


# ---- 4. both tables in tracked fleets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fix", "map"])
def test_the_tables_in_tracked_fleets(which):
    """k_fleet_step_track on the table's shapes: every record of a tracked fleet fed one submit per tick is what an UNTRACKED twin
    holds behind the same message given alone (bit for bit), the last record is the slot, the final states are the bits the untracked
    lockstep run left, and both ticks in ONE tracked submit give the same records and bits again."""
    t = TABLES[which]
    cases, ref = t.cases(), left(which)
    fl, tw, one = t.fleet(cases, track=True), t.fleet(cases), t.fleet(cases, track=True)
    try:
        want = TC.twin_records(tw, [(m, c.events[k]) for k in range(2) for m, c in enumerate(cases)])
        for k in range(2):
            fl.submit(tick(cases, k))
        one.submit(tick(cases, 0) + tick(cases, 1))
        for f in (fl, one):
            tracks = f.take_track()
            for m, c in enumerate(cases):
                TC.assert_records(tracks[m], want[m], c.name)
                assert tracks[m].kind.tolist() == [FC.EV_SCAN, FC.EV_SCAN] and tracks[m].K[0] == len(c.events[0][3]), c.name
                lens = tuple(len(x) for x in c.expect[0])
                assert (tracks[m].n_state[0], tracks[m].n_map[0], tracks[m].n_new[0]) == (lens if len(lens) == 3 else (lens[0], 0, lens[1])), c.name
                assert TC.last_record_is_the_slot(f, tracks[m], m), c.name
                assert FC.same_bits(FC.state_bits(f, m), ref.bits[1][m]), (c.name, "other bits than the untracked run left")
            assert (f.n() == ref.n).all() and (f.flags() == ref.flags).all()
        for m, c in enumerate(cases):
            assert FC.same_bits(FC.state_bits(tw, m), ref.bits[1][m]), (c.name, "the twin, one message per submit")
    finally:
        for f in (fl, tw, one):
            f.close()


# ---- 5. other call patterns ------------------------------------------------------------------------------------------------------------
def test_map_members_in_other_call_patterns():
    """Eight members of the map table, one per n mod 16, four with a fix: alone at index 0, among the others in reversed order, and
    with both scans in one submit -- the bits the table's lockstep run left, each time."""
    members = NC.pattern_members()
    index = {c.name: i for i, c in enumerate(NC.map_cases())}
    ref = left("map")
    want = [ref.bits[1][index[c.name]] for c in members]

    def same(fl, i, c, how):
        assert FC.same_bits(FC.state_bits(fl, i), want[members.index(c)]), (c.name, how)
        got = H.norm_match(fl.last_match(i))
        assert all(np.array_equal(a, b) for a, b in zip(got, FM.want_lists(c, 1))), (c.name, how)

    for c in members:
        fl = map_fleet([c])
        try:
            for k in range(2):
                fl.submit([FC.fev(0, c.events[k])])
            same(fl, 0, c, "alone at index 0")
        finally:
            fl.close()
    rev = members[::-1]
    fl = map_fleet(rev)
    try:
        for k in range(2):
            fl.submit(tick(rev, k)[::-1])
        for i, c in enumerate(rev):
            same(fl, i, c, "reversed")
    finally:
        fl.close()
    fl = map_fleet(members)
    try:
        fl.submit(tick(members, 0) + tick(members, 1))
        for i, c in enumerate(members):
            same(fl, i, c, "both scans in one submit")
    finally:
        fl.close()
