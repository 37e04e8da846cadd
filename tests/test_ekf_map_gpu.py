"""The single filter on a pre-loaded map (set_map) in every launch form, against the longdouble witness with the map branch
(tests/witness/fleet_map_witness.py) on the cases of tests/ekf_map_cases.py: dense SPD states written with set_state, map rows at
the 16-row and 64-row edges, beside state rows in one block step, with a pose fix, with duplicate rows, under rotated and
non-symmetric weights.  tests/test_ekf_map_cpu.py shows that the bound fails on the planted defects.

Each case runs from a fresh handle in the six call patterns of tests/test_ekf_shapes_gpu.py (run_pattern; one handle alive at a
time).  All three lists of last_match(), n, flags and sync_code() must be the witness's / the case's; sigma as returned exactly
symmetric; both relative errors within fleet_cases.GPU_FACTOR (16) x the FP64 floor that tests/test_ekf_map_cpu.py measures, never
looser than the suite's absolute tolerances.  The three pipelined forms end on the same bits, and so do the two readers.
rekf_debug_counters is read once per run (`_check_counters` says what the host's rules in rekf_api.hip make of each kind).

The cases of the fleet's map (tests/fleet_map_cases.py: map sizes at the wave sweep's edges, exact ties, the order of the branches,
the gate, weights, fixes) run through a single handle in the reader pattern with that module's floors; its nan cases (a NaN
weighted distance never wins) additionally without the match grid and pipelined.  KNOWN_DIVERGENCES lists, by case and call
pattern, where the single filter's map_match_wave does not follow the NaN rule yet (DESIGN.md, quirk register)."""
from __future__ import annotations

import pytest

from tests import ekf_map_cases as XC
from tests import fleet_cases as FC
from tests import fleet_map_cases as MC
from tests import test_ekf_shapes_gpu as SG
from tests.test_ekf_shapes_gpu import PATTERNS, run_pattern
from tests.witness import fleet_map_witness as MW

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not MW.available(), reason="numpy.longdouble has no 64-bit mantissa here")]


def _check_counters(case, runs):
    """rekf_debug_counters after each pattern ([18] scans k_mid matched itself through the match grid; [20] scans whose speculative
    record was taken; [22] scans that met a pending downdate, [23] of those, the ones that computed its correction themselves;
    [24] > 0: the one-launch form ran).  What is asserted follows from the host's rules by reading; the rest is printed."""
    c = {p: r.cnt for p, r in runs.items()}
    line = "; ".join(f"{p} " + " ".join(f"[{i}] {c[p][i]}" for i in (18, 20, 21, 22, 23, 24)) for p in runs)
    print(f"  {case.name}: {line}")
    blocks = [XC.block_steps(case, k) is not None for k in range(len(case.events))]
    staged = [len(ev[3]) > 64 for ev in case.events]
    p4, p5, p6 = c["pipelined"], c["pipelined_spec_off"], c["pipelined_two_launch"]
    # the knobs: REKF_SCAN_LAUNCH=0 has no one-launch form, hence no speculation and no scan that meets a pending downdate;
    # REKF_SPEC=0 takes no speculative record; without the match grid k_mid matches no scan itself
    assert p6[24] == 0 and p6[20] == 0 and p6[22] == 0 and p5[20] == 0 and c["reader_grid_off"][18] == 0, line
    full = case.cap == case.L
    if all(blocks):
        assert p4[24] == 0 and p4[22] == 0 and p4[20] == 0 and p5[24] == 0, line     # (65 rows with a fix: every scan in block steps)
    elif case.kind == "wide":
        # as for the wide scans without a map: scan 2 (a whole scan) takes scan 1's last downdate along as a role of its own launch,
        # and there is no panel of a wide scan (a miss) -- unless scan 1 was staged through HBM, whose downdate is not held back
        if staged[0]:
            assert p4[24] == 0 and p4[22] == 0 and p5[24] == 0, line
        else:
            assert p4[24] > 0 and p4[22] == 1 and p4[23] == 1 and p5[24] > 0 and p5[22] == 1, line
        assert p4[20] == 0, line                                   # (two scans: nothing to speculate for)
    elif getattr(case, "non_symmetric", False):
        assert p4[20] == 0, line                                   # holdable needs map_lip >= 0: such a map is never speculated for
    elif full and len(case.events) == 4:
        # the map does not switch the speculation off, nor the one-launch form: scans 2, 3 and 4 meet a pending downdate
        for p in (p4, p5):
            assert p[24] > 0 and p[22] == 3, line
        assert p4[20] >= 1, line
        if case.MM >= 1:
            # The write-ahead panel is keyed on the scan's REFLECTORS (RekfCtl::cp_uid: the distinct landmarks of the state pairs;
            # map pairs have no part in it): a hit at scan 2 (the same set), a miss at scan 3, and at scan 4 a hit only where its
            # three state observations are all of scan 3's set (MM = 1).  With no state pair at all (MM = 0) the key is empty on
            # both sides; what the update makes of that is printed, not asserted.
            hits = 1 + (1 if case.MM == 1 else 0)
            assert p4[23] == 3 - hits and p5[23] == 3 - hits, line
    # the match grid serves host-predicted whole scans, whatever the map: behind set_state (scan 1 of every pattern) and behind a
    # read of the state or the pose -- but not the scan whose front end rides in k_dd_front (the node's scan 2 behind an appending
    # scan 1).  (n = 3: a grid without a reflector -- printed, not asserted.)
    if case.kind != "pure":
        whole = sum(1 for b in blocks if not b)
        assert c["reader"][18] == whole and c["node"][18] == whole - (1 if case.N2 else 0), line
        assert p4[18] == p5[18] == p6[18] == (0 if blocks[0] else 1), line


def _run_case(case, monkeypatch):
    runs = {p: run_pattern(case, p, monkeypatch, XC.SUITE) for p in PATTERNS}
    assert SG._same_bits(runs["pipelined"], runs["pipelined_spec_off"]), f"{case.name}: REKF_SPEC=0 ends on other bits than the pipelined run"
    assert SG._same_bits(runs["pipelined"], runs["pipelined_two_launch"]), f"{case.name}: REKF_SCAN_LAUNCH=0 ends on other bits than the pipelined run"
    assert SG._same_bits(runs["reader"], runs["reader_grid_off"]), f"{case.name}: the reader without the match grid ends on other bits"
    _check_counters(case, runs)
    return runs


def _ids(kind):
    return [c.name for c in XC.cases() if c.kind == kind]


@pytest.mark.parametrize("name", _ids("mix"))
def test_map_and_state_rows_on_a_full_filter(name, monkeypatch):
    """NS state pairs and Mm map pairs in one launch: 64 rows of either kind, the NBR switch, n = 63 | 65, map rows only."""
    _run_case(XC.case_named(name), monkeypatch)


@pytest.mark.parametrize("name", _ids("pure"))
def test_pure_localisation(name, monkeypatch):
    """n = 3 on a handle of capacity 8: up to 64 map rows and nothing else; and the case that also maps (n = 3 -> 9)."""
    c = XC.case_named(name)
    runs = _run_case(c, monkeypatch)
    assert all(r.cap == XC.PURE_CAP for r in runs.values())


@pytest.mark.parametrize("name", _ids("growing"))
def test_growing_filter_with_map_rows(name, monkeypatch):
    """k_mid<*, 1> and k_augment with map rows in the same scan; new rows up to and across the 16-row (and 64-row) edge."""
    c = XC.case_named(name)
    runs = _run_case(c, monkeypatch)
    assert all(r.cap == c.cap for r in runs.values())


@pytest.mark.parametrize("name", _ids("wide"))
def test_wide_scans_with_map_pairs_in_block_steps(name, monkeypatch):
    """A step of one map pair alone, a step that holds the state | map boundary of the record, map-only steps, a staged scan."""
    _run_case(XC.case_named(name), monkeypatch)


@pytest.mark.parametrize("name", _ids("pose"))
def test_pose_fix_with_map_rows(name, monkeypatch):
    """31 | 33 rows, 63 rows in one pass, 65 rows in steps of 30 pairs with the fix on the last."""
    _run_case(XC.case_named(name), monkeypatch)


@pytest.mark.parametrize("name", _ids("weights"))
def test_weighted_map(name, monkeypatch):
    """Rotated anisotropic weights (map_lip = 2), and one non-symmetric weight (map_lip < 0: no speculation)."""
    _run_case(XC.case_named(name), monkeypatch)


# ---- the fleet's map cases through a single handle ----------------------------------------------------------------------------
NAN_PATTERNS = ("reader", "reader_grid_off", "pipelined")
# (case, pattern) -> why the single filter misses the check.  Known divergences, DESIGN.md section 6 and the quirk register (Q17):
# to be fixed by the next change that re-measures the profiles (csrc/ekf_kernels.hip and csrc/rekf_api.hip are pinned by
# profiles/MANIFEST.json).  Measured on the MI355X; every other (case, pattern) passes.
_NAN_WHY = ("map_match_wave (csrc/ekf_kernels.hip:314-331) seeds each lane of the wave sweep with its first candidate, NaN or not, and "
            "wave_argmin (:108-116) never replaces a NaN (`od < d` is false): {} -- the observation comes out as new, not as the map pair")
_NAN_LOST = {"nan_p0_q1": "lane 0, which decides for the wave, holds the NaN of point 0",
             "nan_p5_q69": "point 69 is lane 5's second candidate, behind the NaN of point 5",
             "nan_p5_q37": "lane 37's minimum reaches lane 0 only through lane 5 (xor 32), which holds the NaN of point 5",
             "nan_nearest_5_runner_up_69": "point 69 is lane 5's second candidate, behind the NaN of point 5"}
KNOWN_DIVERGENCES = {(name, p): _NAN_WHY.format(lost) for name, lost in _NAN_LOST.items() for p in NAN_PATTERNS}
KNOWN_DIVERGENCES[("fix_0_31", "reader")] = (
    "n = 3, 31 map pairs and a pose fix (65 rows): process_scan (csrc/rekf_api.hip:1019-1041) runs block steps of 30 pairs with the fix "
    "on the LAST step, behind the map rows that pin the pose -- the order that cost k_fleet_step_map 242 x the floor in mu until it "
    "took the fix first (DESIGN.md section 10): the supposed cause, by that analogy.  Measured: mu off by 1.08e-14 relative = 98 x the map suite's floor (bound 16 x); "
    "lists, n, flags and sigma hold")


def _nan_names():
    return [c.name for c in MC.nan_cases()]


def _params(names, patterns):
    out = []
    for name in names:
        for p in patterns:
            why = KNOWN_DIVERGENCES.get((name, p))
            out.append(pytest.param(name, p, id=f"{name}-{p}", marks=[pytest.mark.xfail(strict=True, reason=why)] if why else []))
    return out


def _fleet_layer_names():
    nan = set(_nan_names())
    return [c.name for c in MC.all_cases() if c.use and c.max_landmarks == 128 and c.name not in nan]


def test_the_fleet_layer_is_every_case_that_uses_the_map():
    names = _fleet_layer_names()
    assert len(names) >= 30 and len(_nan_names()) == 9 and all(c.use and c.max_landmarks == 128 for c in MC.nan_cases())
    assert set(names) | set(_nan_names()) == {c.name for c in MC.all_cases() if c.use and c.max_landmarks == 128}
    assert {n for n, _ in KNOWN_DIVERGENCES} <= set(names) | set(_nan_names())


@pytest.mark.parametrize("name, pattern", _params(_fleet_layer_names(), ("reader",)))
def test_fleet_map_cases_through_a_single_filter(name, pattern, monkeypatch):
    """Every case of tests/fleet_map_cases.py that uses the map on a capacity of 128 (the nan cases have their own test below)."""
    run_pattern(next(c for c in MC.all_cases() if c.name == name), pattern, monkeypatch, MC.SUITE)


def test_branch_order_cases_through_a_single_filter(monkeypatch):
    """The two cases with an observation inside BOTH gates (capacities 6 and 4: with room and full), which no dense case can have."""
    cases = [c for c in MC.branch_cases()]
    assert [c.max_landmarks for c in cases] == [6, 4]
    for c in cases:
        run_pattern(c, "reader", monkeypatch, MC.SUITE)


@pytest.mark.parametrize("name, pattern", _params(_nan_names(), NAN_PATTERNS))
def test_nan_cases_through_a_single_filter(name, pattern, monkeypatch):
    """A NaN weighted distance never wins: with last_match() after the scan (front_role), without the match grid, and unread (the
    launch behind set_state)."""
    c = next(c for c in MC.all_cases() if c.name == name)
    run_pattern(c, pattern, monkeypatch, MC.SUITE)


def test_worst_multiples_of_the_floor():
    """Reports what the tests above measured (run the module with -s); the figures are in DESIGN.md section 6."""
    for suite, (ws, wm) in SG.WORST.items():
        print(f"\n{suite} cases: worst sigma error {ws[0]:.2f} x the FP64 floor ({ws[1]}), worst mu error {wm[0]:.2f} x ({wm[1]}); "
              f"the bound is {FC.GPU_FACTOR:.0f} x")
        assert ws[0] <= FC.GPU_FACTOR and wm[0] <= FC.GPU_FACTOR
