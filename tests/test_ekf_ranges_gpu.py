"""dd_body (csrc/ekf_kernels.hip) on ranges of more than one tile, in each of its three places -- alone (k_downdate2), beside the
next scan's front end (k_dd_front) and as the queue-fed role inside k_mid -- against the longdouble witness
(tests/witness/fleet_witness.py) on the dense SPD states of tests/ekf_range_cases.py.  The shape sweep
(tests/test_ekf_shapes_gpu.py) hands every workgroup one tile; here the state size is chosen, from the device's CU count and the
restated schedule (tests/downdate_schedule.py), as the smallest at which the static schedule has each range form: sub = 1 with
ranges of 2 and of 3 tiles, sub = 2 with ranges of 3, 4 (the last straight-line form) and 5 (the first trip of the generic
loop), k-chunks 16, 32, 48 and 64 on ranges of 2, and a growing filter at a size with ranges of 3.  tests/test_ekf_ranges_cpu.py
plants six defects of a multi-tile range and shows each at more than 10^6 x the bound used here.

Each case runs from a fresh handle in four of the call patterns of tests/test_ekf_shapes_gpu.py (run_pattern, _check_state and
_counters are its own), one handle alive at a time:
    reader                 the state is read after scan 1: its downdate runs alone (k_downdate2), scan 2's at the final read
    pipelined_two_launch   scan 1's downdate beside scan 2's front end (k_dd_front, K workgroups fewer in the schedule)
    pipelined              scan 1's downdate as the queue-fed role of scan 2's launch (runs of three tiles, sub = 2)
    pipelined_spec_off     the same with REKF_SPEC=0
Association lists, n, flags and sync_code() are the case's; sigma is exactly symmetric as returned; sigma and mu are within
fleet_cases.GPU_FACTOR (16) x the FP64 floor recorded in tests/ekf_range_cases.py and never looser than 1e-9 / 1e-11.  The
three pipelined patterns end on the same bits -- the queue hands out other ranges than the static schedule, and the sweep
already requires this identity at one tile per workgroup, so a difference is a defect of a range form: the failure names the
tiles whose bits differ and the workgroup of the static schedule that held them.  Counters: [24] > 0 (the one-launch form ran) for
pipelined and pipelined_spec_off, [24] == 0 for pipelined_two_launch, [22] == 1 for the scan that met a pending downdate; on the
growing case scan 1 appends reflectors, its k_augment is pending with its downdate, and scan 2 takes the two-launch chain in every
pattern ([24] == 0, [22] == 0).  Where the restatement gives the queue role more items than workgroups (every form but
sub1_range2: 176 - 330 items for 128 - 80 workgroups on 256 CUs, and [24] = items + workgroups says so) some workgroup takes a second item (the `again` barrier); at
T = 23 the role has a workgroup for each of its 100 items.

Measured on an MI355X (256 CUs; T = 23, 31, 32, 38, 43, n = 1409 ... 2689): 46 tests in 28 s.  The first pattern of a case
(reader) builds the case and computes the witness, 1.3 - 3.5 s (3.5 s at n = 2689); every further pattern 0.2 - 0.6 s; the
comparison 0.1 s.  Worst sigma error 0.56 x the FP64 floor, worst mu error 0.92 x (both the growing case, scan 2, reader); among
the full filters sigma stays below 0.5 x.  Every pattern of every case ends on the same bits; [24] = 200, 304, 315, 364, 410 =
items + workgroups as restated.  No kernel defect found.
"""
from __future__ import annotations

import time

import numpy as np
import pytest

from tests import downdate_schedule as DS
from tests import ekf_range_cases as RC
from tests import fleet_cases as FC
from tests import test_ekf_shapes_gpu as SG
from tests.witness import fleet_witness as FW

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not FW.available(), reason="numpy.longdouble has no 64-bit mantissa here")]

PATTERNS = ("reader", "pipelined_two_launch", "pipelined", "pipelined_spec_off")
SLOTS = ("sub1_range2", "sub1_range3", "sub2_range3", "sub2_range4", "sub2_range5", "sub1_range2_K16", "sub1_range2_K24", "sub1_range2_K32", "grow")
_runs = {}                                                       # the current case's runs, by pattern (one case's states at a time)


_n_cu = []


def n_cu():
    """multiProcessorCount of the current device, asked of the HIP runtime the library itself has loaded (the figure
    launch_downdate_any and rekf_launch_scan plan with).  No second runtime is brought into the process for it."""
    if not _n_cu:
        import ctypes as C
        from reflector_ekf_slam_amd import _lib
        _lib.rekf()
        with open("/proc/self/maps") as f:
            paths = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln and "/torch/" not in ln})
        assert len(paths) == 1, paths
        hip = C.CDLL(paths[0])
        dev, cu = C.c_int(-1), C.c_int(0)
        HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63              # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h; the enum is ABI)
        assert hip.hipGetDevice(C.byref(dev)) == 0 and dev.value >= 0
        assert hip.hipDeviceGetAttribute(C.byref(cu), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, dev.value) == 0
        assert 8 <= cu.value <= 1024, cu.value
        _n_cu.append(int(cu.value))
    return _n_cu[0]


def _case(slot):
    """The case of a slot for THIS device's CU count: T comes from the same search as the pinned table (a form that no L <= 1500
    reaches is an assertion of ekf_range_cases.specs, not a skip)."""
    names = RC.names(n_cu())
    assert len(names) == len(SLOTS)
    return RC.case_named(names[SLOTS.index(slot)], n_cu())


def _run(case, pattern, monkeypatch):
    if _runs.get("case") != case.name:
        _runs.clear()
        _runs["case"] = case.name
    if pattern not in _runs:
        t0 = time.perf_counter()
        _runs[pattern] = SG.run_pattern(case, pattern, monkeypatch, RC.SUITE)
        print(f"  {case.name} {pattern}: {time.perf_counter() - t0:.2f} s")
    return _runs[pattern]


def _differing_tiles(case, a, b):
    """The 64 x 64 tiles of the lower triangle whose bits differ between two final states, with the workgroup of scan 1's static
    schedule (k_dd_front) that held each."""
    d = a.sigma != b.sigma
    T = DS.tiles_of(a.sigma.shape[0])
    out = []
    for I in range(T):
        for J in range(I + 1):
            if d[64 * I: 64 * I + 64, 64 * J: 64 * J + 64].any():
                blk, pos, tl = DS.holder(T, case.slots_front, (I, J))
                out.append(f"tile ({I}, {J}): workgroup {blk}, position {pos} of {tl}")
    return out


def _agree(case, runs):
    """The three pipelined patterns end on the same bits, and the counters show which form carried scan 1's downdate."""
    p4, p5, p6 = runs["pipelined"], runs["pipelined_spec_off"], runs["pipelined_two_launch"]
    for other, what in ((p5, "REKF_SPEC=0"), (p6, "REKF_SCAN_LAUNCH=0 (k_dd_front, the static ranges)")):
        if not SG._same_bits(p4, other):
            tiles = _differing_tiles(case, p4, other)
            pytest.fail(f"{case.name}: {what} ends on other bits than the pipelined run (the queue's runs of three): mu differs: "
                        f"{not np.array_equal(p4.mu, other.mu)}; {len(tiles)} tiles differ: " + "; ".join(tiles[:12]))
    line = "; ".join(f"{p} " + " ".join(f"[{i}] {runs[p].cnt[i]}" for i in (18, 20, 22, 23, 24)) for p in PATTERNS)
    print(f"  {case.name}: {line}; queue role: {case.role_items} items for {case.role_wgs} workgroups; k_downdate2 {case.form_alone}, "
          f"k_dd_front {case.form_front}")
    assert p6.cnt[24] == 0 and p6.cnt[22] == 0 and runs["reader"].cnt[24] == 0, line
    if case.kind == "range_grow" or not case.one_launch_fits:
        # scan 1's k_augment is pending with its downdate (or the role would be left too few CUs): the two-launch chain
        assert p4.cnt[24] == 0 and p5.cnt[24] == 0 and p4.cnt[22] == 0 and p5.cnt[22] == 0, line
    else:
        assert p4.cnt[24] > 0 and p5.cnt[24] > 0 and p4.cnt[22] == 1 and p5.cnt[22] == 1, line
        # every role workgroup asks the queue until it is handed a number past the last item: [24] is items + workgroups, as restated.
        # More items than workgroups: some workgroup took a second item (the smallest form has a workgroup per item).
        assert p4.cnt[24] == p5.cnt[24] == case.role_items + case.role_wgs, (line, case.role_items, case.role_wgs)
        assert case.second_item == (case.role_items > case.role_wgs) and (case.second_item or case.form == "sub1_range2"), line


@pytest.mark.parametrize("slot,step", [(s, p) for s in SLOTS for p in PATTERNS + ("agree",)])
def test_range_form(slot, step, monkeypatch):
    """One case in one call pattern: lists, n, flags, sync code, exact symmetry and the bound (run_pattern checks them); step
    `agree`: the patterns' final bits and counters against each other (it runs whichever pattern has not run yet)."""
    case = _case(slot)
    if slot != "grow" and "_K" not in slot:
        assert case.form_alone == slot and DS.form_of(case.T, DS.slots_of(n_cu(), 0)) == slot
    if step != "agree":
        _run(case, step, monkeypatch)
    else:
        _agree(case, {p: _run(case, p, monkeypatch) for p in PATTERNS})


def test_worst_multiples_of_the_floor():
    """Reports what the tests above measured (run the module with -s)."""
    ws, wm = SG.WORST.get(RC.SUITE.name, ((0.0, ""), (0.0, "")))
    print(f"\nrange cases on {n_cu()} CUs {RC.table(n_cu())}: worst sigma error {ws[0]:.2f} x the FP64 floor ({ws[1]}), worst mu error "
          f"{wm[0]:.2f} x ({wm[1]}); the bound is {FC.GPU_FACTOR:.0f} x")
    assert ws[0] <= FC.GPU_FACTOR and wm[0] <= FC.GPU_FACTOR
    _runs.clear()
