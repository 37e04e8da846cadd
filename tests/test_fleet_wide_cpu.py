"""Fleet filter, wide scans, what can be checked without a GPU: the C ABI's additions, the cases of tests/fleet_wide_cases.py against
the CPU references, the measured FP64 floor, the block form of the witness against the joint form, the planted block-form defects,
and FleetNode(wide_scans=True) over the oracle backend."""
from __future__ import annotations

import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_wide_cases as WC
from tests.witness import fleet_wide_witness as WW

pytestmark = pytest.mark.skipif(not WW.available(), reason="numpy.longdouble has no 64-bit mantissa here")

WIDE_BENCH_SOURCES = ["include/rfleet.h", "reflector_ekf_slam_amd/csrc/fleet_dev.h", "reflector_ekf_slam_amd/csrc/fleet_host.h", "reflector_ekf_slam_amd/csrc/fleet_kernels.hip",
                      "reflector_ekf_slam_amd/csrc/fleet_wide.hip", "reflector_ekf_slam_amd/csrc/rfleet_api.hip", "reflector_ekf_slam_amd/fleet.py",
                      "scripts/fleet_wide_bench.py"]
WIDE_CALLS = ("rfleet_set_wide_scans", "rfleet_get_last_match_wide", "rfleet_wide_counts")


def test_header_declares_the_wide_calls_and_keeps_the_narrow_limits():
    text = open(H.HEADER).read()
    fleet = H.fleet_mod()
    for name in WIDE_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert int(re.search(r"#define\s+RFLEET_MAX_OBS_WIDE\s+(\d+)", text).group(1)) == fleet.MAX_OBS_WIDE == 256
    assert int(re.search(r"#define\s+RFLEET_MAX_OBS\s+(\d+)", text).group(1)) == fleet.MAX_OBS == 32
    assert int(re.search(r"#define\s+RFLEET_ABI_VERSION\s+(\d+)", text).group(1)) == fleet.RFLEET_ABI_VERSION == 2
    scope = text[text.index("Deliberately OUT OF SCOPE"):]
    scope = scope[:scope.index("\n *\n")]
    assert "wider than RFLEET_MAX_OBS" in scope and "rfleet_set_wide_scans" in scope and "RFLEET_MAX_OBS_WIDE" in scope


def test_library_exports_the_wide_calls():
    lib = H._lib()
    for name in WIDE_CALLS:
        assert hasattr(lib, name), name
    fleet = H.fleet_mod()
    assert fleet._wide_lib() is not None
    for name in ("wide_scans", "wide_counts"):
        assert callable(getattr(fleet.ReflectorEKFSLAMFleet, name))
    assert callable(fleet.FleetMember.wide_scans)


def test_null_handle_is_refused_before_any_hip_call():
    import ctypes as C
    lib = H.fleet_mod()._wide_lib()
    a, b = C.c_long(), C.c_long()
    n = C.c_int()
    assert lib.rfleet_set_wide_scans(None, 1) == -1
    assert lib.rfleet_wide_counts(None, C.byref(a), C.byref(b)) == -1
    assert lib.rfleet_get_last_match_wide(None, 0, 256, C.byref(n), None, C.byref(n), None, C.byref(n), None) == -1


def test_pack_takes_a_256_row_cloud():
    fleet = H.fleet_mod()
    cloud = np.arange(512, dtype=np.float64).reshape(256, 2)
    arr, count, keep = fleet.ReflectorEKFSLAMFleet.pack([fleet.scan_event(0, 1.0, cloud), fleet.odom_event(0, 1.1, 0.1, 0.0, 0.0)])
    assert count == 2 and arr[0].K == 256 == fleet.MAX_OBS_WIDE and arr[0].kind == fleet.EV_SCAN
    assert keep[0].dtype == np.float32 and keep[0].shape == (256, 2) and arr[0].xy == keep[0].ctypes.data


def test_the_cases_are_what_the_issue_lists():
    cases = {c.name: c for c in WC.all_cases()}
    mm = sorted(sum(WC.counts(c)[:2]) for c in cases.values() if c.name.startswith("wide_L128"))
    assert mm == [33, 63, 64, 65, 96, 97, 256]
    assert {c.model for c in cases.values() if c.name.startswith("wide_L128_MM")} == {FC.DIFF, FC.OMNI}
    assert [(len(c.events[0][3]), *WC.counts(c)) for c in cases.values() if c.name.startswith("wide1_")] == [(33, 32, 0, 1), (40, 31, 0, 9)]
    assert [(c.mu.shape[0], WC.counts(c)) for c in cases.values() if "tall" in c.name] == [(5, (40, 0, 0)), (7, (40, 0, 0))]
    assert WC.counts(cases["wide_new100_from_n3"]) == (0, 0, 100) and WC.counts(cases["wide_new140_capacity"]) == (0, 0, 128)
    assert WC.counts(cases["wide_new40_room1"]) == (0, 0, 1) and len(cases["wide_new40_room1"].events[0][3]) == 40
    assert any(WC.counts(c) == (33, 0, 33) for c in cases.values())
    assert [WC.counts(c) for c in cases.values() if c.name.startswith("wide_map")] == [(20, 20, 0), (32, 8, 0), (33, 7, 0), (0, 40, 0)]
    assert [(WC.counts(c), c.use, c.events[0][4] is not None) for c in cases.values() if "fix" in c.name] == \
        [((33, 0, 0), False, True), ((65, 0, 0), False, True), ((20, 20, 0), True, True), ((0, 0, 40), False, True)]
    for c in cases.values():
        assert len(c.events[0][3]) > 32 and len(c.events[0][3]) <= 256, c.name


def test_references_agree_on_every_case():
    """oracle/ekf_oracle.c, oracle/ekf_numpy.py, the joint witness and the block witnesses give the claimed lists on every scan
    (asserted inside), and every scan of every case has a state."""
    runs = WC.runs()
    for c in WC.all_cases():
        assert sorted(runs[c.name]) == list(range(len(c.events))), c.name


def test_fp64_floor():
    WC.measure_floor(WC.all_cases(), WC.runs())


def test_block_form_is_joint_form():
    """In longdouble the block form equals the joint form to round-off on every case (bound recorded in the witness's file)."""
    worst_s, worst_m = (0.0, ""), (0.0, "")
    for c in WC.all_cases():
        for k, (wits, *_rest) in WC.runs()[c.name].items():
            es, em = H.rel_err(*wits[1], *wits[0])
            worst_s, worst_m = max(worst_s, (es, f"{c.name} scan {k}")), max(worst_m, (em, f"{c.name} scan {k}"))
    print(f"\nblock form vs joint form, longdouble: sigma {worst_s[0]:.3e} at {worst_s[1]}; mu {worst_m[0]:.3e} at {worst_m[1]}")
    assert worst_s[0] <= WW.BLOCK_VS_JOINT_SIGMA and worst_m[0] <= WW.BLOCK_VS_JOINT_MU
    assert WW.BLOCK_VS_JOINT_SIGMA < WC.FP64_FLOOR_SIGMA / 100 and WW.BLOCK_VS_JOINT_MU < WC.FP64_FLOOR_MU / 10


# the cases on which each planted defect has to show (it may show on more)
DEFECT_CASES = {"no_correction": ("wide_L128_MM33_N0_diff", "wide_tall_L1_MM40"), "relinearise": ("wide_L128_MM97_N0_omni", "wide_tall_L2_MM40"),
                "drop_last_partial": ("wide_L128_MM33_N0_diff", "wide_L128_MM65_N0_omni"), "local_row_width": ("wide_map_NS20_NM20", "wide_map_NS33_NM7"),
                "wrap_every_block": ("wide_heading_across_pi",), "pose_in_loop": ("wide_fix_plain_MM33", "wide_fix_plain_MM65")}


@pytest.mark.parametrize("mutate", WW.WIDE_MUTATIONS)
def test_every_planted_defect_exceeds_the_gpu_bound(mutate):
    cases = {c.name: c for c in WC.all_cases()}
    caught = []
    for name in DEFECT_CASES[mutate]:
        c = cases[name]
        w = WC.block_witness_of(c)
        ev = FC.reference_events(c)[0]
        w.handle_observation(ev[1], ev[3], None if ev[4] is None else np.asarray(ev[4], np.float64), mutate=mutate)
        ref = WC.runs()[name][0][0][0]
        es, em = H.rel_err(*w.state(), *ref)
        bs, bm = H.bounds_within_tolerances(*ref, WC.SUITE)
        print(f"  {mutate} on {name}: sigma {es / bs:.3g} x the GPU bound, mu {em / bm:.3g} x")
        if es > bs or em > bm:
            caught.append(name)
    assert caught, mutate


def test_fleet_node_with_wide_scans_is_a_node(oracle_lib, tmp_path):
    """FleetNode(wide_scans=True) over the oracle backend on a trace with a 34-centre scan equals single oracle Nodes, exactly; the
    default FleetNode raises and makes no wide call."""
    from reflector_ekf_slam_amd import synth
    from reflector_ekf_slam_amd.node_replay import FleetNode, synth_dump
    from tests import oracle_fleet_node as OF
    from tests import oracle_fleet_wide as OW
    metas = [synth_dump(str(tmp_path / f"r{i}.npz"), synth.SessionConfig(f"w{i}", 40, 12, synth.DIFF, seed=31 + i), max_scans=2).meta
             for i in range(2)]
    msgs = OW.plate_messages()
    fn = FleetNode(metas, OW.wide_oracle_fleet_backend(), wide_scans=True)
    assert fn.fleet.wide
    assert fn.tick([], [(0, msgs[0]), (1, msgs[0])]) == []
    assert sorted(fn.tick([], [(0, msgs[1]), (1, msgs[1])])) == [0, 1]
    nodes = [OW.single_node(m, msgs) for m in metas]
    assert [c.shape[0] for _, c in fn.logs[0].observations] == [OW.PLATES] and fn.fleet.n()[0] == 3 + 2 * OW.PLATES
    assert OF.differences(fn, nodes) == []
    for m, node in enumerate(nodes):
        got, want = fn.fleet.get_state(m), node.slam.GetState()
        assert np.array_equal(got.mu, want.mu) and np.array_equal(got.sigma, want.sigma)
    plain = FleetNode(metas[:1], OF.oracle_fleet_backend())                       # (this backend has no wide_scans: none is called)
    plain.tick([], [(0, msgs[0])])
    with pytest.raises(ValueError) as e:
        plain.tick([], [(0, msgs[1])])
    assert str(OW.PLATES) in str(e.value)
    many = OW.plate_messages(plates=34)[1]
    assert "wide_scans" in FleetNode.__doc__ and "MAX_OBS_WIDE" in FleetNode.__doc__ and many is not None


def test_fleet_wide_bench_describes_the_tree():
    """profiles/fleet_wide_bench.json was measured on the fleet sources of this tree (SHA-256 by content), and its ratios are its legs'."""
    rec = json.load(open(os.path.join(H.ROOT, "profiles", "fleet_wide_bench.json")))
    sums = rec["_sources_sha256"]
    assert sorted(sums) == sorted(WIDE_BENCH_SOURCES)
    for rel in WIDE_BENCH_SOURCES:
        have = hashlib.sha256(open(os.path.join(H.ROOT, rel), "rb").read()).hexdigest()
        assert have == sums[rel], f"{rel} changed since profiles/fleet_wide_bench.json was measured: measure again (scripts/fleet_wide_bench.py)"
    assert sorted(rec["widths"]) == ["48", "96"] and rec["reps"] == 5
    for K, w in rec["widths"].items():
        assert w["blocks"] == (int(K) + 31) // 32 and sorted(w["fleet"]) == sorted(w["handles"]) == ["256", "4", "64"]
        for B in w["fleet"]:
            assert w["fleet_min_over_handles_max"][B] == w["fleet"][B]["min"] / w["handles"][B]["max"]
            assert w["fleet_is_a_speed_up_over_handles"][B] == (w["fleet"][B]["min"] > w["handles"][B]["max"])
            assert not w["fleet"][B]["flags_any"] and w["max_abs_mu_diff"][B] < 1e-9
