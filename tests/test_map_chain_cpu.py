"""MapBuilder::AddRangeData's composition without a GPU: reflector_ekf_slam_amd.map_builder.MapBuilder runs over the CPU oracle behind a
recorder (tests/map_chain_cases.py), and every recorded decision is held to tests/witness/map_builder_witness.py, every recorded stage
result to the stage witnesses on the recorded inputs.  The chains reach what they are named after, the measured floors and the
share of the transform bound agree with what the cases module records, and every planted defect of the composition is seen."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import map_chain_cases as MC
from tests.witness import map_builder_witness as MW


@pytest.fixture(scope="module")
def recorded(oracle_lib):
    from tests.oracle_front_end import OracleFrontEnd
    return {ch.name: (ch, MC.run_chain(ch, OracleFrontEnd())) for ch in MC.chains()}


def _scans(recorded):
    for name, (ch, recs) in recorded.items():
        for k, rec in enumerate(recs):
            yield ch, k, rec


TRANSFORMS = ("align_returns", "align_misses", "insert_origin", "insert_returns", "insert_misses", "in_local_origin", "in_local_returns",
              "in_local_misses")


def test_every_decision_and_every_stage_of_every_scan_holds(recorded):
    floors, ratio, off, matched = [0.0, 0.0, 0.0], 0.0, 0, 0
    for ch, k, rec in _scans(recorded):
        comp = MC.composition(rec, ch)
        st, fig = MC.stages(("cpu", ch.name, k), rec, ch)
        assert MC.holds(comp) == [] and MC.holds(st) == [], (ch.name, k, MC.holds(comp), MC.holds(st), fig)
        ratio = max([ratio] + [comp[n] for n in TRANSFORMS if n in comp])
        if fig.refine is not None:
            floors = [max(a, b) for a, b in zip(floors, fig.refine)]
            matched, off = matched + 1, off + bool(fig.off_centre)
            assert fig.margin >= MC.MARGIN and fig.refine[0] <= MC.STABLE_POSE                     # every scan, none skipped
    print(f"refinement floors over {matched} matched scans: pose {floors[0]:.2e} initial {floors[1]:.2e} final {floors[2]:.2e}")
    print(f"largest share of the transform bound: {ratio:.3f}")
    print(f"best candidate off the window's centre: {off} of {matched}")
    assert all(f <= r <= 10 * f for f, r in zip(floors, MC.FLOORS)), (floors, MC.FLOORS)          # as recorded, rounded up
    assert ratio <= MC.BOUND_RATIO <= 2 * ratio
    assert 2 * off >= matched >= 12                                                               # the EKF noise moves the match
    assert MW.K == 10.0 and MC.GPU_FACTOR == 16.0


def test_chains_reach_what_they_are_named_after(recorded):
    from reflector_ekf_slam_amd.map_builder import yaw_of_quaternion_f32
    chains = [ch for ch, _ in recorded.values()]
    assert len(chains) == 8 and {ch.origin for ch in chains} == {(0.0, 0.0), (0.3, -0.2), (2.5, 1.0)}
    assert {ch.resolution for ch in chains} == {0.05, 0.1, 0.03}
    starts = {c[0]: c[5][2] for c in MC.CHAINS}
    assert {starts["control"], starts["quarter"], starts["minus_quarter"], starts["near_pi"], starts["near_minus_pi"]} == {0.0, math.pi / 2, -math.pi / 2, 3.1, -3.1}
    beyond = [s.true[2] for s in recorded["beyond_pi"][0].scans]
    assert beyond == [3.5, -4.0] and all(abs(s.ekf_pose[2]) > math.pi for s in recorded["beyond_pi"][0].scans)
    paths, crossed, sizes, two_yaws = set(), 0, set(), 0
    for ch, k, rec in _scans(recorded):
        scan = rec.scan
        assert scan.rd.returns.shape[0] <= MC.MAX_RETURNS and scan.rd.misses.shape[0] <= MC.MAX_MISSES
        w = MC.stage_witness(("cpu", ch.name, k), rec, ch)
        if rec.result is None:
            continue
        assert w.path[0] == ch.path, (ch.name, k, w.path)
        limits = rec.state_after[1]
        sizes.add(limits[:2])
        assert limits[2] == float(np.float32(ch.resolution)) != ch.resolution                  # the float32 cast shows
        if "Match" in rec.calls:
            paths.add(w.path[0])
            est, theta = rec.calls["RefineMatch"].result.pose_estimate, scan.ekf_pose[2]
            crossed += abs(theta) <= math.pi < abs(est[2] + theta)
            # range_data_in_local's yaw (the double product, cast) and in_local2's (the float32 half angle) are different floats
            aw, az, qw, qz = math.cos(0.5 * est[2]), math.sin(0.5 * est[2]), math.cos(theta / 2), math.sin(theta / 2)
            ha = np.float32(np.float32(0.5) * np.float32(est[2]))
            two_yaws += yaw_of_quaternion_f32(aw * qw - az * qz, aw * qz + az * qw) != yaw_of_quaternion_f32(math.cos(float(ha)), math.sin(float(ha)))
        else:
            cells, res, max_xy = rec.calls["SetGrid"].args
            assert rec.calls["Insert"].before[1][:2] == (100, 100) and (limits[0] > 100 or ch.resolution >= 0.1)  # outgrown by the first scan
            # the maxima show the float32 resolution: with the double one they would differ
            origin = rec.calls["Insert"].args[0].astype(np.float64)
            assert max_xy == (origin[0] + 50 * res, origin[1] + 50 * res)
            assert max_xy != (origin[0] + 50 * ch.resolution, origin[1] + 50 * ch.resolution)
    assert paths == {"sparse", "first", "ladder"} and crossed >= 1 and two_yaws >= 1
    assert (200, 200) in sizes and max(max(s) for s in sizes) <= 400
    first = recorded["control"][1][0]
    assert first.calls["Insert"].before[1][:2] == (100, 100) and first.state_after[1][:2] == (200, 200)
    # the outcomes: nothing left behind the gate first (no grid is made) and later (nothing changes), no returns, no misses
    ch, recs = recorded["outcomes"]
    assert [r.scan.kind for r in recs] == list("fesfes") and [r.result is None for r in recs] == [True, True, False, True, True, False]
    assert recs[0].state_after is None and recs[1].state_after is None and recs[1].order == []
    assert recs[3].order == ["VoxelFilter", "VoxelFilter", "AdaptiveVoxelFilter"] and recs[3].calls["AdaptiveVoxelFilter"].result.shape[0] == 0
    assert recs[3].state_after is recs[3].state_before and recs[3].count_after == recs[3].count_before == 1
    assert any(r.scan.kind == "n" and r.result is not None and r.calls["Insert"].args[2].shape[0] == 0 for _, _, r in _scans(recorded))
    assert recs[4].scan.rd.misses.shape[0] > 0 and recs[4].scan.rd.returns.shape[0] == 0


# MEASURED: the first (chain, scan, decision) that sees each planted defect
CAUGHT_BY = {
    "rotation_by_minus_yaw": ("quarter", 0, "align_returns"),
    "origin_not_rotated": ("quarter", 0, "insert_origin"),
    "origin_not_translated": ("control", 0, "insert_origin"),
    "in_local_from_filtered": ("control", 0, "in_local_returns"),
    "insert_raw_returns": ("control", 0, "insert_returns"),
    "insert_adaptive_cloud": ("minus_quarter", 0, "insert_returns"),
    "match_voxel_cloud": ("minus_quarter", 1, "match_cloud"),
    "refine_target_coarse": ("control", 1, "refine_target"),
    "prediction_keeps_theta": ("quarter", 0, "insert_origin"),
    "local_pose_without_alignment": ("quarter", 0, "local_pose"),
    "grid_on_aligned_origin": ("control", 0, "grid_created"),
    "grid_without_half_extent": ("control", 0, "grid_created"),
    "grid_float64_resolution": ("control", 0, "grid_created"),
}
DISPLACEMENT = 1000.0                 # a defect that is seen through a bound is seen by at least this many bounds


def test_every_planted_defect_of_the_composition_is_seen(recorded):
    """A defect counts as seen by a scan when a truth value turns false or a number reaches DISPLACEMENT bounds; a scan on which it
    moves something by less (a yaw within a hair of pi, where -yaw is nearly yaw) is no catch.  Every defect has a catch."""
    assert set(CAUGHT_BY) == set(MW.MUTANTS)
    first, smallest = {}, {}
    for mutant in MW.MUTANTS:
        catches, marginal = [], 0
        for ch, k, rec in _scans(recorded):
            comp = MC.composition(rec, ch, mutant)
            seen = [(n, math.inf if comp[n] is False else comp[n]) for n in MC.holds(comp)]
            strong = [(n, v) for n, v in seen if v >= DISPLACEMENT]
            marginal += bool(seen) and not strong
            if strong:
                catches.append((ch.name, k, strong[0][0], max(v for _, v in strong)))
        assert catches, mutant
        first[mutant], smallest[mutant] = catches[0][:3], min(c[3] for c in catches)
        print(f"mutant {mutant}: first seen by {first[mutant]}, on {len(catches)} scans, by {smallest[mutant]:.3g} bounds at least; {marginal} marginal")
    assert min(smallest.values()) >= DISPLACEMENT
    assert first == CAUGHT_BY
