"""The voxel filters' witness without a GPU: the CPU oracle equals tests/witness/voxel_witness.py bit for bit on every case of
tests/voxel_cases.py, the witness takes the search paths written beside the cases, the cases reach the edges they are named after,
and every planted defect of the witness changes the result of a named case."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fleet_filter_scan_cases as FC
from tests import voxel_cases as VC
from tests.witness import voxel_witness as W

F32 = np.float32


class _Options:
    def __init__(self, values):
        self.max_length, self.min_num_points, self.max_range = values


def _gated(case):
    """The points the search sees: behind VoxelFilter(size) and the gate, by the witness."""
    return W.range_gate(VC.witness_of(case)[0], case.options[2])


def batches(label, ni):
    """Which round trips of the host's walk accept a candidate: the letters of a ladder trace, cut at the levels one round trip
    evaluates (5 for ni <= 4096, 3 for ni <= 8192, 2 above) -> a tuple of booleans, one per round trip."""
    depth = 5 if ni <= 4096 else (3 if ni <= 8192 else 2)
    trace = label[2]
    return tuple("A" in trace[k:k + depth] for k in range(0, len(trace), depth))


def test_oracle_equals_witness_on_every_cloud_and_the_labels_are_as_written(oracle_lib):
    worst = 0
    for c in VC.all_cases():
        fr, fm, av, label = VC.witness_of(c)
        want = FC.oracle_triple((c.returns, c.misses), c.size, _Options(c.options))
        assert FC.same_cloud(fr, want[0]) and FC.same_cloud(fm, want[1]) and FC.same_cloud(av, want[2]), (c.name, label)
        if c.label is not None:
            assert label == c.label, c.name
        worst = max(worst, c.returns.shape[0])
    assert worst == 12000 and len(VC.all_cases()) > 450
    # the stride and rounding families alone are 60 clouds, returns and misses
    assert sum((c.misses is not None) + 1 for c in VC.all_cases() if c.name.startswith(("stride/", "rounding/"))) >= 60


def test_reused_adaptive_cases_take_the_stated_paths_in_the_witness():
    got = [VC.witness_of(c)[3] for c in VC.all_cases() if c.name.startswith("adaptive/")]
    assert got == [path for *_, path in FC.ADAPTIVE] and len(got) == 11
    got = [VC.witness_of(c)[3][0] for c in VC.all_cases() if c.name.startswith("fraction/")]
    assert tuple(got) == FC.FRACTION_PATHS


def test_division_family_holds_points_that_the_two_divisions_put_in_different_voxels():
    for size in VC.DIVISION_SIZES:
        differ, halves = VC.division_points(size)
        a, b = W.cell_index(differ, size), W.cell_index(differ, size, "double_division")
        assert differ.shape[0] >= VC.DIVISION_MIN and (a != b).all() and (differ > 0).any() and (differ < 0).any(), size
        assert (np.abs(a - b) == 1).all()
    differ, halves = VC.division_points(VC.HALF_SIZE)
    q = (halves / F32(VC.HALF_SIZE)).astype(np.float64)
    assert halves.shape[0] == 8 and (np.abs(q) % 1 == 0.5).all() and (q > 0).sum() == 4 and (q < 0).sum() == 4
    assert np.array_equal(W.cell_index(halves, VC.HALF_SIZE), np.sign(q) * (np.floor(np.abs(q)) + 1))      # away from zero
    assert np.log2(float(F32(VC.HALF_SIZE))) % 1 != 0
    # the probes say where a special point went: exactly one of its two neighbours goes with it
    for c in VC.all_cases():
        if c.name.startswith("division/"):
            fr = VC.witness_of(c)[0]
            assert fr.shape[0] * 3 == c.returns.shape[0] * 2, c.name
            assert not FC.same_cloud(fr, W.voxel_filter(c.returns, c.size, "double_division")), c.name


def test_first_occurrence_cases_sit_on_the_block_borders_and_the_read_group():
    assert VC.FIRST_COUNTS == (255, 256, 257, 263, 264, 265, 511, 512, 513) and VC.SMALL_HANDLE % VC.GROUP != 0
    for n in VC.FIRST_COUNTS + (VC.SMALL_HANDLE,):
        by_kind = {c.name.split("/")[1]: c for c in VC.all_cases() if c.name.startswith("first/") and c.name.endswith(f"/{n}")}
        assert set(by_kind) == set(VC.FIRST_KINDS)
        for kind, c in by_kind.items():
            assert c.returns.shape[0] == n
            keys = W.keys_of(c.returns, c.size)
            pairs = VC.first_pairs(kind, n)
            for a, b in pairs:
                assert keys[a] == keys[b] and not np.array_equal(c.returns[a], c.returns[b]), (c.name, a, b)
            fr = VC.witness_of(c)[0]
            if kind == "one":
                assert len(set(keys)) == 1 and FC.same_cloud(fr, c.returns[:1])
            else:
                assert len(set(keys)) == n - len(pairs) and FC.same_cloud(fr, np.delete(c.returns, [b for _, b in pairs], 0)), c.name
        if n > VC.BLOCK:
            assert (VC.BLOCK - 1, VC.BLOCK) in VC.first_pairs("borders", n)
        if n > 2 * VC.BLOCK:
            assert (2 * VC.BLOCK - 1, 2 * VC.BLOCK) in VC.first_pairs("borders", n)
        a, b = VC.first_pairs("tail", n)[0]
        assert b == n - 1 and (a // VC.GROUP == b // VC.GROUP or (n - 1) % VC.GROUP == 0)
    assert any(n % VC.GROUP not in (0, 1) for n in VC.FIRST_COUNTS)                   # a partial group that holds a pair


def test_compaction_cases_keep_the_named_lanes_waves_and_tiles():
    assert VC.COMPACT_COUNTS == (1023, 1024, 1025, 2047, 2049)
    for c in VC.all_cases():
        if not c.name.startswith("compact/"):
            continue
        _, how, kind, n = c.name.split("/")
        keep = VC.compact_keep(kind, int(n))
        fr, _, av, label = VC.witness_of(c)
        got = fr if how == "v" else av
        assert label == ("sparse",) and FC.same_cloud(got, c.returns[keep]), c.name
        assert (fr.shape[0] < c.returns.shape[0]) == (how == "v" and not keep.all())    # (one tile keeps everything under "tiles")
    i = np.arange(2049)
    lanes, waves, tiles = (VC.compact_keep(k, 2049) for k in VC.COMPACT_KINDS)
    assert set(i[lanes] % VC.WAVE) == {0, VC.WAVE - 1}
    assert set(i[waves] % VC.TILE // VC.WAVE) == {0, VC.TILE // VC.WAVE - 1}
    assert tiles[:VC.TILE].all() and not tiles[VC.TILE:2 * VC.TILE].any() and tiles[2 * VC.TILE:].all() and tiles[2 * VC.TILE:].size == 1


def test_walk_cases_cover_every_size_class_and_every_pattern_of_two_batches():
    walk = [c for c in VC.all_cases() if c.name.startswith("walk/")]
    seen = {}
    for c in walk:
        ni, label = _gated(c).shape[0], VC.witness_of(c)[3]
        cls = 0 if ni <= 4096 else (1 if ni <= 8192 else 2)
        if label[0] == "ladder":
            seen.setdefault(cls, set()).add(batches(label, ni))
        removed = VC.witness_of(c)[0].shape[0] - ni                                  # points the gate removed in front
        seen.setdefault("ni", {})[ni] = max(removed, seen.get("ni", {}).get(ni, 0))
        seen.setdefault("labels", set()).add((cls, label[0]))
    for ni in (4096, 4097, 8192, 8193):
        assert seen["ni"].get(ni, 0) > 0, ni                                         # reached with points the gate removes
    assert 12000 in seen["ni"] and max(seen["ni"]) == 12000
    assert all(len(b) == 1 for b in seen[0])
    for cls in (1, 2):
        assert {(True, True), (True, False), (False, True), (False, False)} <= seen[cls], (cls, seen[cls])
    assert (2, "nothing") in seen["labels"] and (2, "first") in seen["labels"]
    assert {c.options[0] for c in walk} == {0.9, 5.0, 0.3}
    # 3- and 4-letter traces both occur, and a ladder has 7 rungs whatever max_length is
    assert {len(VC.witness_of(c)[3][2]) for c in walk if VC.witness_of(c)[3][0] == "ladder"} == {3, 4}


def test_ladder_has_seven_rungs_for_every_max_length_and_ge_never_differs_from_gt():
    """The planted defect `ladder_ge` cannot show: see voxel_cases.EQUIVALENT.  Shown here over many lengths instead."""
    rng = np.random.default_rng(3)
    lengths = np.concatenate([rng.uniform(1e-3, 100.0, 20000), np.array([0.9, 5.0, 0.3, 1.0, 0.5, 0.64, 1.28, 100.0 / 128])])
    for maxl in lengths.tolist():
        bound = np.float64(F32(1e-2)) * np.float64(maxl)
        high = F32(maxl)
        rungs = 0
        while np.float64(high) > bound:
            assert np.float64(high) != bound
            high, rungs = F32(high / F32(2)), rungs + 1
        assert rungs == 7 and np.float64(high) != bound, maxl
    assert set(VC.EQUIVALENT) == {"ladder_ge"}


# The first case, in the order of voxel_cases.all_cases() without the crowd, whose result a planted defect changes.
CAUGHT_BY = {
    "half_even": "rounding/0",
    "truncate": "stride/0.025/0",
    "floor_half": "rounding/0",
    "double_division": "division/0.025",
    "last_occurrence": "stride/0.025/0",
    "shared_set": "stride/0.025/2",
    "gate_lt": "gate/0",
    "gate_double": "gate/norm",
    "size_lt": "tie/size",
    "count_gt": "first/distinct/265",
    "reject_overwrites": "stride/0.11/5",
    "tolerance_double": "tie/tolerance",
}


def _differs(case, mutant):
    a, b = VC.witness_of(case), VC.witness_of(case, mutant)
    return not all(FC.same_cloud(x, y) for x, y in zip(a[:3], b[:3]))


def test_every_planted_defect_changes_a_named_case():
    assert set(CAUGHT_BY) | set(VC.EQUIVALENT) == set(W.MUTANTS)
    cases = [c for c in VC.all_cases() if not c.name.startswith("crowd/")]
    first = {m: next((c.name for c in cases if _differs(c, m)), None) for m in W.MUTANTS if m not in VC.EQUIVALENT}
    for mutant, name in first.items():
        print(f"mutant {mutant}: first seen by {name}")
    assert first == CAUGHT_BY
    # the float32-against-double family is what catches "division in double": no other family does
    for c in cases:
        if c.returns.shape[0] <= 3000:
            assert _differs(c, "double_division") == c.name.startswith("division/"), c.name
