"""The voxel filters on the GPU against tests/witness/voxel_witness.py: GridFrontEnd.VoxelFilter and AdaptiveVoxelFilter (kg_keys,
kg_first, kg_compact, kg_range_gate, the batched kg_*_b and the host's walk of the adaptive search) on handles of 1021 and 12288
points, and ScanMatchFleet.filter (kgb_filter) on every cloud within its limit, all scans of a size and options in one call and
once reversed.  Every assertion is equality with the witness of counts, order and bit patterns."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fleet_filter_scan_cases as FC
from tests import voxel_cases as VC

pytestmark = pytest.mark.gpu


def _options(values):
    from reflector_ekf_slam_amd.grid import AdaptiveVoxelFilterOptions
    return AdaptiveVoxelFilterOptions(*values)


def _handle_cases(max_points):
    """The crowd goes to the fleet whole; a handle takes every sixteenth of its scans."""
    crowd = [c for c in VC.all_cases() if c.name.startswith("crowd/")]
    rest = [c for c in VC.all_cases() if not c.name.startswith("crowd/")]
    return [c for c in rest + crowd[::16] if max(c.returns.shape[0], FC.misses_of((c.returns, c.misses)).shape[0]) <= max_points]


@pytest.mark.parametrize("max_points", [VC.SMALL_HANDLE, VC.LARGE_HANDLE])
def test_front_end_filters_equal_the_witness(max_points):
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    cases = _handle_cases(max_points)
    assert any(c.returns.shape[0] == max_points for c in cases) or max_points == VC.LARGE_HANDLE
    gf = GridFrontEnd(max_points=max_points, max_cells=64, max_candidates=1 << 10)
    for c in cases:
        want = VC.witness_of(c)
        got = FC.handle_triple(gf, (c.returns, c.misses), c.size, _options(c.options))
        assert FC.same_cloud(got[0], want[0]) and FC.same_cloud(got[1], want[1]), (c.name, got[0].shape, want[0].shape)
        assert FC.same_cloud(got[2], want[2]), (c.name, want[3], got[2].shape, want[2].shape)
    gf.close()
    if max_points == VC.LARGE_HANDLE:
        assert max(c.returns.shape[0] for c in cases) == 12000 and len(cases) == len(_handle_cases(1 << 30))
    else:
        assert len(cases) >= 100 and sum(c.name.startswith("first/") for c in cases) == 5 * (len(VC.FIRST_COUNTS) + 1)


def test_fleet_filter_equals_the_witness_in_one_call_and_reversed():
    from reflector_ekf_slam_amd import fleet_match as M
    groups = VC.fleet_groups()
    assert sum(len(g) for g in groups.values()) >= len(VC.all_cases()) - 20 and M.filter_max_points() >= VC.FLEET_LIMIT
    m = M.ScanMatchFleet(max_scans=max(len(g) for g in groups.values()), max_points=VC.FLEET_LIMIT, max_cells=64, max_rotations=1)
    for (size, options), cases in groups.items():
        scans = [(c.returns, c.misses) for c in cases]
        opt = _options(options)
        for order in (slice(None), slice(None, None, -1)):
            got = m.filter(scans[order], size, opt)[order]
            assert len(got) == len(cases)
            for c, r in zip(cases, got):
                want = VC.witness_of(c)
                assert r.status == FC.OK and FC.same_result(r, want[:3]), (c.name, want[3], r.filtered.shape, want[2].shape)
    m.close()
