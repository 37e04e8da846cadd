"""The 2D detector sweep on the CPU (cases: tests/detect2d_sweep_cases.py): on every case the C oracle, fed the same odometry,
options and sensor_to_base_link, equals the independent witness tests/witness/detect2d_witness.py BIT FOR BIT on centres and
de-skewed returns; every case's claims hold on the witness's outputs; every family holds the cases it was built for.  Where the two
CPU statements disagreed, laser_reflector_detect.cc and pose_extrapolator.cc of the reference would decide."""
import numpy as np
import pytest

from tests import detect2d_sweep_cases as SC

CASES = SC.all_cases()


@pytest.fixture(scope="module")
def results():
    return SC.witness_results(CASES)


def _oracle(c):
    """-> (obs_time, centres, returns) of OracleDetect2D, or BAD_SCAN."""
    from oracle.binding import OracleDetect2D
    o = OracleDetect2D(sensor_to_base_link=c["s2b"], **SC.options(c))
    try:
        for rec in c["odom"]:
            o.handle_odometry(*rec)
        try:
            t, cen = o.handle_scan(c["scan"])
        except ValueError as e:
            assert "rc=-1" in str(e), c["name"]
            return SC.BAD_SCAN
        return t, cen, o.returns()
    finally:
        o.close()


@pytest.mark.parametrize("family", sorted(SC.FAMILIES))
def test_oracle_equals_the_witness_on_every_case(oracle_lib, results, family):
    n = 0
    for c in CASES:
        if not c["name"].startswith(family):
            continue
        n += 1
        got, want = _oracle(c), results[c["name"]]
        if want == SC.BAD_SCAN or got == SC.BAD_SCAN:
            assert got == want, c["name"]
            continue
        t, cen, ret = got
        nan = SC.claims_nan(c)
        assert t == c["scan"].stamp, c["name"]
        assert cen.shape == want[0].shape and np.array_equal(cen, want[0], equal_nan=nan), c["name"]
        assert ret.shape == want[2].shape and np.array_equal(ret, want[2]), c["name"]
    assert n >= len(SC.REQUIRED[family])


def test_every_case_is_what_it_claims_to_be(results):
    for c in CASES:
        assert c["claims"], c["name"]
        SC.check_claims(c, results)


def test_names_are_unique_and_every_family_is_complete():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert all(n[0] in SC.FAMILIES and n[1] in "_1234567" for n in names)
    for family, required in SC.REQUIRED.items():
        missing = [n for n in required if n not in names]
        assert not missing, (family, missing)
    beams = sorted(c["scan"].ranges.shape[0] for c in CASES)
    assert [n for n in beams if n > 1500] == [8192, 8192]                 # (A7, still and moving: one scan)
    assert {1081, 1440, 1460, 1025, 257, 65} <= set(beams)
    # more lidars than the fleet's eight cached angle tables, and the bright plates of a decision under test pass the gate: see the claims
    geometries = {(c["scan"].ranges.shape[0], c["scan"].angle_min, c["scan"].angle_increment) for c in CASES}
    assert len(geometries) > 8
