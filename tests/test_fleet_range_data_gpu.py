"""GetRangeData of any list of members in ONE launch (rdet2d_batch_get_range_data_all / LaserReflectorDetectFleet.range_data,
k_det2d_batch_range_data of csrc/det2d_batch.hip) against its specification, the per-member getter, and against the oracle's
returns: counts, origins and rows BIT FOR BIT.  Nothing has a tolerance.  Cases: tests/fleet_range_data_cases.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import fleet_range_data_cases as RC

pytestmark = pytest.mark.gpu

OK, INVALID, BUFFER = 0, -1, -5
SENTINEL = np.float32(-7.25)


def _fleet(members, max_beams=RC.MAX_BEAMS):
    from reflector_ekf_slam_amd import LaserReflectorDetectFleet
    from reflector_ekf_slam_amd.detect import ReflectorDetectOptions
    return LaserReflectorDetectFleet([ReflectorDetectOptions(**m["opts"]) for m in members], max_beams=max_beams,
                                     sensor_to_base_link=np.array([m["s2b"] for m in members], dtype=np.float64))


def _msg(sc):
    from reflector_ekf_slam_amd.detect import LaserScan
    return LaserScan(sc.stamp, sc.angle_min, sc.angle_max, sc.angle_increment, sc.scan_time, sc.range_min, sc.range_max, sc.ranges, sc.intensities)


def _tick(fl, tick):
    from reflector_ekf_slam_amd import OdometryData
    for m, stream in tick["odom"].items():
        for t, px, py, qz, qw, vx, vy, wz in stream:
            fl.HandleOdometryData(m, OdometryData(t, (vx, vy, 0.0), (0.0, 0.0, wz), (px, py, 0.0), (qw, 0.0, 0.0, qz)))
    return fl.detect([(m, _msg(sc)) for m, sc in tick["scans"]])


def _same_rows(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(fl, got, members, want=None, where=""):
    """``range_data``'s list against the per-member getter and, where given, the oracle's rows."""
    assert len(got) == len(members), where
    for g, m in zip(got, members):
        one = fl.GetRangeData(m)
        assert g.origin.dtype == np.float32 and g.origin.tobytes() == one.origin.tobytes(), (where, m)
        assert _same_rows(g.returns, one.returns), (where, m, g.returns.shape, one.returns.shape)
        if want is not None:
            assert _same_rows(g.returns, want[m]), (where, m)


def _raw(fl, members, count, cap, rows=True, origins=True, counts=True, room=None):
    """The C call with sentinel-filled outputs.  -> (rc, counts, origins, rows)."""
    from reflector_ekf_slam_amd.fleet_detect import _range_data_lib
    mem = None if members is None else np.ascontiguousarray(members, dtype=np.int32)
    n = max(abs(count), 1)
    c = np.full(n, -99, np.int32)
    o = np.full((n, 2), SENTINEL, np.float32)
    r = np.full((max(room if room is not None else cap, 1) + 4, 2), SENTINEL, np.float32)
    rc = _range_data_lib().rdet2d_batch_get_range_data_all(fl._h, None if mem is None else mem.ctypes.data, count, c.ctypes.data if counts else None,
                                                          o.ctypes.data if origins else None, r.ctypes.data if rows else None, cap)
    return rc, c, o, r


def _untouched(*arrays):
    return all((a == (-99 if a.dtype == np.int32 else SENTINEL)).all() for a in arrays)


@pytest.fixture(scope="module")
def edge(oracle_lib):
    members, ticks = RC.edge_case()
    want = RC.expected_rows(members, ticks)[0]
    fl = _fleet(members)
    got = _tick(fl, ticks[0])
    assert [s for s, _ in got] == [0] * len(members)
    yield fl, members, want
    fl.close()


def test_all_members_a_permuted_subset_and_every_member_alone(edge):
    fl, members, want = edge
    B = len(members)
    assert [w.shape[0] for w in want] == list(RC.EDGE_COUNTS)
    got = fl.range_data()
    _check(fl, got, range(B), want, "all")
    for g, m in zip(got, members):
        assert g.origin.tobytes() == np.array(m["s2b"][:2], np.float32).tobytes()
    _check(fl, fl.range_data(list(range(B))), range(B), want, "all, listed")
    _check(fl, fl.range_data(RC.PERMUTED), RC.PERMUTED, want, "permuted")
    _check(fl, fl.range_data(list(range(B))[::-1]), list(range(B))[::-1], want, "reversed")
    for m in range(B):
        _check(fl, fl.range_data([m]), [m], want, ("alone", m))
    assert fl.range_data([]) == []
    # the origin is the member's current sensor_to_base_link, as the getter reads it
    fl.SetSensorToBaseLinkTransform(3, (0.5, -0.25, 1.0))
    got = fl.range_data([4, 3])
    assert got[1].origin.tolist() == [0.5, -0.25] and got[0].origin.tobytes() == np.array(members[4]["s2b"][:2], np.float32).tobytes()
    _check(fl, got, [4, 3], want, "after a new transform")
    fl.SetSensorToBaseLinkTransform(3, members[3]["s2b"])


def test_room_counts_only_and_too_little_room(edge):
    fl, members, want = edge
    B = len(members)
    total = sum(RC.EDGE_COUNTS)
    flat = np.concatenate(want)
    # exactly enough room is enough
    rc, c, o, r = _raw(fl, None, B, total)
    assert rc == OK and c.tolist() == list(RC.EDGE_COUNTS) and r[:total].tobytes() == flat.tobytes() and _untouched(r[total:])
    assert o.tobytes() == np.array([m["s2b"][:2] for m in members], np.float32).tobytes()
    # one row too little: counts are right, no row and no origin is touched; counts sizes the second call
    rc, c, o, r = _raw(fl, None, B, total - 1)
    assert rc == BUFFER and c.tolist() == list(RC.EDGE_COUNTS) and _untouched(o, r)
    rc, c2, o2, r2 = _raw(fl, None, B, int(c.sum()))
    assert rc == OK and r2[:total].tobytes() == flat.tobytes()
    sub = list(RC.PERMUTED)
    n_sub = sum(RC.EDGE_COUNTS[m] for m in sub)
    rc, c, o, r = _raw(fl, sub, len(sub), n_sub - 1)
    assert rc == BUFFER and c.tolist() == [RC.EDGE_COUNTS[m] for m in sub] and _untouched(o, r)
    rc, c, o, r = _raw(fl, sub, len(sub), n_sub)
    assert rc == OK and r[:n_sub].tobytes() == np.concatenate([want[m] for m in sub]).tobytes() and _untouched(r[n_sub:])
    # counts only: counts and origins, whatever the room; without origins too
    for cap in (0, 5, total):
        rc, c, o, r = _raw(fl, None, B, cap, rows=False, room=total)
        assert rc == OK and c.tolist() == list(RC.EDGE_COUNTS) and _untouched(r)
        assert o.tobytes() == np.array([m["s2b"][:2] for m in members], np.float32).tobytes()
    rc, c, o, r = _raw(fl, sub, len(sub), 0, rows=False, origins=False, room=total)
    assert rc == OK and c.tolist() == [RC.EDGE_COUNTS[m] for m in sub] and _untouched(o, r)
    # rows without origins; members without rows: nothing to launch, nothing touched
    rc, c, o, r = _raw(fl, sub, len(sub), n_sub, origins=False)
    assert rc == OK and _untouched(o) and r[:n_sub].tobytes() == np.concatenate([want[m] for m in sub]).tobytes()
    rc, c, o, r = _raw(fl, [6, 2], 2, 0)
    assert rc == OK and c.tolist() == [0, 0] and _untouched(r) and not _untouched(o)


def test_refusals_and_a_correct_call_after_each(edge):
    fl, members, want = edge
    B = len(members)
    total = sum(RC.EDGE_COUNTS)

    def then_right():
        _check(fl, fl.range_data([1, 0, 5]), [1, 0, 5], want, "after a refusal")

    refused = [
        ([0, B], 2, total, {}),                              # a member out of range
        ([-1, 0], 2, total, {}),
        ([2, 5, 2], 3, total, {}),                           # a member listed twice
        (list(range(B)) + [0], B + 1, total, {}),
        (None, B - 1, total, {}),                            # members NULL with count != B
        (None, B + 1, total, {}),
        ([0, 1], -1, total, {}),                             # count < 0
        ([0, 1], 2, total, dict(counts=False)),              # null counts with count > 0
        ([0, 1], 2, -1, dict(room=total)),                   # cap_points < 0
    ]
    for mem, count, cap, kw in refused:
        rc, c, o, r = _raw(fl, mem, count, cap, **kw)
        assert rc == INVALID and _untouched(c, o, r), (mem, count, cap)
        then_right()
    from reflector_ekf_slam_amd.fleet_detect import _range_data_lib
    call = _range_data_lib().rdet2d_batch_get_range_data_all
    assert call(None, None, B, None, None, None, 0) == INVALID                    # a null handle
    rc, c, o, r = _raw(fl, [3], 0, 0)                                             # count == 0: OK, does nothing
    assert rc == OK and _untouched(c, o, r)
    assert call(fl._h, None, 0, None, None, None, 0) == (OK if B == 0 else INVALID)
    then_right()
    # between submit and collect: refused like the getter, and the submit stays pending
    _, ticks = RC.edge_case()
    fl.submit([(m, _msg(sc)) for m, sc in ticks[0]["scans"][:4]])
    rc, c, o, r = _raw(fl, None, B, total)
    assert rc == INVALID and _untouched(c, o, r)
    from reflector_ekf_slam_amd.detect import RdetError
    with pytest.raises(RdetError):
        fl.range_data([0])
    with pytest.raises(RdetError):
        fl.GetRangeData(0)
    assert [s for s, _ in fl.collect()] == [0] * 4
    _check(fl, fl.range_data(), range(B), want, "after the collect")              # (the same scans again: the same rows)


def test_members_that_sat_out_had_no_beams_or_a_malformed_message(oracle_lib):
    members, ticks = RC.history_case()
    want = RC.expected_rows(members, ticks)
    fl = _fleet(members, max_beams=1024)
    assert [r.returns.shape[0] for r in fl.range_data()] == [0] * 4                # before any scan
    assert [s for s, _ in _tick(fl, ticks[0])] == [0] * 4
    _check(fl, fl.range_data(), range(4), want[0], "tick 1")
    assert [s for s, _ in _tick(fl, ticks[1])] == [0, -3, 0]
    got = fl.range_data()
    assert [g.returns.shape[0] for g in got] == list(RC.HISTORY_AFTER)
    _check(fl, got, range(4), want[1], "tick 2")
    _check(fl, fl.range_data([3, 1, 0]), [3, 1, 0], want[1], "tick 2, a subset")
    fl.close()


def test_three_hundred_members_in_one_call(oracle_lib):
    members, ticks = RC.many_case()
    want = RC.expected_rows(members, ticks)[0]
    fl = _fleet(members, max_beams=64)
    assert [s for s, _ in _tick(fl, ticks[0])] == [0] * RC.MANY
    rc, counts, origins, rows = fl.range_data_code()
    assert rc == OK and counts.tolist() == RC.many_counts() and rows.tobytes() == np.concatenate(want).tobytes()
    got = fl.range_data()
    for m in range(RC.MANY):
        assert _same_rows(got[m].returns, want[m]), m
    for m in (0, 1, 64, 150, 299):
        _check(fl, [got[m]], [m], want, m)
    order = np.random.default_rng(4).permutation(RC.MANY)[:200].tolist()
    sub = fl.range_data(order)
    assert all(_same_rows(g.returns, want[m]) for g, m in zip(sub, order))
    fl.close()
