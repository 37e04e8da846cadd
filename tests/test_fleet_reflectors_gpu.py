"""rfleet_get_reflectors on the MI355X: k_fleet_reflectors' marker ellipses against the single filter's k_ellipses (the same bits),
positions and blocks against get_state (copies), against the oracle on a real session and an eigen-solver comparison on crafted
blocks, the member list's offsets and the capacity rules, stream order behind submit, and the saved map's bytes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import fleet_reflector_cases as RC

pytestmark = pytest.mark.gpu

INVALID, BUFFER = -1, -6
SENTINEL = -7.25


def _options(n):
    from reflector_ekf_slam_amd import EKFOptions
    return [EKFOptions() for _ in range(n)]


def _make(members, max_landmarks):
    from reflector_ekf_slam_amd import ReflectorEKFSLAMFleet
    fl = ReflectorEKFSLAMFleet(_options(len(members)), max_landmarks=max_landmarks)
    for i, m in enumerate(members):
        fl.set_state(i, m.t, m.mu, m.sigma)
    return fl


@pytest.fixture(scope="module")
def fleets():
    """Fleet A and fleet B with their cases' states; no test changes them."""
    A, B = RC.fleet_a(), RC.fleet_b()
    fa, fb = _make(A, RC.ML_A), _make(B, RC.ML_B)
    yield (fa, A), (fb, B)
    fa.close()
    fb.close()


def test_same_bits_as_the_single_filter(fleets):
    from reflector_ekf_slam_amd import EKFOptions, ReflectorEKFSLAM
    nan_rows = 0
    for fl, members in fleets:
        ell = fl.marker_ellipses()
        assert len(ell) == len(members)
        for i, m in enumerate(members):
            g = ReflectorEKFSLAM(EKFOptions(), max_landmarks=128, device=0, auto_grow=False)
            g.set_state(m.t, m.mu, m.sigma)
            want = g.marker_ellipses()
            g.close()
            assert want.shape == ell[i].shape == (m.L, 5)
            assert RC.same_bits(ell[i], want), (i, np.argwhere(ell[i] != want)[:4].tolist())
            assert RC.same_bits(fl.member(i).marker_ellipses(), want)
            nan_rows += int(np.isnan(want).any(axis=1).sum())
    assert nan_rows >= 2                                                                # the NaN patterns were among the bits


def test_positions_and_blocks_are_copies(fleets):
    for fl, members in fleets:
        got = fl.landmarks()
        assert len(got) == len(members)
        for i, m in enumerate(members):
            st = fl.get_state(i)
            xy, cov = got[i]
            assert xy.shape == (m.L, 2) and cov.shape == (m.L, 2, 2)
            assert np.array_equal(xy, st.mu[3:].reshape(-1, 2))
            for k in range(m.L):
                assert np.array_equal(cov[k], st.sigma[3 + 2 * k: 5 + 2 * k, 3 + 2 * k: 5 + 2 * k]), (i, k)
            want_xy, want_cov = RC.expected_landmarks(m)                                # and both are the case's lower triangle
            assert np.array_equal(xy, want_xy) and np.array_equal(cov, want_cov)


def test_crafted_blocks_against_an_eigen_solver(fleets):
    """The ellipses of the positive definite crafted blocks, drawn, are the blocks: within 16 x the floor the oracle's rows reach."""
    from tests.test_fleet_reflectors_cpu import ELLIPSE_FLOOR, GPU_FACTOR
    worst = 0.0
    for fl, members in fleets:
        ell = fl.marker_ellipses()
        for i, m in enumerate(members):
            keep = RC.spd_rows(m)
            if keep.any():
                worst = max(worst, RC.ellipse_error(ell[i][keep], m.blocks[keep]))
    print(f"\nfleet ellipses against the crafted blocks: {worst:.3e} = {worst / ELLIPSE_FLOOR:.2f} x the floor (bound {GPU_FACTOR:g} x)")
    assert worst <= GPU_FACTOR * ELLIPSE_FLOOR


def test_real_session_against_the_oracle(oracle_lib):
    from oracle.binding import OracleEKF
    from reflector_ekf_slam_amd import ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd import session as S
    from tests.helpers import ellipse_matrices
    ss = RC.sessions()
    opts = [S.options_for(s) for s in ss]
    fl = ReflectorEKFSLAMFleet(opts, max_landmarks=32)
    try:
        for i, (s, opt) in enumerate(zip(ss, opts)):
            o = OracleEKF(s.config.odom_model, s.init_time, s.init_pose, opt.linear_velocity_cov, opt.angular_velocity_cov, opt.observation_cov)
            S.replay(s, fl.member(i))
            S.replay(s, o)
            eg, eo = fl.marker_ellipses([i])[0], o.marker_ellipses()
            L = (o.n - 3) // 2
            o.close()
            assert eg.shape == eo.shape == (L, 5) and L >= 8 and int(fl.n()[i]) == 3 + 2 * L
            assert np.abs(eg[:, :2] - eo[:, :2]).max() < 1e-12                          # the tolerances of tests/test_ekf_gpu.py
            Mg, Mo = ellipse_matrices(eg), ellipse_matrices(eo)
            assert np.abs(Mg - Mo).max() <= 1e-9 * np.abs(Mo).max()
            assert np.allclose(eg[:, 3:], eo[:, 3:], rtol=1e-9, atol=0) and np.abs(np.sin(eg[:, 2] - eo[:, 2])).max() < 1e-6
        both = fl.marker_ellipses()
        assert RC.same_bits(both[1], eg) and both[0].shape[0] >= 8
        assert not fl.flags().any()
    finally:
        fl.close()


# ---- lists, offsets, capacity ---------------------------------------------------------------------------------------------------
def _raw(fl, members, cap, want=(True, True, True), count=None):
    """rfleet_get_reflectors itself on sentinel-filled arrays of cap (+ 2 guard) rows: -> (code, counts, ell, xy, cov)."""
    from reflector_ekf_slam_amd import fleet
    L = fleet._reflectors_lib()
    mem = None if members is None else np.ascontiguousarray(members, np.int32)
    count = (fl.B if mem is None else mem.shape[0]) if count is None else count
    counts = np.full(max(count, 1) + 1, -3, np.int32)
    arrs = [np.full((cap + 2, w), SENTINEL) for w in (5, 2, 4)]
    ptrs = [a.ctypes.data if w else None for a, w in zip(arrs, want)]
    rc = L.rfleet_get_reflectors(fl._h, None if mem is None else mem.ctypes.data, count, counts.ctypes.data, *ptrs, cap)
    assert counts[-1] == -3
    return rc, counts[:count], arrs[0], arrs[1], arrs[2]


def _expected_rows(fl, members, cases):
    """The rows of the listed members one after the other, from per-member calls' parts: ellipses of single-member calls and
    get_state's means and blocks."""
    e = [fl.marker_ellipses([i])[0] for i in members]
    xc = [RC.expected_landmarks(cases[i]) for i in members]
    return (np.concatenate(e).reshape(-1, 5), np.concatenate([x for x, _ in xc]).reshape(-1, 2),
            np.concatenate([c for _, c in xc]).reshape(-1, 4))


@pytest.mark.parametrize("members", [[5, 0, 3, 6], [2], [7, 6, 5, 4, 3, 2, 1, 0], None], ids=["scrambled", "alone", "reversed", "all"])
def test_lists_and_offsets(fleets, members):
    (fl, cases), _ = fleets
    listed = list(range(fl.B)) if members is None else members
    want_counts = [cases[i].L for i in listed]
    R = sum(want_counts)
    we, wx, wc = _expected_rows(fl, listed, cases)
    rc, counts, e, x, c = _raw(fl, members, R)                                          # an exact fit
    assert rc == 0 and counts.tolist() == want_counts
    assert RC.same_bits(e[:R], we) and np.array_equal(x[:R], wx) and np.array_equal(c[:R], wc)
    assert (e[R:] == SENTINEL).all() and (x[R:] == SENTINEL).all() and (c[R:] == SENTINEL).all()
    # the Python face: the same rows, per member
    got = fl.marker_ellipses(members)
    assert [g.shape[0] for g in got] == want_counts and RC.same_bits(np.concatenate(got).reshape(-1, 5), we)
    lm = fl.landmarks(members)
    assert np.array_equal(np.concatenate([a for a, _ in lm]).reshape(-1, 2), wx)
    assert np.array_equal(np.concatenate([b for _, b in lm]).reshape(-1, 4), wc)


def test_capacity(fleets):
    for fl, cases in fleets:
        want_counts = [m.L for m in cases]
        R = sum(want_counts)
        rc, counts, e, x, c = _raw(fl, None, R - 1)                                     # one row short
        assert rc == BUFFER and counts.tolist() == want_counts
        assert (e == SENTINEL).all() and (x == SENTINEL).all() and (c == SENTINEL).all()
        rc, counts, e, x, c = _raw(fl, None, R + 1)
        assert rc == 0 and counts.tolist() == want_counts and (e[R:] == SENTINEL).all() and not (e[:R] == SENTINEL).any()
        rc, counts, e, x, c = _raw(fl, None, 0, want=(False, False, False))             # counts alone
        assert rc == 0 and counts.tolist() == want_counts
    (fl, cases), _ = fleets
    rc, counts, e, x, c = _raw(fl, [0, 6], 0, want=(False, False, False))
    assert rc == 0 and counts.tolist() == [0, 0]
    rc, counts, e, x, c = _raw(fl, [0, 6], 1)                                           # members without reflectors: count 0 and nothing else
    assert rc == 0 and counts.tolist() == [0, 0] and (e == SENTINEL).all() and (x == SENTINEL).all() and (c == SENTINEL).all()
    rc, counts, e, x, c = _raw(fl, [], 4)
    assert rc == 0 and (e == SENTINEL).all()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_one_output_alone(fleets, which):
    (fl, cases), _ = fleets
    listed = [3, 7, 1]
    R = sum(cases[i].L for i in listed)
    want = _expected_rows(fl, listed, cases)
    rc, counts, *arrs = _raw(fl, listed, R, want=tuple(k == which for k in range(3)))
    assert rc == 0 and counts.tolist() == [cases[i].L for i in listed]
    for k in range(3):
        if k == which:
            assert RC.same_bits(arrs[k][:R], want[k]) and (arrs[k][R:] == SENTINEL).all()
        else:
            assert (arrs[k] == SENTINEL).all()


def test_bad_lists_are_refused(fleets):
    from reflector_ekf_slam_amd import RekfError
    (fl, cases), (fb, _) = fleets
    for bad in ([1, 2, 1], [0, 0], [8], [-1], [3, 9, 4], [1, 2, 3, 4, 5, 6, 7, 0, 1]):
        rc, counts, e, x, c = _raw(fl, bad, 400)
        assert rc == INVALID, bad
        assert (counts == -3).all() and (e == SENTINEL).all() and (x == SENTINEL).all() and (c == SENTINEL).all()
    assert _raw(fl, None, 400, count=3)[0] == INVALID                                    # "all members" is B of them
    assert _raw(fb, [3], 10)[0] == INVALID
    with pytest.raises(RekfError) as err:
        fl.marker_ellipses([2, 2])
    assert err.value.code == INVALID
    with pytest.raises(IndexError):
        fl.save_map_txt(8, "unused")
    assert fl.marker_ellipses([]) == [] and fl.landmarks([]) == []


# ---- stream order ---------------------------------------------------------------------------------------------------------------
def _clouds(rng, K, far):
    """K robot-frame points, metres apart from each other and from every earlier scan's (far: the ring they lie on)."""
    ang = np.linspace(0.0, 2 * np.pi, K, endpoint=False) + rng.uniform(0.0, 0.1)
    return np.stack([far * np.cos(ang), far * np.sin(ang)], -1).astype(np.float32)


def test_stream_order():
    from reflector_ekf_slam_amd import ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd.fleet import scan_event
    rng = np.random.default_rng(12)
    first = {0: _clouds(rng, 5, 4.0), 2: _clouds(rng, 9, 4.0), 3: _clouds(rng, 1, 4.0)}
    second = {0: _clouds(rng, 3, 8.0), 1: _clouds(rng, 7, 8.0), 2: _clouds(rng, 2, 8.0)}
    fl, twin = (ReflectorEKFSLAMFleet(_options(4), max_landmarks=16) for _ in range(2))
    try:
        assert [e.shape for e in fl.marker_ellipses()] == [(0, 5)] * 4
        ev1 = [scan_event(b, 0.1, xy) for b, xy in first.items()]
        fl.submit(ev1)
        got = fl.marker_ellipses()                                                      # no sync in between
        twin.submit(ev1)
        twin.sync()
        want = twin.marker_ellipses()
        assert [g.shape[0] for g in got] == [5, 0, 9, 1] == ((fl.n() - 3) // 2).tolist()
        assert all(RC.same_bits(g, w) for g, w in zip(got, want))
        assert all(np.isfinite(g).all() for g in got)
        ev2 = [scan_event(b, 0.2, xy) for b, xy in second.items()]
        fl.submit(ev2)
        got2 = fl.landmarks()
        twin.submit(ev2)
        twin.sync()
        want2 = twin.landmarks()
        assert [xy.shape[0] for xy, _ in got2] == [8, 7, 11, 1] == ((twin.n() - 3) // 2).tolist()
        for (gx, gc), (wx, wc), i in zip(got2, want2, range(4)):
            assert RC.same_bits(gx, wx) and RC.same_bits(gc, wc)
            st = fl.get_state(i)
            assert np.array_equal(gx, st.mu[3:].reshape(-1, 2))
    finally:
        fl.close()
        twin.close()


# ---- the saved map --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference_bytes", [False, True])
def test_saved_map(reference_bytes, tmp_path):
    from reflector_ekf_slam_amd.ekf_slam import Map, save_map_txt
    cases = RC.fleet_b()
    fl = _make(cases, RC.ML_B)
    try:
        a, b = str(tmp_path / "fleet.txt"), str(tmp_path / "state.txt")
        for i in range(fl.B):                                                           # no shared map
            assert fl.loaded_map(i) is None
            fl.save_map_txt(i, a, reference_bytes)
            save_map_txt(b, fl.get_state(i), None, reference_bytes)
            assert open(a, "rb").read() == open(b, "rb").read(), i
        rng = np.random.default_rng(3)
        xy, cov = rng.uniform(-30, 30, size=(4, 2)).astype(np.float32), rng.uniform(0.001, 0.1, size=(4, 2, 2))
        fl.set_map(xy, cov, members=[0, 1])                                             # members 0 (5 reflectors) and 1 (none) use it
        for i in range(fl.B):
            loaded = Map(xy, cov) if i < 2 else None
            fl.save_map_txt(i, a, reference_bytes)
            save_map_txt(b, fl.get_state(i), loaded, reference_bytes)
            got = open(a, "rb").read()
            assert got == open(b, "rb").read() and got.count(b"\n") == 2, i
            assert len(got.split(b"\n")[0].replace(b",", b" ").split()) == 2 * (cases[i].L + (4 if i < 2 else 0))
        fl.set_map(np.zeros((0, 2), np.float32), np.zeros((0, 2, 2)))                   # cleared: no loaded points any more
        fl.save_map_txt(0, a, reference_bytes)
        save_map_txt(b, fl.get_state(0), None, reference_bytes)
        assert open(a, "rb").read() == open(b, "rb").read()
    finally:
        fl.close()
