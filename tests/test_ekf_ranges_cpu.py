"""The range cases of the downdate (tests/ekf_range_cases.py) on the CPU, so that tests/test_ekf_ranges_gpu.py is about the
kernels only: the table of forms is what tests/downdate_schedule.py derives for 256 CUs, every case has the form it is named
for, the FP64 floor that sets the GPU bound is measured here, and six defects of a multi-tile range are planted into a numpy
emulation of the tile pipeline -- each moves sigma by more than 1000 x the GPU bound on every case whose schedule contains the
situation, and none is visible (bit-equal) when every workgroup holds one tile, which is the schedule the shape sweep
(tests/ekf_shape_cases.py) runs on 256 CUs."""
from __future__ import annotations

import hashlib
import math

import numpy as np
import pytest

from tests import downdate_schedule as DS
from tests import ekf_range_cases as RC
from tests import ekf_shape_cases as EC
from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests.witness import fleet_witness as FW

pytestmark = pytest.mark.skipif(not FW.available(), reason="numpy.longdouble has no 64-bit mantissa on this platform")


@pytest.fixture(scope="module")
def all_cases():
    return RC.cases(256)


@pytest.fixture(scope="module")
def reference_runs(all_cases, oracle_lib):
    return {c.name: H.run_references(c, RC.SUITE) for c in all_cases}


# ---- the restated launches -----------------------------------------------------------------------------------------------------
def test_launch_arithmetic_is_the_sources():
    assert (DS.DT, DS.DD_WG_PER_CU, DS.FRONT_MB, DS.REKF_SCAN_MIN_DD_WGS, DS.MID_ROWS) == (64, 1, 32, 48, 16)
    assert DS.slots_of(256) == 256 and DS.slots_of(256, 8) == 248 and DS.slots_of(256, 40) == 224 and DS.slots_of(8, 8) == 8
    # n = 1921: 121 mid workgroups and 8 for the front end, rounded up to the XCD count; 176 items for 120 workgroups
    assert DS.role_wgs(256, 1921, 8) == (120, 176, True)
    assert DS.role_wgs(256, 1409, 8) == (100, 100, True)                 # more workgroups than items: one item each
    assert DS.role_wgs(256, 3331, 8)[2] is False                         # (209 + 8 -> 224) + 48 > 256: the two-launch chain
    assert DS.role_wgs(304, 3331, 8)[2] is True
    for T in range(1, 70):
        assert DS.role_wgs(256, 64 * T, 0)[1] == len(DS.queue_items(T))


def test_the_cursor_seed_is_exact():
    """The issue of a range whose FIRST look-up walks the cursor off its sqrtf seed does not exist up to T = 64: at the first tile
    of a column the discriminant is the square of an odd integer below 2^24, so the closed form is exact in float32 and between
    two such tiles it lies strictly between two integers.  The cursor's loops are exercised by ranges that cross a column."""
    for sub in (1, 2):
        for T in range(sub + 1, 65):
            TT = T - sub
            t0 = 0
            for J in range(TT):
                for tt in range(t0, t0 + TT - J):
                    assert DS.seed_column(TT, tt) == J, (T, sub, tt)
                t0 += TT - J


def test_the_table_of_forms_on_256_cus(all_cases):
    assert RC.table(256) == RC.TABLE_256
    assert RC.names(256) == [c.name for c in all_cases] and len({c.name for c in all_cases}) == 9
    by_form = {c.form: c for c in all_cases if c.kind == "range" and c.K == RC.K_DEFAULT}
    assert list(by_form) == list(DS.FORMS)
    want = {"sub1_range2": dict(sub=1, lengths={1, 2}, classA={1}), "sub1_range3": dict(sub=1, lengths={2, 3}, classA={1}),
            "sub2_range3": dict(sub=2, lengths={2, 3}, classA={1, 2}), "sub2_range4": dict(sub=2, lengths={3, 4}, classA={1, 2}),
            "sub2_range5": dict(sub=2, lengths={4, 5}, classA={1, 2})}
    total = dict(cross=0, col0_mixed=0, off_seed=0)
    for form, c in by_form.items():
        assert (c.T, c.L, c.n) == (*RC.TABLE_256[form], 64 * (c.T - 1) + 1) and c.form_alone == form
        f = DS.forms(c.T, c.slots_alone)
        assert {k: f[k] for k in ("sub", "lengths", "classA")} == want[form] and f["renumbered"], (form, f)
        assert DS.smallest_T(form, c.slots_alone) == c.T and DS.form_of(c.T - 1, c.slots_alone) != form
        for slots in (c.slots_alone, c.slots_front):
            g = DS.forms(c.T, slots)
            for k in total:
                total[k] += g[k]
        print(f"\n  {c.name}: k_downdate2 {f}; k_dd_front ({c.slots_front} workgroups): {c.form_front}; queue role: {c.role_items} items "
              f"for {c.role_wgs} workgroups")
    # what k_dd_front runs (K workgroups fewer): the same form, but the switch to sub = 2 comes one tile row earlier
    assert [by_form[f].form_front for f in DS.FORMS] == ["sub1_range2", "sub2_range3", "sub2_range3", "sub2_range4", "sub2_range5"]
    assert DS.smallest_T("sub1_range3", 248) is None
    # over all cases: a range crosses a column (needH, the cursor's walk), a range holds a column-0 tile and another column's
    assert total["cross"] >= 1 and total["col0_mixed"] >= 1, total
    assert total["off_seed"] == 0                                        # (test_the_cursor_seed_is_exact says why)
    # the queue role hands out more items than it has workgroups wherever the state is large enough for it
    assert [by_form[f].second_item for f in DS.FORMS] == [False, True, True, True, True]
    assert [(by_form[f].role_items, by_form[f].role_wgs) for f in DS.FORMS] == [(100, 100), (176, 128), (187, 128), (260, 104), (330, 80)]
    assert all(c.one_launch_fits for c in all_cases)
    chunks = [c for c in all_cases if c.kind == "range" and c.K != RC.K_DEFAULT]
    assert [(c.T, c.K, 16 * math.ceil(2 * c.K / 16)) for c in chunks] == [(23, 16, 32), (23, 24, 48), (23, 32, 64)]
    assert all(c.form_alone == c.form_front == "sub1_range2" for c in chunks)
    print(f"\n  over the form cases: {total}")


def test_the_growing_case_derives_a_multi_tile_schedule(all_cases):
    g = [c for c in all_cases if c.kind == "range_grow"]
    assert len(g) == 1
    c = g[0]
    assert c.cap == c.L + 8 and not c.auto_grow and c.N2 == 3 and c.MM + c.N2 == RC.K_DEFAULT and c.T == 31 == c.T_host == c.T_grown
    for slots in (c.slots_alone, c.slots_front):
        grid = DS.host_plan(c.T_host, slots)[0]
        for T in (c.T, c.T_grown):
            lo, x, sub = DS.kernel_plan(T, grid)
            lengths = {len(DS.device_tiles(T, grid, lo, x, sub, b)) for b in range(grid)}
            assert max(lengths) >= 2, (slots, T, lengths)
    assert DS.form_of(c.T, c.slots_alone, derived=True) == "sub1_range3"
    assert len(c.expect[0][1]) == 3 and {c.L + 2, c.L} <= {g_ for _, g_ in c.expect[1][0]}


def test_the_generic_loop_sizes_of_test_ekf_gpu():
    """The figures in the docstring of tests/test_ekf_gpu.py::test_states_beyond_the_baseline_size_take_the_generic_downdate_loop."""
    got = [(DS.tiles_of(3 + 2 * L), DS.host_plan(DS.tiles_of(3 + 2 * L), 256)[1:], DS.forms(DS.tiles_of(3 + 2 * L), 256)["lengths"]) for L in (1472, 2048)]
    assert got == [(47, (4, 199, 2), {4, 5}), (65, (10, 106, 2), {10, 11})]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _sha(c):
    m = hashlib.sha256()
    for a in (c.mu, c.P, np.asarray(c.vt)):
        m.update(np.ascontiguousarray(a).tobytes())
    for ev in c.events:
        m.update(np.float64(ev[1]).tobytes())
        m.update(np.ascontiguousarray(ev[3]).tobytes())
    return m.hexdigest()


def test_the_lattice_parameter_leaves_existing_cases_their_bits():
    """Recorded before ekf_shape_cases.Builder took a lattice size."""
    assert _sha(EC.sweep_case(38, 200, 32)) == "cda55c0413afa76801d92926a899b1fdf945d141d86fd1484fde27b172f3b79a"
    assert _sha(EC.growing_case(8, 30, 24, "cross")) == "86c1adc890d49952a113f655fca0db6c3805ecbc549459b522a42ae2f3afc3c8"


def test_cases_are_what_they_claim(all_cases):
    worst = 0.0
    for c in all_cases:
        assert c.n == 3 + 2 * c.L == c.mu.shape[0] and (c.cap == c.L) == (c.kind == "range") and c.flags == 0 and not c.kept
        assert c.vt[0] != 0 and c.vt[2] != 0 and [ev[1] for ev in c.events] == [EC.T0 + EC.DT, EC.T0 + 2 * EC.DT]
        d = np.diag(c.P)
        assert 1e-4 <= d.min() and d.max() <= 1e-1 and np.array_equal(c.P, c.P.T), c.name
        assert np.count_nonzero(c.P) == c.P.size                          # dense: a wrong panel moves every element of a tile
        lm = c.mu[3:].reshape(-1, 2)
        assert np.array_equal(lm, lm.astype(np.float32).astype(np.float64))
        assert np.abs(np.round((lm / EC.PITCH)) * EC.PITCH - lm).max() <= EC.JITTER * (1 + 1e-6)
        for k in (0, 1):
            assert len(c.margins[k]) == len(c.events[k][3])
            assert all(a >= FC.MARGIN_MIN and b >= FC.MARGIN_MIN for a, b in c.margins[k]), (c.name, k)
        sets = [[g for _, g in c.expect[k][0]] for k in (0, 1)]
        assert len(c.events[0][3]) == c.K and len(sets[0]) == c.MM == len(set(sets[0])) == len(set(sets[1])) and set(sets[0]) != set(sets[1])
        assert len(c.expect[0][1]) == c.N2 and len(c.expect[1][1]) == 0
        # reflector 0, the last one (its y is the one row of the last tile row), both straddlers, the last but one (the growing
        # case's five: scan 1 gives the last but one up so that scan 2's set differs)
        assert {0, c.L - 1, 6, 30} <= set(sets[0]) and (c.kind == "range_grow" or c.L - 2 in sets[0]), (c.name, sets[0])
        assert {6, 30} <= set(sets[1]) and (c.kind == "range_grow" or {0, c.L - 1, c.L - 2} <= set(sets[1])), (c.name, sets[1])
        assert (4 + 2 * (c.L - 1)) // 64 == c.T - 1 and (3 + 2 * (c.L - 1)) // 64 == c.T - 2 and (3 + 2 * 30) % 64 == 63 and (3 + 2 * 6) % 16 == 15
        worst = max(worst, max(c.cond_S.values()))
    print(f"\nlargest cond(S): {worst:.3g}")
    assert worst < 1e5


def test_fp64_floor(all_cases, reference_runs):
    H.measure_floor(all_cases, reference_runs, RC.SUITE)
    print(f"recorded at: sigma {RC.FP64_FLOOR_SIGMA_CASE}, mu {RC.FP64_FLOOR_MU_CASE}")
    assert RC.SUITE.floor_sigma == RC.FP64_FLOOR_SIGMA and RC.SUITE.floor_mu == RC.FP64_FLOOR_MU


# ---- planted defects of a multi-tile range ----------------------------------------------------------------------------------------
DEFECTS = ("stale_hpt_panel", "stale_kn_panel", "last_tile_not_stored", "store_one_tile_on", "predict_skipped_mid_range", "class_a_mirrors_the_wrong_tile")


def _situation(defect, tl, classA):
    """Whether the tile list of one workgroup contains what the defect needs."""
    if defect == "stale_hpt_panel":
        return len(tl) >= 2 and tl[1][1] != tl[0][1]
    if defect == "stale_kn_panel":
        return len(tl) >= 2 and tl[1][0] != tl[0][0]
    if defect == "last_tile_not_stored":
        return len(tl) > DS.AHEAD + 1
    if defect == "store_one_tile_on":
        return len(tl) >= 2
    if defect == "predict_skipped_mid_range":
        return any(J == 0 for _, J in tl[1:])
    return classA and len(tl) == 2


def _inputs(c):
    """Scan 1 of a case in float64, as the downdate sees it: the stored P, the pending Predict's two factors, Kn = -K and
    HPt = (H P)^T (rows padded to whole tiles), and the pose block after the update."""
    n, T = c.n, c.T
    dt = c.events[0][1] - c.t
    vx, vy, w = c.vt
    th = float(c.mu[2])
    if c.model == FC.DIFF:
        half = th + w * dt / 2
        pa, pb = -vx * dt * math.sin(half), vx * dt * math.cos(half)
    else:
        pa, pb = -vx * dt * math.sin(th) - vy * dt * math.cos(th), vx * dt * math.cos(th) - vy * dt * math.sin(th)
    ek = FC.numpy_of(c)
    mu_p, P_p = ek.predict_state(c.events[0][1])
    pairs = [(l, g) for l, g in c.expect[0][0]]
    m = 2 * len(pairs)
    Hm = np.zeros((m, n))
    cs, sn = math.cos(mu_p[2]), math.sin(mu_p[2])
    for i, (_, g) in enumerate(pairs):
        dx, dy = mu_p[3 + 2 * g] - mu_p[0], mu_p[4 + 2 * g] - mu_p[1]
        Hm[2 * i, 0:3] = [-cs, -sn, -dx * sn + dy * cs]
        Hm[2 * i + 1, 0:3] = [sn, -cs, -dx * cs - dy * sn]
        Hm[2 * i: 2 * i + 2, 3 + 2 * g: 5 + 2 * g] = [[cs, sn], [-sn, cs]]
    W = P_p @ Hm.T
    K = W @ np.linalg.inv(Hm @ W + FC.OBS_COV * np.eye(m))
    Kn, HPt = np.zeros((64 * T, m)), np.zeros((64 * T, m))
    Kn[:n], HPt[:n] = -K, W
    P = np.zeros((64 * T, 64 * T))
    P[:n, :n] = c.P
    D = P_p - K @ W.T
    return dict(P=P, pa=pa, pb=pb, Kn=Kn, HPt=HPt, post=D[:3, :3], dense=D, n=n, T=T)


_ranges_of = {}


def _ranges(T, plan):
    """-> [(tile list, class A)] of the workgroups of a schedule that hold a tile."""
    if (T, plan) not in _ranges_of:
        grid = plan[0]
        lists = [(DS.device_tiles(T, *plan, b), DS.renumbered(grid, b) < T) for b in range(grid)]
        _ranges_of[(T, plan)] = [(tl, a) for tl, a in lists if tl]
    return _ranges_of[(T, plan)]


def emulate(inp, plan, defect=None):
    """P - Kn HPt^T tile by tile, every workgroup's range in the order tests/downdate_schedule.py gives, with the pipeline of
    dd_body: the panels are re-fetched only when the row / column changes, the Predict is applied to column-0 tiles as they are
    read, tile pos - 1 is stored while tile pos is computed, a diagonal tile (the last of a class-A range) mirrors its lower half.
    The output buffer starts as the stored P (what a tile that is never written keeps).  -> sigma, symmetric from the lower triangle."""
    T, n = inp["T"], inp["n"]
    grid, lo, x, sub = plan
    P, Kn, HPt = inp["P"], inp["Kn"], inp["HPt"]
    out = P.copy()

    def at(I, J):
        return slice(64 * I, 64 * I + 64), slice(64 * J, 64 * J + 64)

    for tl, classA in _ranges(T, plan):
        kI, hJ = tl[0]
        done = []
        for pos, (I, J) in enumerate(tl):
            if pos:
                pI, pJ = tl[pos - 1]
                if I != pI and not (defect == "stale_kn_panel" and pos == 1):
                    kI = I
                if J != pJ and not (defect == "stale_hpt_panel" and pos == 1):
                    hJ = J
            blk = P[at(I, J)].copy()
            if J == 0 and not (defect == "predict_skipped_mid_range" and pos > 0):
                r0 = 3 if I == 0 else 0
                c2 = blk[r0:, 2].copy()
                blk[r0:, 0] = blk[r0:, 0] + inp["pa"] * c2
                blk[r0:, 1] = blk[r0:, 1] + inp["pb"] * c2
            blk += Kn[64 * kI: 64 * kI + 64] @ HPt[64 * hJ: 64 * hJ + 64].T
            if I == 0 and J == 0:
                blk[:3, :3] = inp["post"]
            mirror = classA and (pos == len(tl) - 1)
            if defect == "class_a_mirrors_the_wrong_tile" and classA and len(tl) == 2:
                mirror = pos == 0
            if mirror:
                blk = np.tril(blk) + np.tril(blk, -1).T
            done.append(blk)
            if pos:
                out[at(*tl[pos if defect == "store_one_tile_on" else pos - 1])] = done[pos - 1]
        if not (defect == "last_tile_not_stored" and len(tl) > DS.AHEAD + 1):
            out[at(*tl[-1])] = done[-1]
    low = np.tril(out[:n, :n])
    return low + np.tril(low, -1).T


@pytest.fixture(scope="module")
def emulations(all_cases):
    """Per case (the K = 8 cases, the K = 32 one and the growing one): the inputs, the schedules and the clean emulation."""
    out = {}
    for c in all_cases:
        if c.kind == "range" and c.K not in (RC.K_DEFAULT, 32):
            continue
        inp = _inputs(c)
        plans = {"k_downdate2": DS.schedule(c.T, c.slots_alone, derived=c.kind == "range_grow")}
        if c.form_front != c.form_alone:
            plans["k_dd_front"] = DS.schedule(c.T, c.slots_front)
        nT = c.T * (c.T + 1) // 2
        single = DS.host_plan(c.T, 2 * nT + c.T)                          # more workgroups than tiles: one tile each
        assert all(len(DS.device_tiles(c.T, *single, b)) <= 1 for b in range(single[0]))
        out[c.name] = (c, inp, plans, single, emulate(inp, single))
    return out


def test_the_emulation_is_the_update(emulations):
    """Clean, the emulation is P_pred - K H P_pred whatever the schedule: bit-equal between schedules (a tile's arithmetic does not
    depend on who computes it), and equal to the dense product up to its rounding."""
    for name, (c, inp, plans, single, clean1) in emulations.items():
        ref = inp["dense"]
        ref = np.tril(ref) + np.tril(ref, -1).T
        assert np.abs(clean1 - ref).max() <= 1e-13 * np.abs(ref).max(), name
        for which, plan in plans.items():
            assert np.array_equal(emulate(inp, plan), clean1), (name, which)


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_bound_can_fail(defect, emulations):
    """Each defect, planted into every multi-tile schedule of the cases: at least 1000 x the GPU bound wherever the schedule holds the
    situation, and invisible at one tile per workgroup."""
    bound = FC.GPU_FACTOR * RC.FP64_FLOOR_SIGMA
    hit = 0
    for name, (c, inp, plans, single, clean) in emulations.items():
        assert np.array_equal(emulate(inp, single, defect), clean), (defect, name, "visible at one tile per workgroup")
        for which, plan in plans.items():
            there = sum(_situation(defect, tl, classA) for tl, classA in _ranges(c.T, plan))
            bad = emulate(inp, plan, defect)
            err = float(np.abs(bad - clean).max() / np.abs(clean).max())
            print(f"\n  {defect} on {name} ({which}, {there} ranges): sigma moves by {err:.3e} = {err / bound:.3g} x the GPU bound {bound:.2e}")
            if there:
                hit += 1
                assert err >= 1000 * bound, (defect, name, which, err)
            else:
                assert np.array_equal(bad, clean), (defect, name, which)
    assert hit >= 2, (defect, hit)
