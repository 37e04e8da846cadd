"""Fleet filter, the shape sweep of the wide scans, what can be checked without a GPU: the tables of tests/fleet_wide_sweep_cases.py
cover what they claim, every margin holds, every CPU reference gives the claimed lists, the block form of the witness equals the
joint form, the suite's FP64 floors are the measured ones, and six planted block-form defects -- slips the 24 hand-picked cases of
tests/fleet_wide_cases.py cannot all see -- each exceed the GPU bound on at least one new case."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as FM
from tests import fleet_wide_cases as WC
from tests import fleet_wide_sweep_cases as SC
from tests.witness import fleet_wide_witness as WW
from tests.witness.fleet_witness import LDKIT, chol_inverse

pytestmark = pytest.mark.skipif(not WW.available(), reason="numpy.longdouble has no 64-bit mantissa here")


# ---- the tables ----------------------------------------------------------------------------------------------------------------
def plain():
    return [c for c in SC.sweep_cases() if c.kind == "wsweep"]


def test_every_case_is_what_its_shape_says():
    shapes = SC.sweep_shapes()
    cases = plain()
    assert len(cases) == len(shapes)
    for s, c in zip(shapes, cases):
        sp, mp, nw = c.expect[0]
        kept = min(s.N2, s.cap - s.L)
        assert (c.L, len(sp), len(mp), len(nw)) == (s.L, s.MM, 0, kept) and c.mu.shape[0] == 3 + 2 * s.L == c.n, c.name
        assert len(c.events[0][3]) == s.MM + s.N2 and 32 < s.MM + s.N2 <= 256 and c.model == s.model and not c.use, c.name
        assert s.cls in SC.N2_CLASSES and s.cls in SC.n2_classes(s.L, s.N2, s.cap), (c.name, s.cls)
        assert c.flags == (FC.FLAG_CAPACITY if s.cls == "over_capacity" else 0), c.name
        if s.cls == "over_capacity":
            assert c.kept[0] == sorted([q for q, _ in sp] + nw) and len(c.kept[0]) < len(c.events[0][3]) and s.L + kept == s.cap, c.name
        if s.cls == "to_capacity":
            assert s.L + len(nw) == c.max_landmarks == SC.CAP_SMALL and 0 not in c.kept, c.name
        assert any(v != 0.0 for v in c.vt) and c.vt[0] > 0 and len(c.events) == 2 and len(c.events[1][3]) <= 2, c.name
        assert len({j for _, j in sp}) == min(s.L, s.MM), c.name                    # MM > L: every reflector is seen, some several times
    assert sum(c.n > 163 for c in SC.all_cases()) <= 2 and all(6 <= s.L <= 80 for s in shapes)


def test_the_plain_table_covers_what_it_claims():
    shapes = SC.sweep_shapes()
    groups = SC.m_groups()
    assert sorted(v for vs in groups.values() for v in vs) == list(SC.MMLAST_LISTED) and len(groups) == 13
    seen, lasts, blocks, by_class = set(), set(), {}, {}
    for s in shapes:
        nb, last = SC.last_block(s.MM)
        res = (3 + 2 * s.L) % 16
        seen.add((res, SC.m_group(last)))
        lasts.add(last)
        blocks[nb] = blocks.get(nb, 0) + 1
        by_class.setdefault(s.cls, set()).add(res)
    residues = (1, 3, 5, 7, 9, 11, 13, 15)
    assert seen >= {(r, g) for r in residues for g in groups}, "every residue meets every group of the last block"
    assert lasts == set(SC.MMLAST_LISTED)
    assert sorted(blocks) == [2, 3, 5] and blocks[5] == 1 and min(blocks[2], blocks[3]) >= 40
    five = next(s for s in shapes if SC.last_block(s.MM)[0] == 5)
    assert 129 <= five.MM <= 160 and 3 + 2 * five.L <= 67
    for cls in SC.N2_CLASSES:
        assert len(by_class.get(cls, ())) >= 4, (cls, by_class.get(cls))
    assert any(s.N2 > 32 and SC.last_block(s.MM)[0] == 3 for s in shapes)
    models = [s.model for s in shapes[:-1]]
    assert models[0::2] == [FC.DIFF] * len(models[0::2]) and models[1::2] == [FC.OMNI] * len(models[1::2])
    print(f"\n{len(shapes)} plain shapes: blocks {blocks}; classes " + ", ".join(f"{k}: {sum(s.cls == k for s in shapes)}" for k in SC.N2_CLASSES))


def test_the_map_table_and_the_fixes_cover_what_they_claim():
    on_map = [c for c in SC.sweep_cases() if c.use]
    assert sorted({c.NSn for c in on_map}) == list(SC.MAP_NS)
    for ns in SC.MAP_NS:
        pair = [c for c in on_map if c.NSn == ns]
        assert sorted(c.fixed for c in pair) == [False, True], ns
        for c in pair:
            sp, mp, nw = c.expect[0]
            nb, last = SC.last_block(len(sp) + len(mp))
            assert len(sp) == ns and nb in (2, 3) and last in SC.MMLAST_LISTED and len(mp) > 0, c.name
            assert (c.events[0][4] is not None) == c.fixed, c.name
    assert len({c.n % 16 for c in on_map}) >= 4
    assert any(len({j for _, j in c.expect[0][1]}) < len(c.expect[0][1]) for c in on_map), "map points seen twice"
    third_mixed = [c for c in on_map if c.NSn > 64 and len(c.expect[0][0]) + len(c.expect[0][1]) > 64]
    assert third_mixed, "a third block with state and map rows"
    fixed_plain = [c for c in SC.sweep_cases() if c.fixed and not c.use]
    assert len(fixed_plain) == 4 and all(c.events[0][4] is not None and SC.last_block(c.MM)[0] >= 2 for c in fixed_plain)
    assert sum(abs(c.mu[2] + c.vt[2] * 0.1 - (math.pi - 5e-4)) < 1e-12 for c in fixed_plain) == 1
    two = [c for c in SC.all_cases() if c.kind == "wtwo"]
    assert [c.n % 16 for c in two] == [15, 1, 9]
    for c in two:
        (s0, m0, n0), (s1, m1, n1), _ = (c.expect[k] for k in range(3))
        assert len(s0) + len(m0) > 32 and len(c.events[1][3]) > 32 and len(n0) and len(n1) and len(c.events[2][3]) <= 32, c.name
        assert {j for _, j in s1} >= set(range(c.L, c.L + len(n0))), (c.name, "scan 1 matches what scan 0 appended")
    assert len({c.n % 16 for c in SC.track_members()}) == 8
    assert sum(c.use for c in SC.track_members()) >= 2 and sum(c.fixed for c in SC.track_members()) >= 2


def test_every_margin_holds():
    worst = (np.inf, "")
    for c in SC.all_cases():
        for k in range(len(c.events)):
            assert len(c.margins[k]) == len(FC.kept_cloud(c, k)), c.name
            for a, b in c.margins[k]:
                assert a >= SC.MARGIN_MIN and b >= SC.MARGIN_MIN, (c.name, k, a, b)
                worst = min(worst, (min(a, b), f"{c.name} scan {k}"))
            assert len(c.map_margins[k]) == (len(c.margins[k]) if c.use else 0), c.name
            for a, b, inside in c.map_margins[k]:
                assert a >= SC.MARGIN_MIN and b >= SC.MARGIN_MIN, (c.name, k, "map", a, b)
                worst = min(worst, (min(a, b), f"{c.name} scan {k} (map)"))
    print(f"\nsmallest margin over {len(SC.all_cases())} cases: {worst[0]:.4f} m at {worst[1]}")


# ---- the references --------------------------------------------------------------------------------------------------------------
def test_references_agree_on_every_case():
    """oracle/ekf_oracle.c, oracle/ekf_numpy.py, the joint witness and the block witnesses (longdouble and FP64) give the claimed
    lists on every scan (asserted inside runs()), and every scan of every case has a state."""
    runs = SC.runs()
    for c in SC.all_cases():
        assert sorted(runs[c.name]) == list(range(len(c.events))), c.name


def test_fp64_floor():
    WC.measure_floor(SC.all_cases(), SC.runs(), SC.SUITE)


def test_block_form_is_joint_form():
    worst_s, worst_m = (0.0, ""), (0.0, "")
    for c in SC.all_cases():
        for k, (wits, *_rest) in SC.runs()[c.name].items():
            es, em = H.rel_err(*wits[1], *wits[0])
            worst_s, worst_m = max(worst_s, (es, f"{c.name} scan {k}")), max(worst_m, (em, f"{c.name} scan {k}"))
    print(f"\nblock form vs joint form, longdouble: sigma {worst_s[0]:.3e} at {worst_s[1]}; mu {worst_m[0]:.3e} at {worst_m[1]}")
    assert worst_s[0] <= SC.BLOCK_VS_JOINT_SIGMA and worst_m[0] <= SC.BLOCK_VS_JOINT_MU
    assert SC.BLOCK_VS_JOINT_SIGMA < SC.FP64_FLOOR_SIGMA / 100 and SC.BLOCK_VS_JOINT_MU < SC.FP64_FLOOR_MU / 10


def test_the_lists_hold_behind_an_odometry_message():
    """The GPU suite puts an odometry message (the state's velocity again, half a step on) in front of the scans of the two-wide
    cases and of the track members: Predict then takes two half steps, and every claimed list is still what oracle/ekf_numpy.py
    gives."""
    for c in [c for c in SC.all_cases() if c.kind == "wtwo"] + SC.track_members():
        e = FM.numpy_of(c)
        e.handle_odometry(c.t + 0.05, *c.vt)
        for k, ev in enumerate(FC.reference_events(c)):
            FC.feed(e, ev)
            got = FM.map_back3(c, k, e.last_match[1], e.last_match[0], e.last_match[2])
            for a, b in zip(got, FM.want_lists(c, k)):
                assert np.array_equal(a, b), (c.name, k)


# ---- planted defects ---------------------------------------------------------------------------------------------------------------
# mu0_before_predict   the linearisation point s_mu0 is copied in front of Predict: rows, h and the correction stand at the old mean
#                      (block 0 of a member without a fix in front is not corrected, as in the kernel)
# rows_in_fours        the last block's rows are counted in fours: with m % 4 == 2 the padded row pair of W / Kn is the block before's
# row_width_rounded    a block that holds state AND map pairs is taken as all-state or all-map, whichever it holds more of
# no_map_correction    H_b (mu_b - mu0) is left out of the map rows' innovation
# augment_at_mu0       Gp and with it the new rows' cross terms and corner are taken at mu0's heading, not at the final mean's
# wrap_before_pose     the heading is normalised between the last block and phase P of a plain member with a fix
DEFECTS = ("mu0_before_predict", "rows_in_fours", "row_width_rounded", "no_map_correction", "augment_at_mu0", "wrap_before_pose")


class DefectWitness(WW.BlockWitnessEKF):
    """A scratch copy of BlockWitnessEKF.handle_observation with one of DEFECTS planted; with ``defect = None`` it is that method,
    statement by statement (test_the_scratch_copy_is_the_block_witness)."""
    defect = None

    def _append_at(self, obs, new, th):
        kit, LD = self.kit, self.kit.T
        N, N2 = self.mu.shape[0], len(new)
        xe, Sg = kit.zeros(N + 2 * N2), kit.zeros((N + 2 * N2, N + 2 * N2))
        xe[:N], Sg[:N, :N] = self.mu, self.sigma
        c, s = LD(math.cos(th)), LD(math.sin(th))
        Gp = kit.zeros((2 * N2, 3))
        for i, l in enumerate(new):
            gx, gy = self.to_global(obs[l])
            xe[N + 2 * i], xe[N + 2 * i + 1] = LD(float(gx)), LD(float(gy))
            rx, ry = LD(float(obs[l, 0])), LD(float(obs[l, 1]))
            Gp[2 * i] = [LD(1), LD(0), -rx * s - ry * c]
            Gp[2 * i + 1] = [LD(0), LD(1), rx * c - ry * s]
        Smx = Gp @ self.sigma[0:3, :]
        Smm = Gp @ self.sigma[0:3, 0:3] @ Gp.T
        for i in range(N2):
            for j in range(N2):
                Smm[2 * i: 2 * i + 2, 2 * j: 2 * j + 2] += self.q * kit.eye(2)       # Gz q I Gz^T = q I at any heading
        Sg[N:, :N], Sg[:N, N:], Sg[N:, N:] = Smx, Smx.T, Smm
        self.mu, self.sigma = xe, Sg

    def handle_observation(self, t, obs, gps_pose=None):
        obs = np.asarray(obs, np.float32).reshape(-1, 2)
        kit, defect = self.kit, self.defect
        before = self.mu.copy()
        self.predict(float(t) - self.time)
        self.time = float(t)
        self.last_match = ([], [], [])
        if obs.shape[0] == 0:
            return
        state, mapped, new = self.match3(obs, None)
        self.last_match = (state, mapped, new)
        pairs = state + mapped
        NSn, MM = len(state), len(pairs)
        mu0 = self.mu.copy()
        if MM > 0:
            lin = before if defect == "mu0_before_predict" else mu0
            kinds = [i >= NSn for i in range(MM)]
            H0, h0 = self._rows_at(lin, obs, pairs, kinds)
            on_map = self.map_xy.shape[0] > 0
            if gps_pose is not None:
                e, R = self._pose_rows(gps_pose, None)

            def pose_step():
                innov2 = e - (self.mu[0:3] - mu0[0:3])
                W2 = self.sigma[:, 0:3].copy()
                K2 = W2 @ chol_inverse(self.sigma[0:3, 0:3] + R, kit)
                self.mu = self.mu + K2 @ innov2
                self.sigma = self.sigma - K2 @ W2.T

            fix_first = gps_pose is not None and on_map
            if fix_first:
                pose_step()
            nb = (MM + WW.BLOCK_PAIRS - 1) // WW.BLOCK_PAIRS
            W_prev = K_prev = None
            for b in range(nb):
                lo, hi = WW.BLOCK_PAIRS * b, min(WW.BLOCK_PAIRS * b + WW.BLOCK_PAIRS, MM)
                kb = kinds[lo:hi]
                if defect == "row_width_rounded" and 0 < NSn - lo < hi - lo:
                    kb = [2 * (NSn - lo) < hi - lo] * (hi - lo)
                    Hb, dz = self._rows_at(lin, obs, pairs[lo:hi], kb)
                else:
                    Hb, dz = H0[2 * lo: 2 * hi], h0[2 * lo: 2 * hi].copy()
                corr = Hb @ (self.mu - lin)
                if defect == "no_map_correction":
                    for i, of_map in enumerate(kb):
                        if of_map:
                            corr[2 * i] = corr[2 * i + 1] = kit.T(0)
                if defect != "mu0_before_predict" or fix_first or b > 0:
                    dz = dz - corr
                m = Hb.shape[0]
                W = self.sigma @ Hb.T
                Kt = W @ chol_inverse(Hb @ W + self.q * kit.eye(m), kit)
                self.mu = self.mu + Kt @ dz
                D = Kt @ W.T
                if defect == "rows_in_fours" and b == nb - 1 and b > 0 and m % 4 == 2:
                    D = D + np.outer(K_prev[:, m], W_prev[:, m]) + np.outer(K_prev[:, m + 1], W_prev[:, m + 1])
                self.sigma = self.sigma - D
                W_prev, K_prev = W, Kt
            if gps_pose is not None and not on_map:
                if defect == "wrap_before_pose":
                    self.mu[2] = kit.wrap(self.mu[2])
                pose_step()
            self.mu[2] = kit.wrap(self.mu[2])
        if new:
            if defect == "augment_at_mu0":
                self._append_at(obs, new, float(mu0[2]))
            else:
                self._append(obs, new)


def defect_witness_of(case, defect, kit=None):
    w = DefectWitness(case.model, case.t, case.mu[:3], FC.LIN_COV, FC.ANG_COV, FC.OBS_COV, kit=kit or LDKIT)
    w.defect = defect
    w.set_state(case.t, case.mu, case.P, case.vt)
    if case.use:
        w.set_map(case.map_xy, case.map_cov)
    return w


def factors(case, defect, ref, suite, kit=None):
    """-> (sigma error, mu error) of the defect on the case's scan 0 as multiples of the GPU bound."""
    w = defect_witness_of(case, defect, kit)
    FC.feed(w, FC.reference_events(case)[0])
    es, em = H.rel_err(*w.state(), *ref)
    bs, bm = H.bounds_within_tolerances(*ref, suite)
    return es / bs, em / bm


def test_the_scratch_copy_is_the_block_witness():
    picks = [next(c for c in SC.sweep_cases() if c.fixed and not c.use), next(c for c in SC.sweep_cases() if c.fixed and c.use),
             next(c for c in SC.sweep_cases() if c.use and not c.fixed and c.N2), next(c for c in plain() if c.cls == "panels3")]
    for c in picks:
        w = defect_witness_of(c, None)
        FC.feed(w, FC.reference_events(c)[0])
        mu, P = SC.runs()[c.name][0][0][1]
        assert np.array_equal(w.mu, mu) and np.array_equal(w.sigma, P), c.name
    # augment_at_mu0's own append, given the final heading, is the witness's append
    c = picks[3]
    w = defect_witness_of(c, None)
    w._append = lambda obs, new: w._append_at(obs, new, float(w.mu[2]))
    FC.feed(w, FC.reference_events(c)[0])
    es, em = H.rel_err(*w.state(), *SC.runs()[c.name][0][0][1])
    assert es < 1e-15 and em == 0.0          # (q (c^2 + s^2) against q with FP64 cos / sin: 2^-52 q / max|sigma|)


def defect_pool(defect):
    """The new cases a defect can act on."""
    cases = SC.sweep_cases()
    if defect == "rows_in_fours":
        pool = [c for c in cases if SC.last_block(c.MM)[1] % 2 == 1]
    elif defect == "row_width_rounded":
        pool = [c for c in cases if c.use and c.NSn % 32]
    elif defect == "no_map_correction":
        pool = [c for c in cases if c.use]
    elif defect == "augment_at_mu0":
        pool = [c for c in cases if len(c.expect[0][2]) > 0]
    elif defect == "wrap_before_pose":
        pool = [c for c in cases if c.fixed and not c.use]
    else:
        pool = list(cases)
    return pool


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_planted_defect_exceeds_the_gpu_bound_on_a_new_case(defect):
    caught = []
    pool = defect_pool(defect)
    for c in pool:
        fs, fm = factors(c, defect, SC.runs()[c.name][0][0][0], SC.SUITE)
        print(f"  {defect} on {c.name}: sigma {fs:.3g} x the GPU bound, mu {fm:.3g} x")
        if fs > 1 or fm > 1:
            caught.append((max(fs, fm), c.name))
    assert caught, defect
    print(f"{defect}: caught on {len(caught)} of {len(pool)} new cases, smallest factor over the bound {min(caught)[0]:.3g} at {min(caught)[1]}")


def test_what_the_hand_picked_cases_see_of_the_planted_defects():
    """The same defects over fleet_wide_cases.all_cases() (FP64 arithmetic for the scratch copy: a factor is a defect's only where it
    is far above 1): printed, and the two the issue names as invisible there are asserted so."""
    seen = {}
    for defect in DEFECTS:
        hits = []
        for c in WC.all_cases():
            fs, fm = factors(c, defect, WC.runs()[c.name][0][0][0], WC.SUITE, kit=WW.F64Kit())
            if max(fs, fm) > 1:
                hits.append((c.name, max(fs, fm)))
        seen[defect] = hits
        print(f"  {defect}: caught by {len(hits)} of {len(WC.all_cases())} hand-picked cases" +
              (": " + ", ".join(f"{n} ({f:.3g} x)" for n, f in hits) if hits else ""))
    moving = {c.name for c in WC.all_cases() if any(v != 0.0 for v in c.vt)}
    assert {n for n, _ in seen["mu0_before_predict"]} <= moving, "a case that stands still cannot see mu0 taken in front of Predict"
    assert not seen["wrap_before_pose"], "no hand-picked plain member with a fix has its heading carried across pi"
