"""Fleet filter, the shape sweep of k_fleet_step_fix / k_fleet_step_map / k_fleet_step_track, what can be checked without a GPU: the
tables of tests/fleet_narrow_sweep_cases.py cover what they claim, every margin holds, every CPU reference gives the claimed lists,
the two suites' FP64 floors are the measured ones, and six defects planted in a scratch copy of the witness -- slips of the code only
these compiles hold, which the hand-picked cases of tests/fleet_map_cases.py and tests/fleet_pose_cases.py see in few cases or in
none -- each exceed the GPU bound on EVERY new case they can act on."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as FM
from tests import fleet_narrow_sweep_cases as NC
from tests import fleet_pose_cases as PC
from tests.witness import fleet_wide_witness as WW
from tests.witness.fleet_witness import LDKIT, chol_inverse

pytestmark = pytest.mark.skipif(not WW.available(), reason="numpy.longdouble has no 64-bit mantissa here")

CLASSES = set(FC.M_CLASSES)


def by_residue(cases, key):
    out = {}
    for c in cases:
        out.setdefault(key(c), set()).add(c.n % 16)
    return out


# ---- the tables ----------------------------------------------------------------------------------------------------------------
def test_the_fix_table_is_what_it_claims():
    shapes = NC.fix_shapes()
    cases = [c for c in NC.fix_cases() if c.cls == "sweep"]
    assert len(shapes) == len(cases) == 72
    assert {((3 + 2 * L) % 16, FC.m_class(MM)) for L, MM, _N2, _m in shapes} == {(r, g) for r in NC.RESIDUES for g in CLASSES}
    for (L, MM, N2, model), c in zip(shapes, cases):
        sp, nw = c.expect[0]
        assert (c.L, len(sp), len(nw), c.model) == (L, MM, N2, model) and c.n == 3 + 2 * L == c.mu.shape[0] and MM + N2 <= 32, c.name
        assert len(c.events) == 2 and all(ev[4] is not None and len(ev[4]) == 3 for ev in c.events), (c.name, "every scan carries a fix")
        assert any(v != 0.0 for v in c.vt) and c.vt[0] > 0, c.name
        if L < 128:                                      # the follow-up scan appends one reflector and matches nothing: its fix is ignored
            assert c.expect[1] == ([], [0]), c.name
        else:
            assert c.expect[1] == ([(0, 0)], []), c.name
    n2 = by_residue(cases, lambda c: FC.n2_class(c.n, c.N2))
    assert sorted(n2) == sorted(NC.N2_CYCLE)
    for cls in NC.N2_CYCLE:
        assert len(n2[cls]) >= 4, (cls, n2[cls])
    assert sorted(c.n for c in NC.fix_cases() if c.n > NC.N_MAX) == [257, 259]
    assert all(c.MM == 32 and c.n >= 67 for c in cases if FC.m_class(c.MM) == ("0", 64) and c.MM == 32)
    models = [m for *_s, m in shapes]
    assert models[0::2] == [FC.DIFF] * 36 and models[1::2] == [FC.OMNI] * 36
    print(f"\n{len(cases)} fix shapes; appended rows: " + ", ".join(f"{k}: {sum(FC.n2_class(c.n, c.N2) == k for c in cases)}" for k in NC.N2_CYCLE))


def test_the_heading_shapes_are_what_they_claim():
    cases = [c for c in NC.fix_cases() if c.cls == "heading"]
    assert len(cases) == 4 and len({c.n % 16 for c in cases}) == 4 and all(c.n % 16 != 35 % 16 for c in cases)
    assert sorted(c.sign for c in cases) == [-1.0, -1.0, 1.0, 1.0] and {c.model for c in cases} == {FC.DIFF, FC.OMNI}
    for c in cases:
        predicted = FC.numpy_of(c).predict_state(c.events[0][1])[0][2]
        assert abs(predicted - c.sign * (math.pi - NC.HEADING_SHORT)) < 1e-12, c.name
        fix = c.events[0][4]
        assert fix[2] * c.sign < 0 and abs(abs(fix[2]) - (math.pi - NC.HEADING_TURN - NC.HEADING_FIX + NC.HEADING_SHORT)) < 1e-9, (c.name, fix)
        assert len(c.expect[0][0]) == c.MM > 0 and len(c.expect[0][1]) == c.N2 and c.expect[1] == ([], [0]) and c.events[1][4] is not None, c.name
        # phases C-F alone carry the heading across pi: the mean of the same scan WITHOUT its fix stands on the other side
        e = FC.numpy_of(c)
        e.handle_observation(c.events[0][1], c.events[0][3])
        assert e.mu[2] * c.sign < 0 and abs(e.mu[2]) > 3.0, (c.name, e.mu[2])


def test_the_map_table_is_what_it_claims():
    shapes = NC.map_shapes()
    cases = NC.map_cases()
    table = [c for c in cases if c.table == "map"]
    assert len(shapes) == NC.MAP_PER_NS * len(NC.MAP_NS) and len(table) == sum(len(s.variants) for s in shapes)
    assert sum(c.fixed for c in table) == 27 and sum(not c.fixed for c in table) == 54 and len(cases) == 81 + 6 + 8
    # every NS, each at five residues, with the boundary positions it stands for
    ns_res = by_residue(table, lambda c: c.NSn)
    assert sorted(ns_res) == list(NC.MAP_NS) and all(len(v) == NC.MAP_PER_NS for v in ns_res.values()), ns_res
    pos = {ns: NC.boundary_positions(ns) for ns in NC.MAP_NS}
    assert {p[0] for p in pos.values()} == {0, 2}, "2 NS on and inside a group of 4 rows"
    assert {p[1] for p in pos.values()} >= {0, 2, 4, 6, 14}, "2 NS on a tile's first row, behind it, inside, before its last pair"
    assert {p[2] for p in pos.values()} == {0, 1, 2, 3}, "2 NS in every tile of the 64 rows"
    assert pos[8] == (0, 0, 1) and pos[7] == (2, 14, 0) and pos[9] == (2, 2, 1) and pos[16] == (0, 0, 2) and pos[31] == (2, 14, 3)
    assert {c.n % 16 for c in table} == set(NC.RESIDUES)
    assert {FC.m_class(c.MM) for c in table} == CLASSES and any(c.MM == 32 and c.NSn < 31 for c in table) and all(c.MM <= 32 for c in table)
    n2 = by_residue(table, lambda c: FC.n2_class(c.n, c.N2))
    for cls in NC.MAP_N2_CYCLE:
        assert len(n2.get(cls, ())) >= 4, (cls, n2.get(cls))
    for c in table:
        sp, mp, nw = c.expect[0]
        assert (len(sp), len(mp), len(nw)) == (c.NSn, c.NMn, c.N2) and c.NMn >= 1 and c.use and len(sp) + len(mp) + len(nw) <= 32, c.name
        assert (c.events[0][4] is not None) == c.fixed and c.events[1][4] is None and len(c.expect[1][1]) == 1, c.name
        assert any(v != 0.0 for v in c.vt) and c.vt[0] > 0 and c.flags == 0, c.name
    # pure localisation that moves
    loc = [c for c in cases if c.table == "localise"]
    assert sorted((len(c.expect[0][1]), c.fixed) for c in loc) == [(nm, f) for nm in NC.LOCALISE_NM for f in (False, True)]
    assert all(c.n == 3 and c.L == 0 and c.vt[0] > 0 and c.use and not c.expect[0][0] and not c.expect[0][2] for c in loc)
    # plain members under the map compile
    unused = [c for c in cases if c.table == "unused"]
    assert sorted(c.n % 16 for c in unused) == list(NC.RESIDUES) and not any(c.use for c in unused) and sum(c.fixed for c in unused) == 4
    assert all(not c.expect[k][1] for c in unused for k in (0, 1))
    assert sorted(c.n for c in cases if c.n > NC.N_MAX) == [259, 259]
    members = NC.pattern_members()
    assert sorted(c.n % 16 for c in members) == list(NC.RESIDUES) and sum(c.fixed for c in members) == 4 and all(c.use for c in members)
    print(f"\n{len(table)} members on the map ({sum(c.fixed for c in table)} with a fix), {len(loc)} of pure localisation, {len(unused)} off the map")


def test_every_margin_holds():
    worst = (np.inf, "")
    for c in NC.fix_cases() + NC.map_cases():
        use = getattr(c, "use", False)
        for k in range(len(c.events)):
            assert len(c.margins[k]) == len(FC.kept_cloud(c, k)), c.name
            for a, b in c.margins[k]:
                assert a >= NC.MARGIN_MIN and b >= NC.MARGIN_MIN, (c.name, k, a, b)
                worst = min(worst, (min(a, b), f"{c.name} scan {k}"))
            if hasattr(c, "map_margins"):
                assert len(c.map_margins[k]) == (len(c.margins[k]) if use else 0), c.name
                for a, b, _inside in c.map_margins[k]:
                    assert a >= NC.MARGIN_MIN and b >= NC.MARGIN_MIN, (c.name, k, "map", a, b)
                    worst = min(worst, (min(a, b), f"{c.name} scan {k} (map)"))
    print(f"\nsmallest margin over {len(NC.fix_cases()) + len(NC.map_cases())} cases: {worst[0]:.4f} m at {worst[1]}")


# ---- the references --------------------------------------------------------------------------------------------------------------
def test_references_agree_on_every_case():
    """oracle/ekf_oracle.c, oracle/ekf_numpy.py and the suite's witness give the claimed lists on every scan (asserted inside
    fleet_harness.run_references / fleet_map_cases.run_references), and every scan of every case has a state."""
    for cases, runs in ((NC.fix_cases(), NC.fix_runs()), (NC.map_cases(), NC.map_runs())):
        for c in cases:
            assert sorted(runs[c.name]) == [0, 1], c.name


def test_fp64_floors():
    H.measure_floor(NC.fix_cases(), NC.fix_runs(), NC.FIX_SUITE)
    H.measure_floor(NC.map_cases(), NC.map_runs(), NC.MAP_SUITE)


# ---- planted defects ---------------------------------------------------------------------------------------------------------------
# map_pose_entries_c1_s0   the pose entries of a map pair's rows (h0[0:3], h1[0:3]) are built with c = 1, s = 0
# map_rows_at_mu           under fix_first the map pairs' dx, dy are taken at the mean the fix has moved (s_mu), not at s_mu0
# no_map_correction        under fix_first H (mu - mu0) is left out of the map rows' innovation
# boundary_row_3_wide      the first row that counts as a map row is 2 NS rounded down to a multiple of 4: with NS odd the last state
#                          pair's rows lose their landmark entries in W = P H^T and S
# pose_innovation_at_mu0   phase P behind phase F takes its innovation without -(mu1 - mu0)
# wrap_before_pose         the heading is normalised between phase E and phase P
DEFECTS = ("map_pose_entries_c1_s0", "map_rows_at_mu", "no_map_correction", "boundary_row_3_wide", "pose_innovation_at_mu0", "wrap_before_pose")


class DefectWitness(WW.BlockWitnessEKF):
    """A scratch copy of BlockWitnessEKF.handle_observation for a narrow scan (one block: the order of k_fleet_step_fix and
    k_fleet_step_map) with one of DEFECTS planted; with ``defect = None`` it gives that method's bits
    (test_the_scratch_copy_is_the_block_witness)."""
    defect = None

    def handle_observation(self, t, obs, gps_pose=None):
        obs = np.asarray(obs, np.float32).reshape(-1, 2)
        kit, defect = self.kit, self.defect
        self.predict(float(t) - self.time)
        self.time = float(t)
        self.last_match = ([], [], [])
        if obs.shape[0] == 0:
            return
        state, mapped, new = self.match3(obs, None)
        self.last_match = (state, mapped, new)
        pairs = state + mapped
        NSn, MM = len(state), len(pairs)
        assert MM <= WW.BLOCK_PAIRS
        if MM > 0:
            mu0 = self.mu.copy()
            kinds = [i >= NSn for i in range(MM)]
            on_map = self.map_xy.shape[0] > 0
            if gps_pose is not None:
                e, R = self._pose_rows(gps_pose, None)

            def pose_step():
                innov2 = e if defect == "pose_innovation_at_mu0" else e - (self.mu[0:3] - mu0[0:3])
                W2 = self.sigma[:, 0:3].copy()
                K2 = W2 @ chol_inverse(self.sigma[0:3, 0:3] + R, kit)
                self.mu = self.mu + K2 @ innov2
                self.sigma = self.sigma - K2 @ W2.T

            fix_first = gps_pose is not None and on_map
            if fix_first:
                pose_step()
            Hb, dz = self._rows_at(mu0, obs, pairs, kinds)
            if defect == "map_rows_at_mu" and fix_first:
                lin = mu0.copy()
                lin[0:2] = self.mu[0:2]                                    # (c and s stay those of mu0's heading: s_cs)
                Hm, dzm = self._rows_at(lin, obs, pairs, kinds)
                for i, of_map in enumerate(kinds):
                    if of_map:
                        Hb[2 * i: 2 * i + 2], dz[2 * i: 2 * i + 2] = Hm[2 * i: 2 * i + 2], dzm[2 * i: 2 * i + 2]
            if defect == "map_pose_entries_c1_s0":
                for i, ((_l, g), of_map) in enumerate(zip(pairs, kinds)):
                    if of_map:
                        dx = kit.T(float(self.map_xy[g, 0])) - mu0[0]
                        dy = kit.T(float(self.map_xy[g, 1])) - mu0[1]
                        Hb[2 * i, 0:3] = [kit.T(-1), kit.T(0), dy]
                        Hb[2 * i + 1, 0:3] = [kit.T(0), kit.T(-1), -dx]
            corr = Hb @ (self.mu - mu0)
            if defect == "no_map_correction" and fix_first:
                for i, of_map in enumerate(kinds):
                    if of_map:
                        corr[2 * i] = corr[2 * i + 1] = kit.T(0)
            dz = dz - corr
            m = Hb.shape[0]
            Hw = Hb
            if defect == "boundary_row_3_wide":
                Hw = Hb.copy()
                Hw[(2 * NSn) & ~3: 2 * NSn, 3:] = kit.T(0)
            W = self.sigma @ Hw.T
            Kt = W @ chol_inverse(Hw @ W + self.q * kit.eye(m), kit)
            self.mu = self.mu + Kt @ dz
            self.sigma = self.sigma - Kt @ W.T
            if gps_pose is not None and not on_map:
                if defect == "wrap_before_pose":
                    self.mu[2] = kit.wrap(self.mu[2])
                pose_step()
            self.mu[2] = kit.wrap(self.mu[2])
        if new:
            self._append(obs, new)


def witness_of(case, cls, defect=None):
    w = cls(case.model, case.t, case.mu[:3], FC.LIN_COV, FC.ANG_COV, FC.OBS_COV, kit=LDKIT)
    w.defect = defect
    w.set_state(case.t, case.mu, case.P, case.vt)
    if getattr(case, "use", False):
        w.set_map(case.map_xy, case.map_cov)
    return w


def factor(case, defect, ref, suite):
    """The defect's error on the case's first scan as a multiple of the GPU bound: the larger of the sigma and the mu figure."""
    k0 = next(k for k, ev in enumerate(case.events) if ev[0] == FC.EV_SCAN)
    w = witness_of(case, DefectWitness, defect)
    for ev in FC.reference_events(case)[:k0 + 1]:
        FC.feed(w, ev)
    es, em = H.rel_err(*w.state(), *ref[k0][0][0])
    bs, bm = H.bounds_within_tolerances(*ref[k0][0][0], suite)
    return max(es / bs, em / bm)


def test_the_scratch_copy_is_the_block_witness():
    fx, mp = NC.fix_cases(), NC.map_cases()
    picks = [fx[5], next(c for c in fx if c.cls == "heading"), next(c for c in mp if c.table == "map" and c.fixed and c.N2),
             next(c for c in mp if c.table == "map" and not c.fixed and c.NSn % 2), next(c for c in mp if c.table == "localise" and c.fixed),
             next(c for c in mp if c.table == "unused" and c.fixed)]
    for c in picks:
        a, b = witness_of(c, DefectWitness), witness_of(c, WW.BlockWitnessEKF)
        for ev in FC.reference_events(c):
            FC.feed(a, ev)
            FC.feed(b, ev)
            assert np.array_equal(a.mu, b.mu) and np.array_equal(a.sigma, b.sigma), c.name
        # and the block form is the suite's joint witness far below the GPU bound
        ref = (NC.fix_runs() if c in fx else NC.map_runs())[c.name][1][0][0]
        es, em = H.rel_err(*a.state(), *ref)
        assert es < 1e-13 and em < 1e-16, (c.name, es, em)


def new_pool(defect):
    """The new cases a defect can act on, with their runs and suite."""
    fx, mp = NC.fix_cases(), NC.map_cases()
    if defect == "map_pose_entries_c1_s0":
        return [c for c in mp if c.use], NC.map_runs(), NC.MAP_SUITE
    if defect in ("map_rows_at_mu", "no_map_correction"):
        return [c for c in mp if c.use and c.fixed], NC.map_runs(), NC.MAP_SUITE
    if defect == "boundary_row_3_wide":                      # (any member of a launch of the map compile, on the map or off it)
        return [c for c in mp if c.NSn % 2 == 1], NC.map_runs(), NC.MAP_SUITE
    if defect == "pose_innovation_at_mu0":
        return list(fx), NC.fix_runs(), NC.FIX_SUITE
    return [c for c in fx if c.cls == "heading"], NC.fix_runs(), NC.FIX_SUITE


_old = None


def old_cases():
    """The hand-picked cases the narrow fix and map paths had, with their suites' references: fleet_map_cases.all_cases() and
    fleet_pose_cases.shape_cases()."""
    global _old
    if _old is None:
        _old = [(c, FM.run_references(c), FM.SUITE) for c in FM.all_cases()] + [(c, H.run_references(c, PC.SUITE), PC.SUITE) for c in PC.shape_cases()]
    return _old


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_planted_defect_exceeds_the_gpu_bound_on_every_new_case_it_can_act_on(defect):
    pool, runs, suite = new_pool(defect)
    assert len(pool) >= 4, defect
    got = sorted((factor(c, defect, runs[c.name], suite), c.name) for c in pool)
    for f, name in got:
        print(f"  {defect} on {name}: {f:.3g} x the GPU bound")
    # (the rounded boundary exists in the map compile only: fleet_pose_cases' shapes run in k_fleet_step_fix and do not count for it)
    old = [o for o in old_cases() if defect != "boundary_row_3_wide" or o[2] is FM.SUITE]
    seen = [(c.name, f) for c, ref, st in old for f in [factor(c, defect, ref, st)] if f > 1]
    print(f"{defect}: over the bound on {sum(f > 1 for f, _ in got)} of {len(pool)} new cases, smallest factor {got[0][0]:.3g} at {got[0][1]}; "
          f"seen by {len(seen)} of {len(old)} hand-picked cases" + (": " + ", ".join(f"{n} ({f:.3g} x)" for n, f in seen) if seen else ""))
    assert got[0][0] > 1, (defect, got[0])


def test_the_defects_leave_the_cases_they_cannot_act_on_alone():
    """A planted defect changes no bit of a case outside its pool: the fix_first defects on a member without a fix, the rounded
    boundary on a member with an even number of state pairs."""
    mp = NC.map_cases()
    quiet = [("map_rows_at_mu", next(c for c in mp if c.table == "map" and not c.fixed)),
             ("no_map_correction", next(c for c in mp if c.table == "map" and not c.fixed)),
             ("boundary_row_3_wide", next(c for c in mp if c.table == "map" and c.NSn % 2 == 0 and c.NSn > 0))]
    for defect, c in quiet:
        a, b = witness_of(c, DefectWitness, defect), witness_of(c, DefectWitness)
        for w in (a, b):
            FC.feed(w, FC.reference_events(c)[0])
        assert np.array_equal(a.mu, b.mu) and np.array_equal(a.sigma, b.sigma), (defect, c.name)
