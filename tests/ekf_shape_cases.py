"""Cases of the single filter's shape sweep, shared by tests/test_ekf_shapes_cpu.py (the cases and the three CPU references
against each other, the FP64 floor, the planted defects) and tests/test_ekf_shapes_gpu.py (every launch form of the single
filter -- k_mid<NBR, MODE>, k_downdate2 / k_dd_front / the downdate role inside k_mid, k_augment, the front end -- against the
longdouble witness).  The record, the helpers and the margins are those of tests/fleet_cases.py; a case here carries in
addition ``cap`` (the handle's capacity), ``auto_grow`` and ``flags``.  numpy only, deterministic seeds.

A case is a random dense SPD state (fleet_cases.dense_spd, the scale range of fleet_cases.sweep_case) over reflectors on a
jittered 2 m lattice of 16 x 16 cells (float32-exact), one non-zero vt, scans 0.1 s apart.  Every observation is within 2 mm
of a chosen reflector's current mean, or a free lattice cell.  Both association margins of every observation of every scan are
asserted at generation (>= MARGIN_MIN); no case is excused.

Four scans, so that every stage of the one-launch pipeline is met on a dense state:
    scan 1   the case's K and matched set                          nothing pending
    scan 2   the same reflectors in another observation order      the write-ahead panel of scan 1 is taken (a hit)
    scan 3   another matched set of the same size                  a miss: the update computes the pending correction itself
    scan 4   part of scan 3's set, one reflector observed 3 times  duplicate H row pairs, fewer reflectors than pairs (a miss
                                                                   too: a panel is taken only for the SAME set of reflectors)
The matched sets hold, where L allows: reflector 0, reflector L - 1, the first reflector whose two rows straddle a 16-row
workgroup edge of k_mid (3 + 2 j = 15 mod 16: j = 6, 14, ...), one that straddles a 64-row tile edge of the downdate
(j = 30, 62, ...) and L - 2 (inside the last, partly filled workgroup).  Scan 4's triple observation is the 16-row straddler.

Kinds:
    sweep      a full filter (cap = L, auto-grow off): MODE 0 / 3 of k_mid, the one-launch pipeline.  L around the 16-row edges
               (6, 7, 14, 15), around the 64-row tiles and their 1 / 3 / 5-row borders (30 .. 33, 62 .. 65), 94, 95, 126 .. 128,
               34 .. 37 (the n mod 16 residues the others leave out), 160 and 200; K over 1, 2, 3, 8, 15, 16 | 17, 24, 31, 32
               (the host picks NBR from 2 K: 16 | 17 is the switch).  160 and 200 have T = 6 and 7 tile rows: on 256 CUs the
               static schedule hands every class-B workgroup ONE tile there (downdate_schedule, dd_sub = 1), so the generic
               tile loop (more than four tiles per workgroup, n beyond ~2900) is not reached at these sizes; what 160 and 200
               add is more than four tile rows in the straight-line form and in the queue of the in-launch downdate role.
    capacity   a full filter, K observations of which only MM match; the others are far and dropped (``kept``), flag CAPACITY.
    growing    cap = L + 8, auto-grow off: never full (MODE 1, k_augment, the early n).  Scan 1 carries N2 new observations
               between the matched ones; n = 3 + 2 L = 15 mod 16 for every L of this kind, so the classes of fleet_cases.n2_for
               against the 16-row edge are N2 = 0 (edge: the last row is row n16 - 2 already), 1 (straddle: x in row n16 - 1,
               y in the next workgroup) and 3 (cross); for L = 30 and 62 that edge is a 64-row tile edge too.  Scans 2 - 4 are on
               the grown state.  One auto-grow case: cap 8 at L = 7 with 4 new reflectors has to double its capacity.
    wide       a full filter, L = 128 and 200, one scan of K = 33 (the second block step holds one pair), 64 (two full steps,
               by value) and 65 (three steps, staged through HBM), then a scan of 2.
    pose       every scan with a pose fix (gps_pose), which the single filter applies jointly with the reflector rows:
               K = 14 | 15 on L = 31 (31 | 33 rows: the NBR switch), K = 30 on L = 64 (63 rows in one pass), K = 31 on L = 64
               (65 rows: block steps with stride 30).  The witness is tests/witness/fleet_pose_witness.py, joint form.

Pre-loaded maps (set_map) are the subject of tests/ekf_map_cases.py, which builds its cases with this module's Builder: a scan
may carry observations of map points (``map_ids``), and a case with a map claims three lists per scan, ``expect[k] =
(state_pairs, map_pairs, new_ids)``, as tests/fleet_map_cases.py does (claim3 reads either form).

Out of scope: exclusive handles (k_mid<*, 2>): no counter proves that path ran, and it is the one form in which a workgroup
waits for another.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

from tests import fleet_cases as FC
from tests.fleet_cases import DIFF, EV_SCAN, MARGIN_MIN, OMNI, _case, dense_spd, feed, margins, reference_events, to_local
from tests.fleet_map_cases import map_margins

GRID, PITCH, JITTER = 16, 2.0, 0.2           # 256 lattice cells, reflectors at least 1.6 m apart
T0, DT = 100.0, 0.1
FIX_SIGMA = (0.05, 0.05, 0.017)

# ---- the FP64 noise floor of these cases -------------------------------------------------------------------------------------
# Measured by tests/test_ekf_shapes_cpu.py::test_fp64_floor (run it with -s) as tests/test_fleet_edges_cpu.py does for the fleet:
# the larger error of oracle/ekf_oracle.c and oracle/ekf_numpy.py against the longdouble witness over every scan of every case
# below, as max|dsigma| / max|sigma_ref| and max|dmu| / max(1, max|mu_ref|).  Recorded = measured, rounded up to two digits; the
# test fails when a re-measurement exceeds it or falls below half of it.  The GPU bound is fleet_cases.GPU_FACTOR times these.
FP64_FLOOR_SIGMA = 1.1e-11    # measured 1.087e-11
FP64_FLOOR_MU = 2.5e-16       # measured 2.494e-16
FP64_FLOOR_SIGMA_CASE = "single_grow_L14_MM8_N3_omni scan 3 (oracle)"
FP64_FLOOR_MU_CASE = "single_grow_L30_MM24_N3_diff scan 2 (numpy)"


def witness_of(case):
    """The longdouble witness of a case: the plain one, or the pose witness (joint form) when a scan carries a fix."""
    if any(len(ev) > 4 and ev[4] is not None for ev in case.events):
        from tests.fleet_pose_cases import pose_witness_of
        return pose_witness_of(case, "joint")
    return FC.witness_of(case)


SUITE = NS(name="single", floor_sigma=FP64_FLOOR_SIGMA, floor_mu=FP64_FLOOR_MU, witnesses={"witness": witness_of})


# ---- where the matched reflectors sit ------------------------------------------------------------------------------------------
def claim3(case, k):
    """-> (state pairs, map pairs, new ids) as scan k of `case` claims them; a case without a map claims no map pair."""
    e = case.expect[k]
    return (e[0], e[1], e[2]) if len(e) == 3 else (e[0], [], e[1])


def straddler16(L):
    """The first reflector whose rows 3 + 2 j, 4 + 2 j lie on either side of a 16-row edge; None below L = 7."""
    return 6 if L > 6 else None


def straddler64(L):
    return 30 if L > 30 else None


def musts(L):
    """Reflectors every matched set wants, in the order scan 1 takes them."""
    out = []
    for j in (0, L - 1, straddler16(L), straddler64(L), L - 2):
        if j is not None and 0 <= j < L and j not in out:
            out.append(j)
    return out


def triple_of(L):
    s = straddler16(L)
    return s if s is not None else 0


def matched_sets(L, MM, rng):
    """-> (set of scans 1 and 2, set of scan 3): MM distinct reflectors each, different as sets, scan 3's with the reflector that
    scan 4 observes three times."""
    assert 1 <= MM < L, (L, MM)
    want = musts(L)
    first = want[:MM]
    rest = [j for j in rng.permutation(L) if j not in first]
    first = first + [int(j) for j in rest[:MM - len(first)]]
    tri = triple_of(L)
    order3 = [tri] + [j for j in reversed(want) if j != tri]
    third = order3[:MM]
    rest = [int(j) for j in rng.permutation(L) if j not in third]
    # fill from reflectors scan 1 left out first, so that the sets differ wherever L allows
    rest.sort(key=lambda j: j in first)
    third = third + rest[:MM - len(third)]
    if set(third) == set(first):                           # (small L: scan 1 gives way, scan 3 keeps the triple's reflector)
        first[-1] = next(j for j in reversed(range(L)) if j not in third)
    assert len(set(first)) == len(set(third)) == MM and set(first) != set(third) and tri in third
    return first, third


# ---- one case ----------------------------------------------------------------------------------------------------------------------
class Builder:
    """Lays the scans of a case down one after the other on a run of oracle/ekf_numpy.py (the predicted pose and the current
    means of the reflectors are where the observations are placed)."""

    def __init__(self, L, model, seed, cap, auto_grow=False, n_map=0, map_cov=None, grid=GRID):
        """grid: the lattice has grid x grid cells (256 by default; tests/ekf_range_cases.py needs more reflectors than that).  Positions
        are float32 values whatever the lattice's size (pitch 2 m: below 2^7 m up to grid = 63, 2^-17 m apart there).
        n_map > 0: a pre-loaded map of that many points, free lattice cells (so at least 1.6 m from every reflector and every
        new point); map_cov: its weights (n_map x 4, row-major 2 x 2), identity when None."""
        rng = self.rng = np.random.default_rng(seed)
        self.L0, self.model, self.cap, self.auto_grow = L, model, cap, auto_grow
        n = 3 + 2 * L
        assert L < grid * grid <= 63 * 63
        cells = rng.permutation(grid * grid)
        pts = np.stack([cells % grid, cells // grid], -1) * PITCH + rng.uniform(-JITTER, JITTER, size=(grid * grid, 2))
        pts = pts.astype(np.float32).astype(np.float64)
        lm, free = pts[:L], pts[L:]
        if L >= 2:
            d = np.sort(np.hypot(lm[None, :, 0] - free[:, None, 0], lm[None, :, 1] - free[:, None, 1]), axis=1)
            free = free[d[:, 1] - d[:, 0] >= 0.05]            # new points: the two nearest reflectors are not nearly equidistant
        self.free = list(free)
        self.map_xy = self.map_cov = None
        if n_map:
            # the map takes the front of the free cells (new points come off the back); nothing is drawn for it
            self.map_xy = np.asarray(self.free[:n_map], np.float32).reshape(n_map, 2)
            self.free = self.free[n_map:]
            assert np.array_equal(self.map_xy.astype(np.float64), np.asarray(free[:n_map]))
            self.map_cov = np.tile(np.asarray((1.0, 0.0, 0.0, 1.0)), (n_map, 1)) if map_cov is None else np.asarray(map_cov, np.float64).reshape(n_map, 4)
        mu = np.zeros(n)
        mu[0:2] = 0.5 * grid * PITCH + rng.uniform(-1.5, 1.5, size=2)
        mu[2] = rng.uniform(-3.0, 3.0)
        mu[3:] = lm.reshape(-1)
        P = dense_spd(n, rng, 10.0 ** rng.uniform(-3.7, -2.3))     # as fleet_cases.sweep_case: diagonal 3e-4 .. 6e-3
        vt = (rng.uniform(0.2, 1.0), rng.uniform(-0.3, 0.3) if model == OMNI else 0.0, rng.uniform(-0.4, 0.4))
        self.mu, self.P, self.vt = mu, P, vt
        self.ek = FC.numpy_of(NS(model=model, t=T0, mu=mu, P=P, vt=vt))
        if n_map:
            self.ek.set_map(self.map_xy, self.map_cov)
        self.events, self.expect, self.kept, self.marg, self.map_marg = [], {}, {}, {}, {}
        self.fix_rng = None
        self.cond = None                      # a dict: cond(S) of every scan is recorded as the scan is laid down (else case() runs cond_S_of)

    def with_fixes(self, seed):
        self.fix_rng = np.random.default_rng(seed)
        return self

    def L(self):
        return (self.ek.mu.shape[0] - 3) // 2

    def scan(self, ids, far=0, avoid=None, map_ids=(), avoid_map=None):
        """One scan: an observation of each reflector of `ids` (in that order, repeats allowed), one of each map point of `map_ids`
        (the same) and `far` free cells, interleaved at random (not in the order `avoid` of reflectors, nor `avoid_map` of map
        points).  On a full filter the far ones are dropped, on any other they become reflectors."""
        rng, ek, k = self.rng, self.ek, len(self.events)
        t = T0 + DT * (k + 1)
        mu_p, P_p = ek.predict_state(t)
        pose = tuple(float(v) for v in mu_p[:3])
        n_s, n_m = len(ids), len(map_ids)
        assert n_m == 0 or self.map_xy is not None
        K = n_s + n_m + far
        while True:
            slots = rng.permutation(K)
            if avoid_map is not None and n_m >= 2 and [int(map_ids[s - n_s]) for s in slots if n_s <= s < n_s + n_m] == avoid_map:
                continue
            if avoid is None or len(ids) < 2 or [int(ids[s]) for s in slots if s < len(ids)] != avoid:
                break
        full = not self.auto_grow and self.L() == self.cap
        # (what a full filter drops never enters the state: the same free cells serve every scan)
        cells = [self.free[i] for i in range(far)] if full else [self.free.pop() for _ in range(far)]
        cloud = np.zeros((K, 2), np.float32)
        pairs, mpairs, new = [], [], []
        for q in range(K):
            if slots[q] < n_s:
                j = int(ids[slots[q]])
                g = ek.mu[3 + 2 * j: 5 + 2 * j] + rng.uniform(-2e-3, 2e-3, size=2)
                pairs.append((q, j))
            elif slots[q] < n_s + n_m:
                j = int(map_ids[slots[q] - n_s])
                g = self.map_xy[j].astype(np.float64) + rng.uniform(-2e-3, 2e-3, size=2)
                mpairs.append((q, j))
            else:
                g = cells[slots[q] - n_s - n_m]
                new.append(q)
            cloud[q] = to_local(pose, g)
        fix = None
        if self.fix_rng is not None:
            f = mu_p[:3] + self.fix_rng.normal(size=3) * FIX_SIGMA
            fix = (float(f[0]), float(f[1]), float(np.arctan2(np.sin(f[2]), np.cos(f[2]))))
        dropped = full and far > 0
        assert full or self.auto_grow or self.L() + far <= self.cap
        keep = sorted(q for q, _ in pairs + mpairs) if dropped else None
        if dropped:
            self.kept[k] = keep
        has_map = self.map_xy is not None
        self.expect[k] = (pairs, mpairs, [] if dropped else new) if has_map else (pairs, [] if dropped else new)
        kc = cloud if keep is None else np.ascontiguousarray(cloud[keep])
        self.marg[k] = margins(mu_p, kc)
        if self.cond is not None and pairs:
            self.cond[k] = float(np.linalg.cond(FC.innovation_cov(mu_p, P_p, pairs)))
        for a, b in self.marg[k]:
            assert a >= MARGIN_MIN and b >= MARGIN_MIN, (k, a, b)      # no case is excused
        if has_map:
            # the map branch's margins (fleet_map_cases.map_margins: over the weight's scale), of every observation of the scan
            self.map_marg[k] = map_margins(self, mu_p, kc)
            kept_q = range(K) if keep is None else keep
            for q, (a, b, inside) in zip(kept_q, self.map_marg[k]):
                assert a >= MARGIN_MIN and b >= MARGIN_MIN and inside == (q in {o for o, _ in mpairs}), (k, q, a, b, inside)
        self.events.append((EV_SCAN, t, (0.0, 0.0, 0.0), cloud) + ((fix,) if self.fix_rng is not None else ()))
        ek.handle_observation(t, kc, *(() if fix is None else (np.asarray(fix),)))
        got = ([tuple(int(v) for v in p) for p in ek.last_match[1]], [int(v) for v in ek.last_match[2]])
        want = FC.map_back(NS(kept=self.kept), k, *got)
        assert [tuple(p) for p in want[0].tolist()] == pairs and want[1].tolist() == self.expect[k][-1], (k, got, pairs, new)
        got_m = FC.map_back(NS(kept=self.kept), k, ek.last_match[0], [])[0]
        assert [tuple(p) for p in got_m.tolist()] == mpairs, (k, got_m.tolist(), mpairs)

    def four_scans(self, MM, far=(0, 0, 0, 0), first_new=0, Mm=0):
        """The sequence of the module docstring.  far[k]: far observations of scan k (a full filter drops them);
        first_new: new reflectors of scan 1 (a growing filter).  Mm: map points per scan (tests/ekf_map_cases.py): scans 1 and 2
        see map points 0 .. Mm - 1, scan 3 sees Mm .. 2 Mm - 1, scan 4 part of those with map point Mm three times (duplicate
        map rows); MM may then be 0 (map rows only)."""
        L = self.L0
        first, third = matched_sets(L, MM, self.rng) if MM else ([], [])
        m1, m3 = list(range(Mm)), list(range(Mm, 2 * Mm))
        self.scan(first, far[0] + first_new, map_ids=m1)
        Lg, pos = self.L(), MM - 1
        for j in ([Lg - 1, L] if Lg > L + 1 else [Lg - 1] if Lg > L else []):
            # the grown state: scan 3 matches the last reflector scan 1 appended and the first one (its rows straddle the edge)
            if pos >= 1 and j not in third:
                third[pos] = j
                pos -= 1
        self.scan(first, far[1], avoid=[g for _, g in self.expect[0][0]], map_ids=m1,
                  avoid_map=[g for _, g in self.expect[0][1]] if Mm else None)
        self.scan(third, far[2], map_ids=m3)
        # scan 4: max(3, MM) state observations and max(3, Mm) map observations, but no more pairs than the case's MM + Mm where
        # that leaves three of each kind (so that the scan stays on the launch form of the others)
        K4, K4m = (max(3, MM) if MM else 0), (max(3, Mm) if Mm else 0)
        over = max(0, K4 + K4m - (MM + Mm)) if Mm else 0
        if K4 >= K4m:
            K4 = max(3, K4 - over) if MM else 0
        else:
            K4m = max(3, K4m - over)
        ids4 = []
        if MM:
            tri = third[0]
            others = [j for j in third if j != tri][:K4 - 3]
            ids4 = [tri] + others[:len(others) // 2] + [tri] + others[len(others) // 2:] + [tri]
        else:
            tri = None
        self.scan(ids4, far[3], map_ids=([Mm] + m3[1:K4m - 2] + [Mm, Mm]) if Mm else ())
        self.sets = (first, third, tri)

    def case(self, name, kind, **tags):
        c = _case(name, kind, self.model, self.mu, self.P, self.vt, T0, self.events, self.expect,
                  max_landmarks=max(self.cap, self.L()), kept=self.kept, L=self.L0, n=3 + 2 * self.L0, cap=self.cap, **tags)
        if self.map_xy is not None:
            c.map_xy, c.map_cov, c.use, c.map_margins = self.map_xy, self.map_cov, True, self.map_marg
        c.margins = self.marg
        c.cond_S = cond_S_of(c) if self.cond is None else dict(self.cond)
        c.flags = FC.FLAG_CAPACITY if self.kept else 0
        c.auto_grow = self.auto_grow
        c.sets = getattr(self, "sets", None)
        return c


def cond_S_of(case):
    """cond(S) of every scan (reflector rows; read off when a case is far out) from a run of oracle/ekf_numpy.py."""
    out = {}
    ek = FC.numpy_of(case)
    if hasattr(case, "map_xy"):
        ek.set_map(case.map_xy, case.map_cov)
    for k, ev in enumerate(reference_events(case)):
        mu_p, P_p = ek.predict_state(ev[1])
        pairs = [(l, g) for l, g in np.asarray(case.expect[k][0]).reshape(-1, 2)]
        if pairs:
            out[k] = float(np.linalg.cond(FC.innovation_cov(mu_p, P_p, pairs)))
        feed(ek, ev)
    return out


def _m(model):
    return "diff" if model == DIFF else "omni"


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
L_LISTED = (6, 7, 14, 15, 30, 31, 32, 33, 62, 63, 64, 65, 94, 95, 126, 127, 128, 160, 200)
L_RESIDUES = (34, 35, 36, 37)                # n mod 16 = 7, 9, 11, 13: the residues the listed L leave out
K_LISTED = (1, 2, 3, 8, 15, 16, 17, 24, 31, 32)
# (L, K): every L with two K, one <= 16 and one >= 17 where L > 17; every K at three L or more; every n mod 16 with both NBR
SWEEP_SHAPES = [(6, 1), (6, 3), (7, 2), (7, 3), (14, 8), (14, 1), (15, 8), (15, 2),
                (30, 15), (30, 17), (31, 16), (31, 24), (32, 3), (32, 31), (33, 16), (33, 32),
                (62, 1), (62, 17), (63, 15), (63, 32), (64, 8), (64, 24), (65, 2), (65, 31),
                (94, 16), (94, 17), (95, 3), (95, 24), (126, 15), (126, 31), (127, 8), (127, 32), (128, 16), (128, 17),
                (160, 1), (160, 32), (200, 2), (200, 24), (200, 32),
                (34, 15), (34, 17), (35, 16), (35, 24), (36, 8), (36, 31), (37, 3), (37, 32)]
# (L, K, MM): a full filter on which only MM of K observations match
CAPACITY_SHAPES = [(31, 16, 1), (63, 16, 15), (30, 17, 1), (64, 17, 16), (127, 32, 1), (33, 32, 31)]
# (L, matched observations of scan 1, N2 class)
GROW_CLASSES = {"edge": 0, "straddle": 1, "cross": 3}
GROWING_SHAPES = [(6, 3, "edge"), (6, 2, "straddle"), (6, 3, "cross"), (14, 8, "edge"), (14, 1, "straddle"), (14, 8, "cross"),
                  (30, 15, "edge"), (30, 17, "straddle"), (30, 24, "cross"), (62, 16, "edge"), (62, 31, "straddle"), (62, 17, "cross"),
                  (126, 24, "edge"), (126, 8, "straddle"), (126, 29, "cross")]
WIDE_SHAPES = [(128, 33), (128, 64), (128, 65), (200, 33), (200, 64), (200, 65)]
POSE_SHAPES = [(31, 14), (31, 15), (64, 30), (64, 31)]


def sweep_case(i, L, K):
    model = DIFF if i % 2 == 0 else OMNI
    b = Builder(L, model, 9100 + i, cap=L)
    b.four_scans(K)
    return b.case(f"single_L{L}_K{K}_{_m(model)}", "sweep", K=K, MM=K, N2=0)


def capacity_case(i, L, K, MM):
    model = DIFF if i % 2 == 0 else OMNI
    b = Builder(L, model, 9200 + i, cap=L)
    b.four_scans(MM, far=(K - MM,) * 3 + (K - max(3, MM),))       # (scan 4 has max(3, MM) pairs)
    return b.case(f"single_full_L{L}_K{K}_MM{MM}_{_m(model)}", "capacity", K=K, MM=MM, N2=0)


def growing_case(i, L, MM, cls):
    model = DIFF if i % 2 == 0 else OMNI
    N2 = GROW_CLASSES[cls]
    n = 3 + 2 * L
    n16 = (n + 15) & ~15
    assert n16 - n == 1 and {"edge": n == n16 - 1, "straddle": n + 2 * N2 == n16 + 1, "cross": n + 2 * N2 > n16 + 1}[cls]
    b = Builder(L, model, 9300 + i, cap=L + 8)
    b.four_scans(MM, first_new=N2)
    return b.case(f"single_grow_L{L}_MM{MM}_N{N2}_{_m(model)}", "growing", K=MM + N2, MM=MM, N2=N2, n2_class=cls)


def auto_grow_case():
    b = Builder(7, DIFF, 9390, cap=8, auto_grow=True)
    b.four_scans(3, first_new=4)
    return b.case("single_autogrow_L7_MM3_N4_diff", "growing", K=7, MM=3, N2=4, n2_class="cross")


def wide_case(i, L, K):
    model = DIFF if i % 2 == 0 else OMNI
    b = Builder(L, model, 9400 + i, cap=L)
    want = musts(L)
    ids = want + [int(j) for j in b.rng.permutation(L) if j not in want][:K - len(want)]
    b.scan(ids)
    b.scan([triple_of(L), L - 1])
    return b.case(f"single_wide_L{L}_K{K}_{_m(model)}", "wide", K=K, MM=K, N2=0)


def pose_case(i, L, K):
    model = DIFF if i % 2 == 0 else OMNI
    b = Builder(L, model, 9500 + i, cap=L).with_fixes(9550 + i)
    b.four_scans(K)
    return b.case(f"single_pose_L{L}_K{K}_{_m(model)}", "pose", K=K, MM=K, N2=0)


_cases = None


def cases():
    """Every case of this module, by kind: sweep, capacity, growing, wide, pose."""
    global _cases
    if _cases is None:
        _cases = ([sweep_case(i, *s) for i, s in enumerate(SWEEP_SHAPES)] + [capacity_case(i, *s) for i, s in enumerate(CAPACITY_SHAPES)] +
                  [growing_case(i, *s) for i, s in enumerate(GROWING_SHAPES)] + [auto_grow_case()] +
                  [wide_case(i, *s) for i, s in enumerate(WIDE_SHAPES)] + [pose_case(i, *s) for i, s in enumerate(POSE_SHAPES)])
    return _cases


def case_named(name):
    return next(c for c in cases() if c.name == name)
