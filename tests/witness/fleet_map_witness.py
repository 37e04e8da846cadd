"""tests/witness/fleet_map_witness.py -- TEST INFRASTRUCTURE: HandleObservationMessage WITH the pre-loaded map branch, dense and
literal in numpy.longdouble, as tests/witness/fleet_witness.py restates the plain update and fleet_pose_witness.py the pose rows.

Written from the reference's text (src/reflector_ekf_slam/reflector_ekf_slam.cc:397-453 ReflectorMatch, :246-305 the rows),
independently of oracle/ekf_oracle.c.  Predict, the state branch's distances, the pose rows, the Cholesky inverse, the append and
the number type come from the two witnesses this one extends.

  * ReflectorMatch is the SPECIFICATION and keeps its own number formats: per observation, if the map is not empty, the float32
    difference `map - g` (that order, :408), widened to FP64, the weighted distance sqrt((delta S) delta^T) with S the point's
    row-major 2 x 2 weight, first minimum, `< 0.05` -> a map pair; otherwise the state branch (`< 0.6`); otherwise new.  The
    all-new shortcut for n == 3 (:379-387) applies only when there is no map.
  * Rows (:246-305): the state pairs' rows first, then the map pairs'.  A map pair's landmark is the map point widened to double
    (:282) and its rows have the three pose entries only (:300).  Everything after the association runs in longdouble, dense H.
  * A pose fix stacks three rows under all of them (fleet_pose_witness.py, joint form).

`mutate` (MAP_MUTATIONS) plants one defect of the kind a slip in k_fleet_step_map would cause; tests/test_fleet_map_cpu.py shows
that each is caught by the association lists or by the GPU bound.
"""
from __future__ import annotations

import math

import numpy as np

from tests.witness.fleet_pose_witness import PoseWitnessEKF
from tests.witness.fleet_witness import LDKIT, available, chol_inverse  # noqa: F401

MAP_GATE, STATE_GATE = 0.05, 0.6
# map_rows_landmark_cols   a map pair's rows also get the c / s block, at the columns its map index would have as a state landmark
# state_gate_first         the state branch is tried before the map
# threshold_unweighted     the first minimum is the weighted one, but `< 0.05` is applied to the Euclidean distance of that point
# map_rows_first           rows [0, 2 n_map) are built as map rows while the pair list still has the state pairs first
# cov_column_major         S[1] and S[2] swapped.  delta S delta^T is the same number for S and S^T, so this one CANNOT be seen but
#                          through FP64 round-off (tests/test_fleet_map_cpu.py::test_transposed_weight_is_the_same_distance)
MAP_MUTATIONS = ("map_rows_landmark_cols", "state_gate_first", "threshold_unweighted", "map_rows_first")
UNOBSERVABLE_MUTATIONS = ("cov_column_major",)


def weighted_distances(map_xy, map_cov, gx, gy, column_major=False):
    """FP64 weighted distances of the float32 global point (gx, gy) to every map point, in the reference's order of operations."""
    ex = (map_xy[:, 0] - gx).astype(np.float32).astype(np.float64)         # :408, map - g in float32
    ey = (map_xy[:, 1] - gy).astype(np.float32).astype(np.float64)
    S = map_cov.reshape(-1, 4)
    s1, s2 = (S[:, 2], S[:, 1]) if column_major else (S[:, 1], S[:, 2])
    t0 = ex * S[:, 0] + ey * s2
    t1 = ex * s1 + ey * S[:, 3]
    with np.errstate(invalid="ignore"):
        return np.sqrt(t0 * ex + t1 * ey), np.sqrt(ex * ex + ey * ey)


class MapWitnessEKF(PoseWitnessEKF):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.map_xy = np.zeros((0, 2), np.float32)
        self.map_cov = np.zeros((0, 4))
        self.last_match = ([], [], [])

    def set_map(self, xy, cov):
        self.map_xy = np.asarray(xy, np.float32).reshape(-1, 2).copy()
        self.map_cov = np.asarray(cov, np.float64).reshape(-1, 4).copy()

    # -- ReflectorMatch (cc:397-453) ------------------------------------------------------------------------------------------
    def match3(self, obs, mutate=None):
        state, mapped, new = [], [], []
        L = (self.mu.shape[0] - 3) // 2
        M_ = self.map_xy.shape[0]
        for i in range(obs.shape[0]):
            in_state = None
            if L > 0:
                d = self.distances(obs[i])
                j = int(np.argmin(d))
                if d[j] < STATE_GATE:
                    in_state = j
            if mutate == "state_gate_first" and in_state is not None:
                state.append((i, in_state))
                continue
            if M_ > 0:
                gx, gy = self.to_global(obs[i])
                dw, de = weighted_distances(self.map_xy, self.map_cov, gx, gy, mutate == "cov_column_major")
                j = int(np.argmin(np.where(np.isnan(dw), np.inf, dw)))     # first minimum; a NaN never wins
                if (de[j] if mutate == "threshold_unweighted" else dw[j]) < MAP_GATE:
                    mapped.append((i, j))
                    continue
            if in_state is not None:
                state.append((i, in_state))
                continue
            new.append(i)
        return state, mapped, new

    # -- HandleObservationMessage (cc:229-368) ----------------------------------------------------------------------------------
    def _map_rows(self, obs, pairs, kinds, mutate):
        """H and dz of `pairs`; kinds[i] says whether row pair i takes its landmark from the map."""
        kit, LD = self.kit, self.kit.T
        N, m = self.mu.shape[0], 2 * len(pairs)
        th = float(self.mu[2])
        c, s = LD(math.cos(th)), LD(math.sin(th))
        H, dz = kit.zeros((m, N)), kit.zeros(m)
        for i, ((l, g), of_map) in enumerate(zip(pairs, kinds)):
            if of_map:
                g = g % self.map_xy.shape[0]                      # (only a planted defect can bring a state index here)
                lx, ly = LD(float(self.map_xy[g, 0])), LD(float(self.map_xy[g, 1]))     # :282
            else:
                g = g % max((N - 3) // 2, 1)
                lx, ly = self.mu[3 + 2 * g], self.mu[4 + 2 * g]
            dx, dy = lx - self.mu[0], ly - self.mu[1]
            dz[2 * i] = LD(float(obs[l, 0])) - (dx * c + dy * s)
            dz[2 * i + 1] = LD(float(obs[l, 1])) - (-dx * s + dy * c)
            H[2 * i, 0:3] = [-c, -s, -dx * s + dy * c]
            H[2 * i + 1, 0:3] = [s, -c, -dx * c - dy * s]
            block = not of_map or (mutate == "map_rows_landmark_cols" and 4 + 2 * g < N)
            if block and N > 3:
                H[2 * i, 3 + 2 * g], H[2 * i, 4 + 2 * g] = c, s
                H[2 * i + 1, 3 + 2 * g], H[2 * i + 1, 4 + 2 * g] = -s, c
        return H, dz

    def handle_observation(self, t, obs, gps_pose=None, mutate=None):
        obs = np.asarray(obs, np.float32).reshape(-1, 2)
        kit = self.kit
        self.predict(float(t) - self.time)
        self.time = float(t)
        self.last_match = ([], [], [])
        if obs.shape[0] == 0:
            return
        state, mapped, new = self.match3(obs, mutate)
        self.last_match = (state, mapped, new)
        pairs = state + mapped
        MM, N = len(pairs), self.mu.shape[0]
        if MM > 0:
            if mutate == "map_rows_first":
                kinds = [i < len(mapped) for i in range(MM)]
            else:
                kinds = [i >= len(state) for i in range(MM)]
            m = 2 * MM
            H, dz = self._map_rows(obs, pairs, kinds, mutate)
            Q = self.q * kit.eye(m)
            if gps_pose is not None:
                e, R = self._pose_rows(gps_pose, None)
                Hj, dzj, Qj = kit.zeros((m + 3, N)), kit.zeros(m + 3), kit.zeros((m + 3, m + 3))
                Hj[:m], dzj[:m], dzj[m:] = H, dz, e
                for k in range(3):
                    Hj[m + k, k] = kit.T(1)
                Qj[:m, :m] = Q
                Qj[m:, m:] = R
                H, dz, Q = Hj, dzj, Qj
            W = self.sigma @ H.T
            Kt = W @ chol_inverse(H @ W + Q, kit)
            self.mu = self.mu + Kt @ dz
            self.sigma = self.sigma - Kt @ W.T
            self.mu[2] = kit.wrap(self.mu[2])
        if new:
            self._append(obs, new)
