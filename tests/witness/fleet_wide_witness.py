"""tests/witness/fleet_wide_witness.py -- TEST INFRASTRUCTURE: HandleObservationMessage in BLOCK form, dense and literal in
numpy.longdouble: what k_fleet_step_wide (csrc/fleet_wide.hip) computes for a scan of more than 32 matched pairs, beside the joint
form of tests/witness/fleet_map_witness.py (the reference's, the one the GPU is held to).

Predict, ReflectorMatch (map branch first), the rows, the pose rows, the Cholesky inverse and the append come from the witnesses this
one extends.  What is restated here is the ORDER of the update.  With mu0, P0 the state behind Predict, H and h(mu0) of all MM pairs
evaluated at mu0 (cos / sin of mu0's FP64 heading), state pairs first, then map pairs:

    block b = pairs [32 b, min(32 b + 32, MM)):
        dz_b = z_b - h_b(mu0) - H_b (mu_b - mu0),  W_b = P_b H_b^T,  S_b = H_b W_b + q I,  K_b = W_b S_b^-1,
        mu_b+1 = mu_b + K_b dz_b,  P_b+1 = P_b - K_b W_b^T

    a pose fix (three rows [I3 0], noise R, innovation wrap(z - mu0[0:3]) - (mu[0:3] - mu0[0:3])) is a step of its own: behind the
    last block for a plain member, in front of the first for a member on the map; the heading is normalised ONCE, behind everything.

The noise is block-diagonal between any two groups of rows, so this equals the joint update: tests/test_fleet_wide_cpu.py holds the
two forms to each other on every case.  Measured there (BLOCK_VS_JOINT_*): the larger of the two errors over all cases is longdouble
round-off times the conditioning of the joint solve, far below the FP64 floor.

`mutate` (WIDE_MUTATIONS) plants one defect of the kind a slip in the block loop would cause:
    no_correction        H_b (mu_b - mu0) left out: every block's innovation is the one at mu0
    relinearise          block b's rows and innovation evaluated at mu_b (an iterated update, not the reference's joint one)
    drop_last_partial    the last block is skipped when it holds fewer than 32 pairs
    local_row_width      whether a row is a map row goes by the pair's index INSIDE the block against NS
    wrap_every_block     the heading is normalised behind every block (the correction then sees a jump of 2 pi)
    pose_in_loop         phase P pasted inside the block loop: the pose rows are applied behind every block, not once
"""
from __future__ import annotations

import numpy as np

from tests.witness.fleet_map_witness import MapWitnessEKF
from tests.witness.fleet_witness import Kit, available, chol_inverse  # noqa: F401

BLOCK_PAIRS = 32
WIDE_MUTATIONS = ("no_correction", "relinearise", "drop_last_partial", "local_row_width", "wrap_every_block", "pose_in_loop")
# block form against joint form, both in longdouble, worst over tests/fleet_wide_cases.all_cases() (rel_err's two figures):
# measured 4.1e-15 (sigma, wideaug_L60_MM33_N33_diff) and 3.1e-18 (mu, wide_tall_L2_MM40): longdouble's 5.4e-20 times the
# conditioning of the joint solve; recorded = what the CPU test asserts, the measured figures rounded up to the next decade
BLOCK_VS_JOINT_SIGMA = 1e-14
BLOCK_VS_JOINT_MU = 1e-17


class F64Kit(Kit):
    """The witness's arithmetic in plain FP64: the block ORDER's own round-off, for the measured floor."""

    def __init__(self):
        self.mp = None
        self.dtype = np.float64
        self.T = np.float64

    def arr(self, x):
        return np.asarray(x).astype(np.float64)


class BlockWitnessEKF(MapWitnessEKF):
    def _rows_at(self, mu_at, obs, pairs, kinds):
        keep = self.mu
        self.mu = mu_at
        try:
            return self._map_rows(obs, pairs, kinds, None)
        finally:
            self.mu = keep

    def handle_observation(self, t, obs, gps_pose=None, mutate=None):
        obs = np.asarray(obs, np.float32).reshape(-1, 2)
        kit = self.kit
        self.predict(float(t) - self.time)
        self.time = float(t)
        self.last_match = ([], [], [])
        if obs.shape[0] == 0:
            return
        state, mapped, new = self.match3(obs, None)
        self.last_match = (state, mapped, new)
        pairs = state + mapped
        NS, MM = len(state), len(pairs)
        if MM > 0:
            mu0 = self.mu.copy()
            kinds = [i >= NS for i in range(MM)]
            H0, h0 = self._rows_at(mu0, obs, pairs, kinds)                 # h0 = z - h(mu0)
            on_map = self.map_xy.shape[0] > 0
            if gps_pose is not None:
                e, R = self._pose_rows(gps_pose, None)                     # at mu0

            def pose_step():
                innov2 = e - (self.mu[0:3] - mu0[0:3])
                W2 = self.sigma[:, 0:3].copy()
                K2 = W2 @ chol_inverse(self.sigma[0:3, 0:3] + R, kit)
                self.mu = self.mu + K2 @ innov2
                self.sigma = self.sigma - K2 @ W2.T

            if gps_pose is not None and on_map:
                pose_step()
            nb = (MM + BLOCK_PAIRS - 1) // BLOCK_PAIRS
            for b in range(nb):
                lo, hi = BLOCK_PAIRS * b, min(BLOCK_PAIRS * b + BLOCK_PAIRS, MM)
                if mutate == "drop_last_partial" and b > 0 and hi - lo < BLOCK_PAIRS:
                    continue
                if mutate == "relinearise":
                    Hb, dz = self._rows_at(self.mu, obs, pairs[lo:hi], kinds[lo:hi])
                else:
                    if mutate == "local_row_width":
                        Hb, dz = self._rows_at(mu0, obs, pairs[lo:hi], [i >= NS for i in range(hi - lo)])
                    else:
                        Hb, dz = H0[2 * lo: 2 * hi], h0[2 * lo: 2 * hi].copy()
                    if mutate != "no_correction":
                        dz = dz - Hb @ (self.mu - mu0)
                m = Hb.shape[0]
                W = self.sigma @ Hb.T
                Kt = W @ chol_inverse(Hb @ W + self.q * kit.eye(m), kit)
                self.mu = self.mu + Kt @ dz
                self.sigma = self.sigma - Kt @ W.T
                if mutate == "wrap_every_block":
                    self.mu[2] = kit.wrap(self.mu[2])
                if mutate == "pose_in_loop" and gps_pose is not None and not on_map and b < nb - 1:
                    pose_step()
            if gps_pose is not None and not on_map:
                pose_step()
            self.mu[2] = kit.wrap(self.mu[2])
        if new:
            self._append(obs, new)
