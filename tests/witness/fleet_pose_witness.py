"""tests/witness/fleet_pose_witness.py -- TEST INFRASTRUCTURE: HandleObservationMessage WITH the pose rows of the USE_GPS branch
(reference reflector_ekf_slam_gps.cc:305-340), dense and literal in numpy.longdouble, as tests/witness/fleet_witness.py restates
the plain update.  Predict, the association, the Cholesky inverse and the number type come from there.

Two forms of the same update:
  joint     the reference's: three rows H = [I3 0] with noise diag(0.05^2, 0.05^2, 0.017^2) stacked under the reflector rows, the
            yaw innovation through the quaternion -> angle-axis wrap (gps.cc:320-328), one solve of up to 67 rows;
  two_step  what k_fleet_step computes: the reflector update alone (mu0 -> mu1, P1), then the pose rows at the SAME linearisation
            point, innovation wrap(z - mu0[0:3]) - (mu1[0:3] - mu0[0:3]), S2 = P1[0:3, 0:3] + R, K2 = P1[:, 0:3] S2^-1.
The noise is block-diagonal between the two groups of rows, so the forms are equal; tests/test_fleet_pose_cpu.py checks it to
longdouble round-off.  The heading is normalised once, after the whole update.  With no matched reflector the fix is ignored
(the rows exist only inside the reference's `if (MM > 0)`).

`mutate` (POSE_MUTATIONS) plants one defect of the kind a slip in the kernel's pose phase would cause.
"""
from __future__ import annotations

import numpy as np

from tests.witness.fleet_witness import LDKIT, WitnessEKF, available, chol_inverse  # noqa: F401

POSE_MUTATIONS = ("unwrapped_yaw", "no_pose_noise", "fix_when_unmatched")
POSE_NOISE = (0.05 * 0.05, 0.05 * 0.05, 0.017 * 0.017)          # gps.cc:312-316


def yaw_innovation(d, kit=LDKIT):
    """gps.cc:320-328: the yaw difference as the quaternion (w, 0, 0, z), normalised, w >= 0, to the angle-axis z component."""
    if kit.mp:
        mp = kit.mp
        w, z = mp.cos(d / 2), mp.sin(d / 2)
        nrm = mp.sqrt(w * w + z * z)
        w, z = w / nrm, z / nrm
        if w < 0:
            w, z = -w, -z
        ang = 2 * mp.atan2(abs(z), w)
        return (mp.mpf(2) if ang < 1e-7 else ang / mp.sin(ang / 2)) * z
    T = kit.T
    w, z = np.cos(d / T(2)), np.sin(d / T(2))
    nrm = np.sqrt(w * w + z * z)
    w, z = w / nrm, z / nrm
    if w < 0:
        w, z = -w, -z
    ang = T(2) * np.arctan2(abs(z), w)
    return (T(2) if ang < 1e-7 else ang / np.sin(ang / T(2))) * z


class PoseWitnessEKF(WitnessEKF):
    def __init__(self, *a, form="joint", **kw):
        super().__init__(*a, **kw)
        assert form in ("joint", "two_step")
        self.form = form

    def _pose_rows(self, fix, mutate):
        kit, LD = self.kit, self.kit.T
        e = kit.zeros(3)
        for k in range(3):
            e[k] = LD(float(fix[k])) - self.mu[k]
        if mutate != "unwrapped_yaw":
            e[2] = yaw_innovation(e[2], kit)
        R = kit.zeros((3, 3))
        if mutate != "no_pose_noise":
            for k in range(3):
                R[k, k] = LD(POSE_NOISE[k])
        return e, R

    def handle_observation(self, t, obs, gps_pose=None, mutate=None):
        obs = np.asarray(obs, np.float32).reshape(-1, 2)
        kit = self.kit
        self.predict(float(t) - self.time)
        self.time = float(t)
        self.last_match = ([], [])
        if obs.shape[0] == 0:
            return
        pairs, new = self.match(obs)
        self.last_match = (pairs, new)
        MM, N = len(pairs), self.mu.shape[0]
        use_fix = gps_pose is not None and (MM > 0 or mutate == "fix_when_unmatched")
        if MM > 0 or use_fix:
            m = 2 * MM
            H, dz = self._reflector_rows(obs, pairs)
            if not use_fix:
                W = self.sigma @ H.T
                Kt = W @ chol_inverse(H @ W + self.q * kit.eye(m), kit)
                self.mu = self.mu + Kt @ dz
                self.sigma = self.sigma - Kt @ W.T
            elif self.form == "joint" or MM == 0:
                e, R = self._pose_rows(gps_pose, mutate)
                Hj, dzj, Q = kit.zeros((m + 3, N)), kit.zeros(m + 3), kit.zeros((m + 3, m + 3))
                Hj[:m], dzj[:m], dzj[m:] = H, dz, e
                for k in range(3):
                    Hj[m + k, k] = kit.T(1)
                Q[:m, :m] = self.q * kit.eye(m)
                Q[m:, m:] = R
                W = self.sigma @ Hj.T
                Kt = W @ chol_inverse(Hj @ W + Q, kit)
                self.mu = self.mu + Kt @ dzj
                self.sigma = self.sigma - Kt @ W.T
            else:
                e, R = self._pose_rows(gps_pose, mutate)                   # at mu0, the linearisation point of both steps
                mu0 = self.mu.copy()
                W = self.sigma @ H.T
                Kt = W @ chol_inverse(H @ W + self.q * kit.eye(m), kit)
                mu1 = self.mu + Kt @ dz
                P1 = self.sigma - Kt @ W.T
                innov2 = e - (mu1[0:3] - mu0[0:3])
                W2 = P1[:, 0:3]
                K2 = W2 @ chol_inverse(P1[0:3, 0:3] + R, kit)
                self.mu = mu1 + K2 @ innov2
                self.sigma = P1 - K2 @ W2.T
            self.mu[2] = kit.wrap(self.mu[2])
        if new:
            self._append(obs, new)
