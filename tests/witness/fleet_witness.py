"""tests/witness/fleet_witness.py -- TEST INFRASTRUCTURE: the EKF-SLAM core once more, dense and literal, in numpy.longdouble
(64-bit mantissa on x86-64), as the high-precision reference of the fleet kernel's edge-case tests.

One HandleOdometryMessage / HandleObservationMessage of the reference (src/reflector_ekf_slam/reflector_ekf_slam.cc:154-223,
:229-368, :370-455) with the formulas of oracle/ekf_numpy.py: dense G, dense H, K = P H^T (H P H^T + Q)^-1, P = P - K H P.
What differs:
  * every product and sum of the filter runs in longdouble;
  * the association is the SPECIFICATION and is kept as it is: float32 differences, FP64 distance, first minimum, `< 0.6`;
  * S^-1 comes from a hand-written Cholesky (numpy.linalg has no longdouble);
  * what the reference rounds stays rounded: sin / cos are taken of the FP64 heading and are FP64 values, the global points of
    new landmarks are float32, dt is the FP64 difference of two FP64 times.
Written independently of oracle/ekf_oracle.c; shares nothing with the kernel.

`mutate` (see MUTATIONS) plants one defect of the kind an indexing slip in k_fleet_step would cause; tests/test_fleet_edges_cpu.py
uses it to show that the GPU bound can fail.  SINGLE_MUTATIONS are the slips of the single filter's launch forms (k_mid gathers
from a covariance stored one scan behind and corrects what it gathers, the downdate works in 64-row tiles with border strips,
wide scans run as block steps); tests/test_ekf_shapes_cpu.py uses those.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
DIFF, OMNI = 0, 1
MUTATIONS = ("drop_last4", "skip_tile", "w_row_shift", "k_pad_col")
# (stale_*: `where` = (i, j), the element that misses the previous scan's rank-m correction; skip_tile64: `where` = (I, J), 64-row
# tiles; border_strip: the last row and column of the state; block_step_drop: the pairs behind the first 32 are not applied)
SINGLE_MUTATIONS = ("stale_gather", "stale_own_row", "skip_tile64", "border_strip", "w_row_shift", "k_pad_col", "block_step_drop")
STEP_PAIRS = 32                                                 # pairs per block step of a wide scan without a pose fix


def available() -> bool:
    return np.finfo(LD).nmant >= 63


class Kit:
    """The scalar type the witness computes in: numpy.longdouble, or mpmath's mpf at 40 digits (object arrays), which pins it."""

    def __init__(self, mp=None):
        self.mp = mp
        self.dtype = object if mp else LD
        self.T = mp.mpf if mp else LD

    def arr(self, x):
        a = np.asarray(x)
        if not self.mp:
            return a.astype(LD)
        if a.dtype == object:
            return a.copy()
        out = np.empty(a.shape, object)
        out.ravel()[:] = [self.mp.mpf(float(v)) for v in a.ravel()]
        return out

    def zeros(self, shape):
        return np.full(shape, self.T(0), dtype=self.dtype)

    def eye(self, n):
        E = self.zeros((n, n))
        for i in range(n):
            E[i, i] = self.T(1)
        return E

    def sqrt(self, v):
        return self.mp.sqrt(v) if self.mp else np.sqrt(v)

    def wrap(self, v):
        if self.mp:
            return self.mp.atan2(self.mp.sin(v), self.mp.cos(v))
        return np.arctan2(np.sin(v), np.cos(v))


LDKIT = Kit()


def chol_inverse(S, kit=LDKIT):
    """S^-1 of an SPD longdouble matrix: S = L L^T, Y = L^-1 by forward substitution, S^-1 = Y^T Y.  Raises on a pivot <= 0."""
    m = S.shape[0]
    Lm = kit.zeros((m, m))
    for j in range(m):
        d = S[j, j] - np.dot(Lm[j, :j], Lm[j, :j])
        if not d > 0:
            raise ArithmeticError(f"pivot {j} of the innovation covariance is not positive ({float(d):.3e})")
        Lm[j, j] = kit.sqrt(d)
        if j + 1 < m:
            Lm[j + 1:, j] = (S[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    Y = kit.zeros((m, m))
    for i in range(m):
        row = -(Lm[i, :i] @ Y[:i, :]) if i else kit.zeros(m)
        row[i] += kit.T(1)
        Y[i, :] = row / Lm[i, i]
    return Y.T @ Y


class WitnessEKF:
    def __init__(self, odom_model, init_time, init_pose, lin_cov, ang_cov, obs_cov, kit=LDKIT):
        self.kit = kit
        self.model = DIFF if odom_model == DIFF else OMNI
        self.time = float(init_time)
        self.mu = kit.arr(np.asarray(init_pose, np.float64))
        self.sigma = kit.zeros((3, 3))
        self.vt = np.zeros(3)
        qs = [lin_cov, ang_cov] if self.model == DIFF else [lin_cov, lin_cov, ang_cov]
        self.Qu = kit.zeros((len(qs), len(qs)))
        for i, v in enumerate(qs):
            self.Qu[i, i] = kit.T(float(v))
        self.q = kit.T(float(obs_cov))
        self.last_match = ([], [])
        self.last_S = None
        self.sigma_stale = None                                 # the covariance the last update started from (the stale_* defects)

    def set_state(self, t, mu, sigma, vt=(0.0, 0.0, 0.0)):
        self.time = float(t)
        self.mu = self.kit.arr(np.asarray(mu, np.float64))
        self.sigma = self.kit.arr(np.asarray(sigma, np.float64))
        self.vt = np.asarray(vt, np.float64).copy()

    # -- Predict (cc:154-206) ---------------------------------------------------------------------------------------------
    def predict(self, dt):
        dt = float(dt)
        kit, LD = self.kit, self.kit.T
        N = self.mu.shape[0]
        vx, vy, w = (float(v) for v in self.vt)
        th = float(self.mu[2])                                  # the FP64 heading
        G = kit.eye(3)
        T = LD(dt)
        if self.model == DIFF:
            half = th + w * dt / 2                              # FP64, as the reference forms the angle
            c, s = LD(math.cos(half)), LD(math.sin(half))
            dx, dy = LD(vx) * T * c, LD(vx) * T * s
            G[0, 2], G[1, 2] = -LD(vx) * T * s, LD(vx) * T * c
            Gu = kit.zeros((3, 2))
            Gu[0, 0], Gu[0, 1] = T * c, -LD(vx) * T * T * s / 2
            Gu[1, 0], Gu[1, 1] = T * s, LD(vx) * T * T * c / 2
            Gu[2, 1] = T
        else:
            c, s = LD(math.cos(th)), LD(math.sin(th))
            dx = LD(vx) * T * c - LD(vy) * T * s
            dy = LD(vx) * T * s + LD(vy) * T * c
            G[0, 2] = -LD(vx) * T * s - LD(vy) * T * c
            G[1, 2] = LD(vx) * T * c - LD(vy) * T * s
            Gu = kit.zeros((3, 3))
            Gu[0, 0], Gu[0, 1] = T * c, -T * s
            Gu[1, 0], Gu[1, 1] = T * s, T * c
            Gu[2, 2] = T
        # G differs from the identity in two entries: G P G^T without the N^3 products
        P = self.sigma.copy()
        P[0, :] += G[0, 2] * self.sigma[2, :]
        P[1, :] += G[1, 2] * self.sigma[2, :]
        P2 = P.copy()
        P2[:, 0] += G[0, 2] * P[:, 2]
        P2[:, 1] += G[1, 2] * P[:, 2]
        P2[:3, :3] += Gu[:3] @ self.Qu @ Gu[:3].T
        self.sigma = P2
        self.mu = self.mu.copy()
        self.mu[0] += dx
        self.mu[1] += dy
        self.mu[2] += LD(w) * T
        self.mu[2] = self.kit.wrap(self.mu[2])

    def handle_odometry(self, t, vx, vy, wz):
        if t < self.time:
            return
        self.vt = np.array([vx, vy, wz], np.float64)
        self.predict(float(t) - self.time)
        self.time = float(t)

    # -- ReflectorMatch, state branch (cc:370-455): the specification, kept in its own number formats -----------------------
    def to_global(self, p):
        x0, y0, th = float(self.mu[0]), float(self.mu[1]), float(self.mu[2])
        c, s = math.cos(th), math.sin(th)
        return (np.float32(float(p[0]) * c - float(p[1]) * s + x0), np.float32(float(p[0]) * s + float(p[1]) * c + y0))

    def distances(self, p):
        """FP64 distances of observation p (sensor frame) to every landmark of the state, as ReflectorMatch forms them."""
        gx, gy = self.to_global(p)
        lm = np.array([float(v) for v in self.mu[3:]], np.float64).astype(np.float32).reshape(-1, 2)
        ex = (gx - lm[:, 0]).astype(np.float32).astype(np.float64)
        ey = (gy - lm[:, 1]).astype(np.float32).astype(np.float64)
        return np.sqrt(ex * ex + ey * ey)

    def match(self, obs):
        pairs, new = [], []
        M = (self.mu.shape[0] - 3) // 2
        for i in range(obs.shape[0]):
            if M > 0:
                d = self.distances(obs[i])
                j = int(np.argmin(d))                           # first minimum
                if d[j] < 0.6:
                    pairs.append((i, j))
                    continue
            new.append(i)
        return pairs, new

    # -- HandleObservationMessage (cc:229-368) ----------------------------------------------------------------------------
    def handle_observation(self, t, obs, mutate=None, where=None):
        obs = np.asarray(obs, np.float32).reshape(-1, 2)
        kit = self.kit
        self.predict(float(t) - self.time)
        self.time = float(t)
        self.last_match = ([], [])
        if obs.shape[0] == 0:
            return
        pairs, new = self.match(obs)
        self.last_match = (pairs, new)
        if pairs:
            upd = pairs[:STEP_PAIRS] if mutate == "block_step_drop" else pairs
            H, dz = self._reflector_rows(obs, upd)
            m = H.shape[0]
            W = self.sigma @ H.T
            if mutate == "w_row_shift":
                i, j = where
                W[i, j] = (self.sigma @ H.T)[i + 1, j]
            if mutate == "stale_own_row":                       # one element of P(own rows, R) without the pending correction
                i, j = where
                Pw = self.sigma.copy()
                Pw[i, j] = self.sigma_stale[i, j]
                W = Pw @ H.T
            S = H @ W + self.q * kit.eye(m)
            if mutate == "stale_gather":                        # one element (and its mirror) of the gathered P(R, R)
                i, j = where
                Pg = self.sigma.copy()
                Pg[i, j] = Pg[j, i] = self.sigma_stale[i, j]
                S = H @ (Pg @ H.T) + self.q * kit.eye(m)
            self.last_S = S
            self.sigma_stale = self.sigma
            Kt = W @ chol_inverse(S, kit)
            self.mu = self.mu + Kt @ dz
            self.mu[2] = self.kit.wrap(self.mu[2])
            self.sigma = self.sigma - self._downdate(Kt, W, m, mutate, where)
        if new:
            self._append(obs, new)

    def _reflector_rows(self, obs, pairs):
        """H and the innovation dz of the matched observations at the current mean (cc:246-305)."""
        kit, LD = self.kit, self.kit.T
        N, m = self.mu.shape[0], 2 * len(pairs)
        th = float(self.mu[2])
        c, s = LD(math.cos(th)), LD(math.sin(th))
        H, dz = kit.zeros((m, N)), kit.zeros(m)
        for i, (l, g) in enumerate(pairs):
            dx, dy = self.mu[3 + 2 * g] - self.mu[0], self.mu[4 + 2 * g] - self.mu[1]
            dz[2 * i] = LD(float(obs[l, 0])) - (dx * c + dy * s)
            dz[2 * i + 1] = LD(float(obs[l, 1])) - (-dx * s + dy * c)
            H[2 * i, 0:3] = [-c, -s, -dx * s + dy * c]
            H[2 * i + 1, 0:3] = [s, -c, -dx * c - dy * s]
            H[2 * i, 3 + 2 * g], H[2 * i, 4 + 2 * g] = c, s
            H[2 * i + 1, 3 + 2 * g], H[2 * i + 1, 4 + 2 * g] = -s, c
        return H, dz

    def _append(self, obs, new):
        """The new observations become reflectors of the state (cc:311-364)."""
        kit, LD = self.kit, self.kit.T
        N, N2 = self.mu.shape[0], len(new)
        Me = N + 2 * N2
        xe = kit.zeros(Me)
        xe[:N] = self.mu
        Sg = kit.zeros((Me, Me))
        Sg[:N, :N] = self.sigma
        th = float(self.mu[2])
        c, s = LD(math.cos(th)), LD(math.sin(th))
        Gz = kit.zeros((2, 2))
        Gz[0, 0], Gz[0, 1], Gz[1, 0], Gz[1, 1] = c, -s, s, c
        Gp = kit.zeros((2 * N2, 3))
        for i, l in enumerate(new):
            gx, gy = self.to_global(obs[l])
            xe[N + 2 * i], xe[N + 2 * i + 1] = LD(float(gx)), LD(float(gy))
            rx, ry = LD(float(obs[l, 0])), LD(float(obs[l, 1]))
            Gp[2 * i] = [LD(1), LD(0), -rx * s - ry * c]
            Gp[2 * i + 1] = [LD(0), LD(1), rx * c - ry * s]
        Smx = Gp @ self.sigma[0:3, :]
        RQR = Gz @ (self.q * kit.eye(2)) @ Gz.T
        Smm = Gp @ self.sigma[0:3, 0:3] @ Gp.T
        for i in range(N2):
            for j in range(N2):
                Smm[2 * i: 2 * i + 2, 2 * j: 2 * j + 2] += RQR          # Gz Qt Gz^T with the stacked Gz (cc:349-354)
        Sg[N:, :N] = Smx
        Sg[:N, N:] = Smx.T
        Sg[N:, N:] = Smm
        self.mu, self.sigma = xe, Sg

    @staticmethod
    def _downdate(Kt, W, m, mutate, where):
        """K H P = K W^T, or one of the planted defects."""
        if mutate == "drop_last4":                              # phase F without its 4-wide tail
            keep = ((m + 3) & ~3) - 4
            return Kt[:, :keep] @ W[:, :keep].T
        if mutate == "k_pad_col":
            # Column m of K and W is padding when m % 4 == 2.  A non-zero K[:, m] alone is invisible (it meets the zero column
            # of W, and the mean update stops at m), so the defect planted is the pair a staged-W rewrite could leave: both
            # padding columns hold stale values (here: the previous column's).
            assert m % 4 == 2
            return Kt @ W.T + np.outer(Kt[:, m - 1], W[:, m - 1])
        D = Kt @ W.T
        if mutate in ("skip_tile", "skip_tile64"):
            I, J = where
            T = 16 if mutate == "skip_tile" else 64
            D[T * I: T * I + T, T * J: T * J + T] = 0
            D[T * J: T * J + T, T * I: T * I + T] = 0           # the kernel holds the lower triangle only: the mirror goes with it
        if mutate == "border_strip":
            D[-1, :] = 0
            D[:, -1] = 0
        return D

    def state(self):
        return self.mu.copy(), self.sigma.copy()
