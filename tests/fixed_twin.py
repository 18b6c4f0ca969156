"""Independent (test-only) numpy twin of fixed parameter blocks, on top of tests/robust_twin.py (not a test file).

Model (include/psba_hip.h, psba_amd/csrc/camera_model.h): cameras and points marked fixed are held
constant.  The problem solved is the reduced one: the columns of J that belong to fixed blocks are deleted and the
fixed values enter the residual as constants.  Embedded in the full-size system that is
    A_ij = 0 for a fixed camera j, B_ij = 0 for a fixed point i (after the whitening and the loss weight),
so W_ij = 0 if either is fixed, g_a,j = 0, g_b,i = 0, and the diagonal blocks of fixed cameras and points are zero
here (mu I once damped; the library stores coeff I there instead).  e and the cost are untouched.
Two statements of the model are kept apart so that tests can hold one against the other: the embedded one
(FixedTwin.linearize and everything that follows from it, fixed_pieces with the oracle's own sums) and the reduced
one (reduced_step: the columns really deleted, a dense solve).
"""
import numpy as np

from lens_twin import oracle_pieces
from robust_twin import NONE, RobustTwin


def masks(prob, fc=None, fp=None):
    """boolean [nC], [nP] from None / index lists / flag arrays"""
    def one(m, n):
        if m is None:
            return np.zeros(n, dtype=bool)
        m = np.asarray(m)
        if m.dtype == bool or m.size == n:  # one flag per block
            return m.reshape(n) != 0
        out = np.zeros(n, dtype=bool)  # a (shorter) list of indices
        out[m.astype(np.int64)] = True
        return out
    return one(fc, int(prob["nC"])), one(fp, int(prob["nP"]))


class FixedTwin(RobustTwin):
    """RobustTwin(prob, kind, c, kc, cov) with fixed cameras fc and fixed points fp (flags or index lists)."""

    def __init__(self, prob, fc=None, fp=None, kind=NONE, c=1.0, kc=None, cov=None):
        super().__init__(prob, kind, c, kc, cov)
        self.fc, self.fp = masks(prob, fc, fp)

    def fixed_entries(self):
        """boolean [nA + nB]: the entries of the parameter vector that belong to fixed blocks"""
        return np.r_[np.repeat(self.fc, 6), np.repeat(self.fp, 3)]

    def linearize(self):
        """e untouched; A, B zeroed for fixed blocks: what the normal equations see"""
        e, A, B = RobustTwin.linearize(self)
        A = np.where(self.fc[self.j][:, None, None], 0.0, A)
        B = np.where(self.fp[self.i][:, None, None], 0.0, B)
        return e, A, B

    def solve_lm(self, iters=50, mu0=1e-3, tol=1e-12):
        """RobustTwin.solve_lm on the masked normal equations.  N + mu I has mu I on the fixed blocks and g = 0 there, so
        dp = 0 on them; mu0 is relative to the largest diagonal entry, which a fixed block (zero) never is."""
        cams, pts, F = RobustTwin.solve_lm(self, iters, mu0, tol)
        fx = self.fixed_entries()
        assert np.array_equal(np.r_[cams.reshape(-1), pts.reshape(-1)][fx],
                              np.r_[self.cams.reshape(-1), self.pts.reshape(-1)][fx])
        return cams, pts, F

    def reduced_jacobian(self):
        """dense J with the columns of fixed blocks deleted (from the unmasked blocks), and the kept column indices"""
        free = np.flatnonzero(~self.fixed_entries())
        _, A, B = RobustTwin.linearize(self)
        J = np.zeros((2 * self.nO, self.nA + self.nB))
        for a in range(self.nO):
            J[2 * a:2 * a + 2, 6 * self.j[a]:6 * self.j[a] + 6] = A[a]
            J[2 * a:2 * a + 2, self.nA + 3 * self.i[a]:self.nA + 3 * self.i[a] + 3] = B[a]
        return J[:, free], free

    def reduced_step(self, mu):
        """dp [nA + nB] of the reduced damped system (J_f^T J_f + mu I) dp_f = J_f^T e by a dense solve, zero elsewhere"""
        Jf, free = self.reduced_jacobian()
        e, _, _ = RobustTwin.linearize(self)
        dp = np.zeros(self.nA + self.nB)
        dp[free] = np.linalg.solve(Jf.T @ Jf + mu * np.eye(free.size), Jf.T @ e.reshape(-1))
        return dp


def fixed_pieces(prob, fc=None, fp=None, kind=NONE, c=1.0, kc=None, cov=None, mu=None):
    """the oracle's U, V, W, g (and with mu: S, e_a, dp) of the masked e, A, B -- the oracle's own sums, unchanged
    (lens_twin.oracle_pieces).  Fixed diagonal blocks are zero (mu I with mu)."""
    t = FixedTwin(prob, fc, fp, kind, c, kc, cov)
    e, A, B = t.linearize()
    return t, (e, A, B), oracle_pieces(prob, e, A, B, mu=mu)


# ---- helpers of tests/test_gpu_fixed.py (kept here so that the test module imports no other test module) ----------
# the K1 / K2 / K3 routes of tests/test_gpu_robust.py's damping-try test, plus K2's global-atomic and runs layouts
ROUTES = {"default": {}, "owner": {"PSBA_SCHUR_OWNER": "1"}, "cam_major": {}, "long": {}, "pcg": {},
          "v1": {"PSBA_LIN_V1": "1"}, "read_w": {"PSBA_BACK_READ_W": "1"},
          "atomic": {"PSBA_SCHUR_ATOMIC": "1"}, "runs": {"PSBA_SCHUR_RUNS": "1"}}


def close(got, want, tol, what=""):
    """max |got - want| <= tol max |want|"""
    got, want = np.asarray(got), np.asarray(want)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= tol * scale, f"{what}: max|diff|={err:.3e} scale={scale:.3e} rel={err / scale:.3e}"


def random_spd(rng, n):
    """n random SPD 2 x 2 covariances"""
    G = rng.normal(size=(n, 2, 2))
    return G @ np.transpose(G, (0, 2, 1)) + 0.5 * np.eye(2)[None]


def random_kc(rng, nC, k1=0.4):
    """kc = (k1..k5) per camera around a moderate barrel distortion"""
    return np.column_stack([k1 * (1 + 0.1 * rng.normal(size=nC)), -0.3 * (1 + 0.1 * rng.normal(size=nC)),
                            2e-3 * rng.normal(size=nC), 2e-3 * rng.normal(size=nC), 0.2 * rng.normal(size=nC)])
