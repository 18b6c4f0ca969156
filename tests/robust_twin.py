"""Independent (test-only) numpy twin of the robust losses, on top of tests/lens_twin.py (not a test file).

Model (include/psba_hip.h, psba_amd/csrc/camera_model.h):
    s_a = ||L_a e_a||^2 (the whitened squared residual), F = sum_a rho(s_a), c > 0 in whitened units, c2 = c^2
    NONE     rho = s                                 rho' = 1
    HUBER    rho = s (s <= c2), 2 c sqrt(s) - c2     rho' = 1, c / sqrt(s)
    CAUCHY   rho = c2 log(1 + s / c2)                rho' = 1 / (1 + s / c2)
    SOFT_L1  rho = 2 c2 (sqrt(1 + s / c2) - 1)       rho' = 1 / sqrt(1 + s / c2)
    IRLS: w = sqrt(rho'(s)), e <- w e, A <- w A, B <- w B (no rho'' term).
Written from the formulas above, not from the kernels; checked against central differences of its own rho and F.
"""
import numpy as np

from lens_twin import Twin, oracle_pieces

NONE, HUBER, CAUCHY, SOFT_L1 = 0, 1, 2, 3
KINDS = {"huber": HUBER, "cauchy": CAUCHY, "soft_l1": SOFT_L1}


def rho(kind, c, s):
    s = np.asarray(s, dtype=np.float64)
    c2 = c * c
    if kind == HUBER:
        return np.where(s <= c2, s, 2.0 * c * np.sqrt(s) - c2)
    if kind == CAUCHY:
        return c2 * np.log1p(s / c2)
    if kind == SOFT_L1:
        return 2.0 * s / (np.sqrt(1.0 + s / c2) + 1.0)  # = 2 c2 (sqrt(1 + s / c2) - 1) without the cancellation
    return s.copy()


def drho(kind, c, s):
    """rho'(s)"""
    s = np.asarray(s, dtype=np.float64)
    c2 = c * c
    if kind == HUBER:
        return np.where(s <= c2, 1.0, c / np.sqrt(np.maximum(s, c2)))
    if kind == CAUCHY:
        return 1.0 / (1.0 + s / c2)
    if kind == SOFT_L1:
        return 1.0 / np.sqrt(1.0 + s / c2)
    return np.ones_like(s)


class RobustTwin(Twin):
    """Twin(prob, kc, cov) plus a robust loss (kind, c)."""

    def __init__(self, prob, kind=NONE, c=1.0, kc=None, cov=None):
        super().__init__(prob, kc, cov)
        self.kind, self.c = kind, float(c)

    def sq_residuals(self, cams=None, pts=None):
        """s [nO] = ||L e||^2"""
        e = Twin.residual(self, cams, pts)
        return (e * e).sum(1)

    def cost(self, cams=None, pts=None):
        return float(rho(self.kind, self.c, self.sq_residuals(cams, pts)).sum())

    def weights(self):
        """w [nO] = sqrt(rho'(s)) at the current parameters"""
        return np.sqrt(drho(self.kind, self.c, self.sq_residuals()))

    def linearize(self):
        """w L e [nO, 2], w L A [nO, 2, 6], w L B [nO, 2, 3]: what the normal equations see"""
        e, A, B = Twin.linearize(self)
        w = np.sqrt(drho(self.kind, self.c, (e * e).sum(1)))
        return w[:, None] * e, w[:, None, None] * A, w[:, None, None] * B

    def gradient(self):
        """g = J~^T e~ (the library's sign: -1/2 dF/dp, since A, B are derivatives of the projection)"""
        e, _, _ = self.linearize()
        return self.jacobian().T @ e.reshape(-1)

    def solve_lm(self, iters=50, mu0=1e-3, tol=1e-12):
        """a plain dense LM on F (the twin's IRLS normal equations, Nielsen's damping update): reference solutions
        for the recovery and solver tests.  Returns (cams, pts, F)."""
        nA = self.nA
        p = np.r_[self.cams.reshape(-1), self.pts.reshape(-1)]
        base = (self.cams.copy(), self.pts.copy())
        F = self.cost()
        N, g = self.normal()
        mu, nu = mu0 * np.diag(N).max(), 2.0
        for _ in range(iters):
            dp = np.linalg.solve(N + mu * np.eye(N.shape[0]), g)
            q = p + dp
            Fn = self.cost(q[:nA], q[nA:])
            pred = dp @ (mu * dp + g)
            rho_ = (F - Fn) / pred if pred > 0 else -1.0
            if rho_ > 0:
                p, F = q, Fn
                self.cams, self.pts = q[:nA].reshape(self.nC, 6).copy(), q[nA:].reshape(self.nP, 3).copy()
                N, g = self.normal()
                mu *= max(1.0 / 3.0, 1.0 - (2.0 * rho_ - 1.0) ** 3)
                nu = 2.0
                if np.abs(dp).max() < tol * (np.abs(p).max() + tol):
                    break
            else:
                mu *= nu
                nu *= 2.0
                if mu > 1e30 * np.diag(N).max():  # no step lowers F: converged to rounding
                    break
        out = (self.cams.copy(), self.pts.copy(), F)
        self.cams, self.pts = base
        return out


def robust_pieces(prob, kind, c, kc=None, cov=None, mu=None):
    """the oracle's U, V, W, g (and with mu: S, e_a, dp) of the weighted e, A, B -- the same sums in the same order
    as the reference's kernels (lens_twin.oracle_pieces)"""
    t = RobustTwin(prob, kind, c, kc, cov)
    e, A, B = t.linearize()
    return t, (e, A, B), oracle_pieces(prob, e, A, B, mu=mu)
