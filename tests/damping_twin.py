"""Numpy twin of the damping rules of the free-intrinsics route (psba_set_damping; test-only, no GPU):
TwinKD (tests/freekd_twin.py) with N + mu D in the place of N + mu I.

    D_k = min(max(N_kk, dmin), dmax)            Marquardt's scaling with the clamps of production solvers
    N_kk                                        the diagonal of J^T J, the placeholder 1 at a held coordinate
    point system V + mu diag(D_b), camera diagonal U_kk + mu D_k, gain_den = dp . (mu D dp + g)
    levmar: mu_0 = tau (not tau max diag), everything else lm_loop.cpp as TwinKD.levmar restates it

The loop is TwinKD.levmar itself: TwinDamp overrides only its starting mu and the D of a linearization, so the two rules
differ in the twin by exactly what they differ by in the library (the test pins the logs of the identity rule equal).
"""
import numpy as np

from freekd_twin import CNP, TwinKD

DMIN, DMAX = 1e-6, 1e32     # the defaults of psba_set_damping
IDENTITY, MARQUARDT = 0, 1


def damp_diag(N, dmin=DMIN, dmax=DMAX):
    """D [n] from N [n, n] or from its diagonal [n]"""
    d = np.diag(N) if np.ndim(N) == 2 else np.asarray(N, dtype=np.float64)
    return np.minimum(np.maximum(d, dmin), dmax)


class TwinDamp(TwinKD):
    damp_diag = staticmethod(damp_diag)

    def diag_normal(self):
        """diag(N) [nT] without the dense J (a problem of 66 000 observations has no dense twin): column sums of
        squares of A and B per camera and per point, the placeholder 1 at held coordinates"""
        _, A, B = self.linearize()
        dU = np.zeros((self.nC, CNP))
        np.add.at(dU, self.j, (A * A).sum(1))
        dV = np.zeros((self.nP, 3))
        np.add.at(dV, self.i, (B * B).sum(1))
        d = np.r_[dU.reshape(-1), dV.reshape(-1)]
        d[:self.nA][~self.free_a] = 1.0
        return d

    def schur(self, N, g, mu, D=None):
        """S and e_a of N + mu diag(D) by a dense solve of the damped point block (D None: TwinKD.schur, mu I)"""
        if D is None:
            return super().schur(N, g, mu)
        nA = self.nA
        Nbb = N[nA:, nA:] + mu * np.diag(D[nA:])
        X = np.linalg.solve(Nbb, np.c_[N[:nA, nA:].T, g[nA:]])
        S = N[:nA, :nA] + mu * np.diag(D[:nA]) - N[:nA, nA:] @ X[:, :nA]
        ea = g[:nA] - N[:nA, nA:] @ X[:, nA]
        return S, ea

    damping, dmin, dmax = IDENTITY, DMIN, DMAX    # the rule of the levmar in progress

    def start_mu(self, tau, N):
        return tau if self.damping == MARQUARDT else super().start_mu(tau, N)

    def damping_diag(self, N):
        return damp_diag(N, self.dmin, self.dmax) if self.damping == MARQUARDT else super().damping_diag(N)

    def levmar(self, max_iter=20, init_mu=0.0, stop_small=True, damping=MARQUARDT, dmin=DMIN, dmax=DMAX):
        """TwinKD.levmar with N + mu D.  damping = IDENTITY: D = 1 and mu_0 = tau max diag (the log of TwinKD.levmar);
        MARQUARDT: D = damp_diag(N) of every linearization and mu_0 = tau."""
        self.damping, self.dmin, self.dmax = damping, dmin, dmax
        return super().levmar(max_iter, init_mu, stop_small)
