"""Numpy twin of the damping rules of the free-intrinsics route (psba_set_damping; test-only, no GPU):
TwinKD (tests/freekd_twin.py) with N + mu D in the place of N + mu I.

    D_k = min(max(N_kk, dmin), dmax)            Marquardt's scaling with the clamps of production solvers
    N_kk                                        the diagonal of J^T J, the placeholder 1 at a held coordinate
    point system V + mu diag(D_b), camera diagonal U_kk + mu D_k, gain_den = dp . (mu D dp + g)
    levmar: mu_0 = tau (not tau max diag), everything else lm_loop.cpp as TwinKD.levmar restates it

With D = 1 and mu_0 = tau max diag the loop below is TwinKD.levmar operation by operation (the test pins the logs
equal), so the two rules differ in the twin by exactly what they differ by in the library.
"""
import numpy as np

from freekd_twin import CNP, LmResult, TwinKD

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

    def levmar(self, max_iter=20, init_mu=0.0, stop_small=True, damping=MARQUARDT, dmin=DMIN, dmax=DMAX):
        """TwinKD.levmar with N + mu D.  damping = IDENTITY: D = 1 and mu_0 = tau max diag (the log of TwinKD.levmar);
        MARQUARDT: D = damp_diag(N) of every linearization and mu_0 = tau."""
        STOP, EPS_SQ = 1e-12, 1e-24
        tau = init_mu if init_mu != 0.0 else 1e-3
        res, log = LmResult(), []
        ex, N, g = self.normal()
        res.init_err = ex
        mu, nu, p_L2, first, flag, tries = 0.0, 2, 0.0, True, 0, 0
        itno = 0
        while itno < max_iter and flag == 0:
            if not first:
                _, N, g = self.normal()
            else:
                mu0 = tau if damping == MARQUARDT else tau * self.max_diag(N)
                mu, p_L2, nu, first = mu0, 1e3, 2, False
                res.mu0 = mu
            D = damp_diag(N, dmin, dmax) if damping == MARQUARDT else np.ones(self.nT)
            while True:
                tries += 1
                try:
                    L = np.linalg.cholesky(N + mu * np.diag(D))
                    dp = np.linalg.solve(L.T, np.linalg.solve(L, g))
                except np.linalg.LinAlgError:
                    dp = None
                if dp is not None:
                    dp[:self.nA][~self.free_a] = 0.0
                    dp_L2 = float(dp @ dp)
                    if dp_L2 < p_L2 * STOP * STOP:
                        flag = 1
                        break
                    if dp_L2 >= (p_L2 + STOP) / EPS_SQ:
                        flag = 2
                        break
                    newc = self.cams + dp[:self.nA].reshape(self.nC, CNP)
                    newp = self.pts + dp[self.nA:].reshape(self.nP, 3)
                    new_ex = self.cost(newc, newp)
                    rho = (ex - new_ex) / float(dp @ ((mu * D) * dp + g))
                    log.append([itno, new_ex, rho, mu, 1.0 if rho > 0 else 0.0])
                    if rho > 0:
                        tmp = 2 * rho - 1
                        tmp = 1.0 - tmp * tmp * tmp
                        mu *= tmp if tmp >= 1.0 / 3.0 else 1.0 / 3.0
                        nu = 2
                        self.cams, self.pts = newc, newp
                        p_L2 = float((newc * newc).sum() + (newp * newp).sum())
                        ex = new_ex
                        break
                else:
                    log.append([itno, np.nan, np.nan, mu, -1.0])
                mu *= nu
                if 2.0 * nu > 1e9:
                    flag = 2
                    break
                nu *= 2
            if stop_small and ex <= STOP:
                flag = 3
            itno += 1
        res.flag, res.iters, res.tries, res.final_err, res.mu_final = flag, itno, tries, ex, mu
        return res, np.asarray(log).reshape(-1, 5)
