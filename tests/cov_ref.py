"""Host reference of the covariance of the estimate (not a test file), on top of tests/fixed_twin.py.

Definition (include/psba_hip.h): at the current parameters, with the whitened, loss-weighted, masked linearization,
N = J^T J on the free blocks and C = scale (N + mu I)^-1 on the free entries, zero on rows and columns of fixed blocks.
Two statements of it are kept apart so that a test can hold one against the other:
  dense_covariance   the columns of fixed blocks really deleted, one dense inverse, embedded with zeros
  schur_covariance   C_aa = scale S(mu)^-1 on the free cameras; C_bb,i = scale V*_i^-1 + sum_jk Y_ij^T C_jk Y_ik
Judges of the device's arithmetic on the device's own inputs:
  refined_inverse    an extended-precision inverse of a given fp64 matrix
  point_judges       the point formula per entry: the long-double sum of its terms and the sum of their magnitudes
"""
import numpy as np

import dense_ref as dr
from fixed_twin import FixedTwin

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def dense_covariance(t, mu=0.0, scale=1.0):
    """(C [nA + nB]^2 embedded, kappa_2 of the reduced N_f + mu I) for a FixedTwin t."""
    Jf, free = t.reduced_jacobian()
    N = Jf.T @ Jf + mu * np.eye(free.size)
    w = np.linalg.eigvalsh(N)
    C = np.zeros((t.nA + t.nB, t.nA + t.nB))
    C[np.ix_(free, free)] = scale * np.linalg.inv(N)
    return C, float(w[-1] / w[0])


def schur_pieces(t, mu):
    """U [nC,6,6], V* [nP,3,3] (mu added), W [nO,6,3] of the masked linearization"""
    _, A, B = t.linearize()
    At = np.transpose(A, (0, 2, 1))
    U = np.zeros((t.nC, 6, 6))
    V = np.zeros((t.nP, 3, 3))
    np.add.at(U, t.j, At @ A)
    np.add.at(V, t.i, np.transpose(B, (0, 2, 1)) @ B)
    return U, V + mu * np.eye(3)[None], At @ B


def schur_covariance(t, mu=0.0, scale=1.0):
    """(C_aa [nA, nA], C_bb [nP, 3, 3]) through the Schur complement, fixed blocks zero."""
    U, Vs, W = schur_pieces(t, mu)
    free_p = ~t.fp
    Vinv = np.zeros_like(Vs)
    Vinv[free_p] = np.linalg.inv(Vs[free_p])
    Y = W @ Vinv[t.i]  # zero for fixed points (B = 0) and fixed cameras (A = 0)
    fa = np.repeat(~t.fc, 6)
    Caa = np.zeros((t.nA, t.nA))
    if fa.any():
        S = np.zeros((t.nA, t.nA))
        for j in range(t.nC):
            S[6 * j:6 * j + 6, 6 * j:6 * j + 6] = U[j] + mu * np.eye(6)
        for i in range(t.nP):
            obs = np.flatnonzero(t.i == i)
            for a in obs:
                for b in obs:
                    S[6 * t.j[a]:6 * t.j[a] + 6, 6 * t.j[b]:6 * t.j[b] + 6] -= Y[a] @ W[b].T
        idx = np.flatnonzero(fa)
        Caa[np.ix_(idx, idx)] = scale * np.linalg.inv(S[np.ix_(idx, idx)])
    Cbb = scale * Vinv
    for i in np.flatnonzero(free_p):
        obs = np.flatnonzero(t.i == i)
        for a in obs:
            for b in obs:
                ja, jb = t.j[a], t.j[b]
                Cbb[i] += Y[a].T @ Caa[6 * ja:6 * ja + 6, 6 * jb:6 * jb + 6] @ Y[b]
    return Caa, Cbb


def refined_inverse(S, tol=1e-15, max_iter=20):
    """(X as long doubles, iterations): X <- X + X0 (I - S X) from LAPACK's inverse X0, X held in np.longdouble, until
    two iterates agree to tol relative (max norm).  X0 (I - S X) contracts the error by about kappa eps per step.
    The residual I - S X is formed column by column with dense_ref.residual's error-free products and sums (about 106
    bits): a plain long-double product leaves kappa 1e-19 n of noise in it, and at kappa = 1.4e9 (54 cameras, mu = 0)
    the iterates then keep moving by 3e-15 and never agree to 1e-15."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    X0 = np.linalg.inv(S)
    I = np.eye(n)
    X = X0.astype(LD)
    X0 = X0.astype(LD)
    for it in range(1, max_iter + 1):
        hi = X.astype(np.float64)
        lo = (X - hi.astype(LD)).astype(np.float64)
        R = np.empty((n, n))
        for c in range(n):
            R[:, c] = dr.residual(S, (hi[:, c], lo[:, c]), I[:, c], use_ld=False)
        Xn = X + X0 @ R.astype(LD)
        done = float(np.abs(Xn - X).max()) <= tol * float(np.abs(Xn).max())
        X = Xn
        if done:
            return X, it
    raise AssertionError(f"refined_inverse: no agreement to {tol} after {max_iter} iterations")


def embedded_inverse(S, free):
    """the refined inverse of S[free, free] embedded with zeros (long doubles), and the iterations it took"""
    idx = np.flatnonzero(free)
    X, it = refined_inverse(S[np.ix_(idx, idx)])
    out = np.zeros(S.shape, dtype=LD)
    out[np.ix_(idx, idx)] = X
    return out, it


def point_judges(i_of_obs, j_of_obs, Vinv, Y, Caa, scale, points):
    """For every point of `points`: (want [3,3] float64 of the long-double sum, bound [3,3]) of
    C_bb,i = scale V*^-1 + sum_{j,k} Y_ij^T C_jk Y_ik on the given fp64 inputs (Vinv [nP,3,3], Y [nO,6,3], Caa).
    A term is one scalar product y c y (or scale vinv); T counts them, the envelope is the sum of their magnitudes and
    bound = 2 (T + 4) eps envelope."""
    out = {}
    i_of_obs = np.asarray(i_of_obs)
    sorted_obs = bool(np.all(np.diff(i_of_obs) >= 0))  # point-major, as the library wants them: a point's run of rows
    for i in points:
        if sorted_obs:
            obs = np.arange(np.searchsorted(i_of_obs, i, "left"), np.searchsorted(i_of_obs, i, "right"))
        else:
            obs = np.flatnonzero(i_of_obs == i)
        cams = j_of_obs[obs]
        Yl = Y[obs].astype(LD)  # [m, 6, 3]
        m = obs.size
        # C blocks [m, m, 6, 6]
        Cb = np.empty((m, m, 6, 6), dtype=LD)
        for a in range(m):
            for b in range(m):
                Cb[a, b] = Caa[6 * cams[a]:6 * cams[a] + 6, 6 * cams[b]:6 * cams[b] + 6]
        first = LD(scale) * Vinv[i].astype(LD)
        # terms[j, k, p, q, a, b] = Y_j[p, a] C_jk[p, q] Y_k[q, b]
        terms = Yl[:, None, :, None, :, None] * Cb[:, :, :, :, None, None] * Yl[None, :, None, :, None, :]
        want = first + terms.sum(axis=(0, 1, 2, 3))
        env = np.abs(first) + np.abs(terms).sum(axis=(0, 1, 2, 3))
        T = 36 * m * m + 1
        out[int(i)] = (want.astype(np.float64), (2.0 * (T + 4) * EPS * env).astype(np.float64), want)
    return out


def twin(prob, fc=None, fp=None, **kw):
    return FixedTwin(prob, fc, fp, **kw)
