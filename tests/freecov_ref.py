"""Host reference of the covariance with free intrinsics (psba_free_covariance_compute; not a test file).
It stands on weight_ref.py, prior_ref.py, held_ref.py, shared_ref.py, cov_ref.py and assembly_ref.py, none of them
edited; no constant is fitted to a GPU result.  A route is a weight_ref.WeightRoute or WeightSharedRoute (zero priors
and no loss where a case has none): its blocks carry the mask, the holds and the weights, its priors the information.

Two statements of the model (include/psba_hip.h), kept apart so that a test can hold one against the other:
  reduced_dense     held and masked columns deleted, the groups as a parametrisation J E, the priors' information
                    added, mu D, one dense inverse, then embedded with zeros and expanded over the groups
  schur_statement   X = S(mu)^-1 on the live coordinates of the folded S, C_aa = scale E X E^T,
                    C_bb,i = scale V*_i^-1 + sum_jk Y_ij^T C_jk Y_ik
Judges of the device's arithmetic on the device's own inputs:
  inverse_judge     an error in units of the standard deviations, max |X - X_ref|_rc / sqrt(X_ref,rr X_ref,cc), with
                    X_ref = cov_ref.refined_inverse of D S D, D = powers of two nearest 1 / sqrt(diag S) (the scaling is
                    exact and is undone exactly); the yardstick is numpy's fp64 inverse of the same D S D, unscaled, and
                    the device may be at most MARGIN = 16 times max(yardstick, n eps) -- 7h's margin for another block
                    size and summation order.  S at mu = 0 is badly scaled (7camsvarK, {f, k1, k2}, poses 0 and 1 held:
                    kappa 3.7e15, 3.1e5 once scaled by its diagonal), which is why 7h's normwise error does not serve
  point_judges      cov_ref.point_judges generalised to CNP: T = (CNP m)^2 + 1 terms, bound = 2 (T + 4) eps envelope,
                    the first term from the hook's V: the exact inverse of V*, widened by scale times the envelope
                    assembly_ref.vinv returns for the closed form
"""
import numpy as np

import assembly_ref as ar
import cov_ref as cr
import free_ref as fr
import prior_ref as pr

LD = ar.LD
EPS = cr.EPS
MARGIN = 16.0
FAULTS = ("folded-zero", "held-placeholder", "mu-identity", "no-cross", "scale-twice")


# ---- the coordinate map ------------------------------------------------------------------------------------------------

def coord_map(rt):
    """src [nA]: -1 for a masked or held coordinate, the coordinate itself when it is live, the representative's
    coordinate for one that is folded away"""
    src = np.asarray(getattr(rt, "phi", np.arange(rt.nA)), dtype=np.int64).copy()
    src[rt.held] = -1
    return src


def full_map(rt):
    """coord_map over all nT coordinates (a held point: -1) and the live ones among them"""
    b = rt.nA + np.arange(rt.nB)
    b[rt.held_b] = -1
    src = np.r_[coord_map(rt), b]
    return src, np.flatnonzero(src == np.arange(rt.nT))


def expansion(src, live):
    """E [n, live.size]: row t copies the live coordinate src[t]; zero rows where src is -1"""
    pos = -np.ones(src.size, dtype=np.int64)
    pos[live] = np.arange(live.size)
    E = np.zeros((src.size, live.size))
    t = np.flatnonzero(src >= 0)
    E[t, pos[src[t]]] = 1.0
    return E


def _damp(diag, rule):
    return rule.clamp(diag) if rule.marquardt else np.ones(diag.size)


def scaled_inverse(M):
    """(M^-1 through the scaling by M's own diagonal, kappa_2 of the scaled matrix)"""
    d = 1.0 / np.sqrt(np.diag(M))
    A = d[:, None] * M * d[None, :]
    w = np.linalg.eigvalsh(A)
    return d[:, None] * np.linalg.inv(A) * d[None, :], float(w[-1] / w[0])


# ---- the two statements (fp64) -----------------------------------------------------------------------------------------

def reduced_dense(rt, mu=0.0, rule=fr.NO_RULE, scale=1.0):
    """(C [nT, nT] embedded and expanded, kappa_2 of the reduced system scaled by its diagonal)"""
    N, _ = pr.dense_system(rt)
    src, live = full_map(rt)
    E = expansion(src, live)
    Nr = E.T @ N @ E
    M = Nr + mu * np.diag(_damp(np.diag(Nr), rule))
    X, kappa = scaled_inverse(M)
    return scale * (E @ X @ E.T), kappa


def schur_statement(rt, mu=0.0, rule=fr.NO_RULE, scale=1.0, fault=None):
    """(C_aa [nA, nA], C_bb [nP, 3, 3]) through the Schur complement.  Faults for test_freecov_ref.py: "folded-zero"
    (folded-away rows left zero), "held-placeholder" (a held coordinate given 1 / placeholder), "mu-identity" (mu I where
    Marquardt's D belongs), "no-cross" (the j != k terms of a point missing), "scale-twice"."""
    N, _ = pr.dense_system(rt)
    nA, nP, cnp = rt.nA, rt.nP, rt.cnp
    srcT, _ = full_map(rt)
    dead = srcT < 0
    N = N.copy()
    N[dead, :] = 0.0
    N[:, dead] = 0.0
    src = coord_map(rt)
    live = np.flatnonzero(src == np.arange(nA))
    E = expansion(src, live)
    use = fr.NO_RULE if fault == "mu-identity" else rule
    order = np.argsort(rt.i, kind="stable")
    ptr = np.searchsorted(rt.i[order], np.arange(nP + 1))
    S = N[:nA, :nA].copy()
    Vinv = np.zeros((nP, 3, 3))
    Y = {}
    for i in range(nP):
        if rt.held_pts[i]:
            continue
        b = slice(nA + 3 * i, nA + 3 * i + 3)
        V = N[b, b]
        Vinv[i] = np.linalg.inv(V + mu * np.diag(_damp(np.diag(V), use)))
        cams = rt.j[order[ptr[i]:ptr[i + 1]]]
        rows = (cnp * cams[:, None] + np.arange(cnp)[None, :]).reshape(-1)
        W = N[rows, b]
        Y[i] = (rows, W @ Vinv[i])
        S[np.ix_(rows, rows)] -= Y[i][1] @ W.T
    Sr = E.T @ S @ E
    Da = _damp(np.diag(E.T @ N[:nA, :nA] @ E), use)
    X, _ = scaled_inverse(Sr + mu * np.diag(Da))
    Caa = scale * (E @ X @ E.T)
    if fault == "folded-zero":
        away = np.flatnonzero((src >= 0) & (src != np.arange(nA)))
        Caa[away, :] = 0.0
        Caa[:, away] = 0.0
    if fault == "held-placeholder":
        Caa[rt.held, rt.held] = scale / (1.0 + mu)
    Cbb = scale * Vinv
    for i, (rows, Yi) in Y.items():
        C = Caa[np.ix_(rows, rows)]
        if fault == "no-cross":
            keep = np.kron(np.eye(rows.size // cnp), np.ones((cnp, cnp)))
            C = C * keep
        Cbb[i] = Cbb[i] + Yi.T @ C @ Yi
    if fault == "scale-twice":
        Caa, Cbb = scale * Caa, scale * Cbb
    return Caa, Cbb


def split(C, rt):
    """C [nT, nT] -> (C_aa, the diagonal point blocks [nP, 3, 3])"""
    nA = rt.nA
    return C[:nA, :nA], np.stack([C[nA + 3 * i:nA + 3 * i + 3, nA + 3 * i:nA + 3 * i + 3] for i in range(rt.nP)])


def scaled_error(got, want):
    """max |got - want|_rc / sqrt(want_rr want_cc) over the rows and columns with want_rr > 0 (square blocks [..., n, n])"""
    got, want = np.asarray(got), np.asarray(want)
    d = np.sqrt(np.einsum("...kk->...k", want).astype(np.float64))
    den = d[..., :, None] * d[..., None, :]
    err = np.abs(got.astype(LD) - want.astype(LD)).astype(np.float64)
    if np.any(err[den == 0.0] != 0.0):  # an entry of a zero-variance row or column differs
        return float("inf")
    return float((err[den > 0] / den[den > 0]).max()) if np.any(den > 0) else 0.0


# ---- the inverse judge -------------------------------------------------------------------------------------------------

def inverse_judge(S, X):
    """S [n, n] the live part of the device's S (bit-symmetric), X the device's inverse of it: (the device's scaled
    error, the yardstick's, the allowed MARGIN max(yardstick, n eps), kappa_2 of D S D)"""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    assert np.array_equal(S, S.T)
    D = 2.0 ** np.round(-0.5 * np.log2(np.diag(S)))
    A = D[:, None] * S * D[None, :]
    assert np.array_equal(A / D[:, None] / D[None, :], S), "the scaling is not exact"
    ref, _ = cr.refined_inverse(A)
    ref = ar.ld(D)[:, None] * ref * ar.ld(D)[None, :]
    yard_X = D[:, None] * np.linalg.inv(A) * D[None, :]
    sd = np.sqrt(np.diag(ref))
    den = sd[:, None] * sd[None, :]

    def err(Z):
        return float((np.abs(np.asarray(Z).astype(LD) - ref) / den).max())
    w = np.linalg.eigvalsh(A)
    yard = err(yard_X)
    return err(X), yard, MARGIN * max(yard, n * EPS), float(w[-1] / w[0])


# ---- the point judge ---------------------------------------------------------------------------------------------------

def damped_V(V, mu, rule):
    """V*_i in fp64 as the kernels form it from the stored V [nP, 3, 3]: v + mu, or fma(mu, clamp(v), v), on the diagonal"""
    Vs = np.array(V, dtype=np.float64)
    k = np.arange(3)
    d = ar.ld(Vs[:, k, k])
    add = LD(mu) * ar.ld(rule.clamp(Vs[:, k, k])) if rule.marquardt else LD(mu)
    Vs[:, k, k] = (d + add).astype(np.float64)
    return Vs


def point_judges(i_of_obs, j_of_obs, V, Y, Caa, mu, rule, scale, points, cnp):
    """For every point of `points`: (want [3, 3] float64, bound [3, 3], want as long doubles) of
    C_bb,i = scale V*^-1 + sum_{j,k} Y_ij^T C_jk Y_ik on the device's own fp64 inputs: V [nP, 3, 3] undamped and
    Y [nO, cnp, 3] from psba_get_free_point_blocks, Caa from the device.  The observations are point-major."""
    i_of_obs = np.asarray(i_of_obs)
    assert np.all(np.diff(i_of_obs) >= 0)
    Vi, Venv = ar.vinv(damped_V(V, mu, rule))
    out = {}
    for i in points:
        obs = np.arange(np.searchsorted(i_of_obs, i, "left"), np.searchsorted(i_of_obs, i, "right"))
        cams = np.asarray(j_of_obs)[obs]
        m = obs.size
        rows = (cnp * cams[:, None] + np.arange(cnp)[None, :]).reshape(-1)
        Yl = ar.ld(Y[obs]).reshape(m * cnp, 3)
        Cl = ar.ld(Caa[np.ix_(rows, rows)])
        first = LD(scale) * Vi[i]
        # the terms Y[p, a] C[p, q] Y[q, b] and their magnitudes, summed over p and q in long doubles
        want = first + Yl.T @ (Cl @ Yl)
        env = (np.abs(first) + np.abs(Yl).T @ (np.abs(Cl) @ np.abs(Yl))).astype(np.float64)
        T = (cnp * m) ** 2 + 1
        bound = 2.0 * (T + 4) * EPS * env + scale * Venv[i]
        out[int(i)] = (want.astype(np.float64), bound, want)
    return out
