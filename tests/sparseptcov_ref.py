"""Host reference of psba_sparse_point_covariance (kernels_free_pcg_points.hip; not a test file, no GPU): the
joint covariance of chosen 3-D points on the block-sparse free-intrinsics route.  It stands on sparsecov_ref.py,
freecov_ref.py, freepcg_ref.py, cov_ref.py and assembly_ref.py, none of them edited; no constant is fitted to a GPU
result.

The model, stated twice (test_sparseptcov_ref.py holds the two against each other):
  schur_points    block (a, b) = scale [ delta_ab V*_a^-1 + Y_a^T S(mu)^-1 Y_b ], V*_i = V_i + mu D_i, Y_ij = W_ij V*_i^-1,
                  S(mu)^-1 = cov_ref.refined_inverse of the live S scaled by powers of two; a held point: zeros
  dense_points    the point rows and columns of the inverse of the full damped normal matrix on the live coordinates
                  (freecov_ref.reduced_dense)
The device's arithmetic, on the device's own inputs:
  rhs             b_{i,c}: column c of Y_ij in the rows of camera j in cams(i), every other row +0.0
  column_judges   sparsecov_ref's column bound carried to ||b|| != 1: ||S x - b||_2 <= (tol + C_GAP gap_unit) ||b||_2,
                  gap_unit = eps iters || |S| |x| ||_inf / ||b||_inf as freepcg_ref defines it.  C_GAP NEEDS NO NEW
                  MEASUREMENT: freepcg_ref measured it (GAP_RATIO 0.540 / 0.312, C_GAP = 4) over pcg_ref.QUALITY with the
                  general right-hand sides of freepcg_ref.rhs, not with unit vectors.  test_sparseptcov_ref.py measures
                  the float64 twin's gap on Y right-hand sides again (worst 0.029 of a unit on the inputs there) and
                  holds it to C_GAP
  contract        the contraction rule in long double and its entrywise bound (below); `fault` injects one of FAULTS
                  (all but "block-diagonal", which is a fault of the solve and lives in schur_points alone)
  exact_parts     C bit-symmetric; a held point's rows and columns of C, its rows of cols, its iters and relres zero

The bound of the contraction.  An entry of block (a, b) is scale (v + sum_{k=1}^{n} y_k x_k), n = cnp |cams(a)|, v the
entry of V*_a^-1 on a diagonal block and absent otherwise.  The device forms the n products and adds them in one chain
(each product exact inside the fused multiply-add of the matrix pipe, or rounded once), adds v and multiplies by scale:
a term passes through at most n + 2 roundings, so by the standard forward bound of a recursive sum
    |C_dev - C_exact| <= gamma(n + 2) scale (|v| + sum |y_k| |x_k|),   gamma(k) = k u / (1 - k u),  u = 2^-53.
V*^-1 itself is the closed form of a 3 x 3 inverse in fp64: assembly_ref.vinv returns the exact inverse of the damped
block and the closed form's envelope, which widens the diagonal blocks by scale times that envelope (freecov_ref's
point judge does the same)."""
import numpy as np

import assembly_ref as ar
import cov_ref as cr
import free_ref as fr
import freecov_ref as fc
import freepcg_ref as fp
import prior_ref as pr
import sparsecov_ref as sc
from freepcg_ref import LD, EPS, C_GAP  # noqa: F401

U = 2.0 ** -53
FAULTS = ("block-diagonal", "no-vinv", "vinv-off-diagonal", "scale-twice", "held-vinv", "mu-identity")


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the model, twice (fp64 inputs from the route's dense system) ------------------------------------------------------

def _pieces(rt, mu, rule):
    """(Caa_unit [nA, nA] = E S(mu)^-1 E^T by the refined inverse, Vinv [nP, 3, 3] (held: of the undamped placeholder
    system, used by a fault only), Y {i: (rows, Y_i [cnp m, 3])}, kappa of the scaled live S)"""
    N0, _ = pr.dense_system(rt)
    nA, nP, cnp = rt.nA, rt.nP, rt.cnp
    dead = fc.full_map(rt)[0] < 0
    N = N0.copy()
    N[dead, :] = 0.0
    N[:, dead] = 0.0
    src = fc.coord_map(rt)
    live = np.flatnonzero(src == np.arange(nA))
    E = fc.expansion(src, live)
    order = np.argsort(rt.i, kind="stable")
    ptr = np.searchsorted(rt.i[order], np.arange(nP + 1))
    S = N[:nA, :nA].copy()
    Vinv = np.zeros((nP, 3, 3))
    Y = {}
    for i in range(nP):
        b = slice(nA + 3 * i, nA + 3 * i + 3)
        if rt.held_pts[i]:
            V0 = N0[b, b]
            Vinv[i] = np.linalg.inv(V0 + mu * np.diag(fc._damp(np.diag(V0), rule)) + (0.0 if np.any(V0) else 1.0) * np.eye(3))
            continue
        V = N[b, b]
        Vinv[i] = np.linalg.inv(V + mu * np.diag(fc._damp(np.diag(V), rule)))
        cams = rt.j[order[ptr[i]:ptr[i + 1]]]
        rows = (cnp * cams[:, None] + np.arange(cnp)[None, :]).reshape(-1)
        W = N[rows, b]
        Y[i] = (rows, W @ Vinv[i])
        S[np.ix_(rows, rows)] -= Y[i][1] @ W.T
    Sr = E.T @ S @ E
    Sr = 0.5 * (Sr + Sr.T) + mu * np.diag(fc._damp(np.diag(E.T @ N[:nA, :nA] @ E), rule))
    D = 2.0 ** np.round(-0.5 * np.log2(np.diag(Sr)))
    A = D[:, None] * Sr * D[None, :]
    ref, _ = cr.refined_inverse(A)
    X = (D.astype(LD)[:, None] * ref * D.astype(LD)[None, :]).astype(np.float64)
    w = np.linalg.eigvalsh(A)
    return E @ X @ E.T, Vinv, Y, float(w[-1] / w[0])


def schur_points(rt, sel, mu=0.0, rule=fr.NO_RULE, scale=1.0, fault=None):
    """(C [3 n, 3 n] by the Schur formula, kappa of the scaled live S)"""
    Caa, Vinv, Y, kappa = _pieces(rt, mu, fr.NO_RULE if fault == "mu-identity" else rule)
    cnp = rt.cnp
    if fault == "block-diagonal":
        Caa = Caa * np.kron(np.eye(rt.nA // cnp), np.ones((cnp, cnp)))
    n = len(sel)
    C = np.zeros((3 * n, 3 * n))
    for a, ia in enumerate(sel):
        for b, ib in enumerate(sel):
            if rt.held_pts[ia] or rt.held_pts[ib]:
                if fault == "held-vinv" and a == b:
                    C[3 * a:3 * a + 3, 3 * a:3 * a + 3] = scale * Vinv[ia]
                continue
            (ra, Ya), (rb, Yb) = Y[ia], Y[ib]
            blk = Ya.T @ Caa[np.ix_(ra, rb)] @ Yb
            if (a == b and fault != "no-vinv") or (a != b and fault == "vinv-off-diagonal"):
                blk = blk + Vinv[ia]
            C[3 * a:3 * a + 3, 3 * b:3 * b + 3] = scale * blk
    if fault == "scale-twice":
        C = scale * C
    return C, kappa


def dense_points(rt, sel, mu=0.0, rule=fr.NO_RULE, scale=1.0):
    """(C [3 n, 3 n], kappa): the chosen point rows and columns of freecov_ref.reduced_dense"""
    C, kappa = fc.reduced_dense(rt, mu, rule, scale)
    q = (rt.nA + 3 * np.asarray(sel)[:, None] + np.arange(3)[None, :]).reshape(-1)
    return C[np.ix_(q, q)], kappa


def sigma_error(got, want):
    """max |got - want|_rc / sqrt(want_rr want_cc) over rows and columns with want_rr > 0; inf if a zero-variance row or
    column of `want` is not zero in `got`"""
    return fc.scaled_error(got, want)


# ---- the device's arithmetic on the device's own inputs ------------------------------------------------------------------

def tracks(i_of_obs, nP):
    """ptr [nP + 1] of the point-major observations"""
    i_of_obs = np.asarray(i_of_obs)
    assert np.all(np.diff(i_of_obs) >= 0)
    return np.searchsorted(i_of_obs, np.arange(nP + 1))


def rhs(Y, ptr, j_of_obs, i, c, cnp, nA):
    """b_{i,c} [nA] from Y [nO, cnp, 3]"""
    b = np.zeros(nA)
    for o in range(ptr[i], ptr[i + 1]):
        b[cnp * j_of_obs[o]:cnp * j_of_obs[o] + cnp] = Y[o, :, c]
    return b + 0.0


def solve_columns(S, n_cams, blocks, Y, ptr, j_of_obs, sel, held_pts, tol, max_iter, c, dtype=np.float64):
    """the float64 twin of the solve: (cols [3 n, nA], iters, relres) by freepcg_ref.twin_pcg per column; a held point
    and a right-hand side of zeros: zero rows, 0 iterations, relres 0"""
    nA = c * n_cams
    cols, iters, relres = np.zeros((3 * len(sel), nA)), np.zeros(3 * len(sel), dtype=np.int64), np.zeros(3 * len(sel))
    for a, i in enumerate(sel):
        if held_pts is not None and held_pts[i]:
            continue
        for k in range(3):
            b = rhs(Y, ptr, j_of_obs, i, k, c, nA)
            if not np.any(b):
                continue
            t = fp.twin_pcg(S, n_cams, blocks, b, tol, max_iter, c, dtype)
            cols[3 * a + k], iters[3 * a + k], relres[3 * a + k] = t["x"], t["iters"], t["relres"]
    return cols, iters, relres


def column_judges(op, cols, Y, ptr, j_of_obs, sel, held_pts, iters, tol, cnp):
    """per column (found ||b - S x||_2 / ||b||_2 in long double, allowed tol + C_GAP gap_unit, ||b||_2); a held point's
    columns and those with b = 0: (0, 0, 0).  op: freepcg_ref.ListOp (long double) of the device's blocks"""
    nA = cnp * op.n_cams
    out = np.zeros((3 * len(sel), 3))
    for a, i in enumerate(sel):
        if held_pts is not None and held_pts[i]:
            continue
        for k in range(3):
            b = rhs(Y, ptr, j_of_obs, i, k, cnp, nA)
            if not np.any(b):
                continue
            tr, gap = fp.list_relres_and_gap(op, cols[3 * a + k], b, int(iters[3 * a + k]))
            out[3 * a + k] = tr, tol + C_GAP * gap, float(np.linalg.norm(b))
    return out


def contract(cols, V, Y, ptr, j_of_obs, sel, held_pts, mu, rule, scale, cnp, fault=None):
    """(C [3 n, 3 n] in long double by the rule of the verb, the entrywise bound [3 n, 3 n]) from the solved columns
    [3 n, nA], the stored V [nP, 3, 3] (undamped) and Y [nO, cnp, 3]: block (a, b), a >= b, from the columns of sel[b],
    mirrored; of a diagonal block the lower triangle"""
    n = len(sel)
    Vi, Venv = ar.vinv(fc.damped_V(V, mu, fr.NO_RULE if fault == "mu-identity" else rule))
    C = np.zeros((3 * n, 3 * n), dtype=LD)
    B = np.zeros((3 * n, 3 * n))
    held = np.zeros(len(V), dtype=bool) if held_pts is None else np.asarray(held_pts).astype(bool)
    for b in range(n):
        for a in range(b, n):
            ia, ib = sel[a], sel[b]
            if held[ia] or held[ib]:
                if fault == "held-vinv" and a == b:
                    C[3 * a:3 * a + 3, 3 * a:3 * a + 3] = LD(scale) * Vi[ia]
                continue
            obs = np.arange(ptr[ia], ptr[ia + 1])
            rows = (cnp * np.asarray(j_of_obs)[obs][:, None] + np.arange(cnp)[None, :]).reshape(-1)
            Ya = ar.ld(Y[obs]).reshape(-1, 3)                                  # [cnp m, 3]
            Xb = ar.ld(cols[3 * b:3 * b + 3][:, rows]).T                       # [cnp m, 3]: column c = x_{b,c}
            T = Ya.T @ Xb
            env = (np.abs(Ya).T @ np.abs(Xb)).astype(np.float64)
            extra = np.zeros((3, 3))
            if (a == b and fault != "no-vinv") or (a != b and fault == "vinv-off-diagonal"):
                T = T + Vi[ia]
                env = env + np.abs(Vi[ia]).astype(np.float64)
                extra = scale * Venv[ia]
            T = LD(scale) * T
            bound = gamma(rows.size + 2) * scale * env + extra
            if a == b:
                T = np.tril(T) + np.tril(T, -1).T
                bound = np.tril(bound) + np.tril(bound, -1).T
            C[3 * a:3 * a + 3, 3 * b:3 * b + 3] = T
            C[3 * b:3 * b + 3, 3 * a:3 * a + 3] = T.T
            B[3 * a:3 * a + 3, 3 * b:3 * b + 3] = bound
            B[3 * b:3 * b + 3, 3 * a:3 * a + 3] = bound.T
    if fault == "scale-twice":
        C = LD(scale) * C
    return C, B


def contract_ratio(C, want, bound):
    """the worst |C - want| / bound; an entry with a zero bound must be equal (inf otherwise)"""
    err = np.abs(np.asarray(C).astype(LD) - want).astype(np.float64)
    if np.any(err[bound == 0.0] != 0.0):
        return float("inf")
    return float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0


def exact_parts(C, info, sel, held_pts):
    """list of what is wrong with the exact parts"""
    bad = []
    Cb = np.ascontiguousarray(C, dtype=np.float64).view(np.int64)
    if not np.array_equal(Cb, Cb.T):
        bad.append("C is not bit-symmetric")
    held = np.repeat(np.asarray([bool(held_pts[i]) if held_pts is not None else False for i in sel]), 3)
    if not (sc.plus_zero(C[held, :]) and sc.plus_zero(C[:, held])):
        bad.append("a held point's row or column of C is not +0.0")
    if info.get("cols") is not None and not sc.plus_zero(info["cols"][held]):
        bad.append("a held point's row of cols is not +0.0")
    if np.any(info["iters"][held] != 0) or not sc.plus_zero(info["relres"][held]):
        bad.append("a held point's iters or relres is not 0")
    return bad
