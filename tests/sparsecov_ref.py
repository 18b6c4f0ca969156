"""Host reference of psba_sparse_camera_covariance (kernels_free_pcg_many.hip; not a test file, no GPU): the
covariance of chosen cameras on the block-sparse free-intrinsics route, C = scale (S^-1)[sel, sel] from the columns
S x_q = e_q.  Everything is built from what freepcg_ref.py and cov_ref.py hold; no constant is measured here.

  solve_columns   the float64 twin of the multi-column solve: freepcg_ref.twin_pcg once per live chosen coordinate
                  (columns are independent by definition, so the twin of many is the twin of one, many times)
  assemble        the assembly rule, written once: block (a, b) of the chosen list, a >= b, from the columns solved for
                  sel[b], rows of sel[a], mirrored; inside a diagonal block the lower triangle is the matrix; rows and
                  columns of dead coordinates +0.0; C scaled, cols not.  `fault` injects one of FAULTS
  judges          column_residuals (b), exact_parts (e), c_error_and_bound (c)

The bound of c.  Let the live part of S be scaled by D = powers of two nearest 1 / sqrt(diag S) (7l's scaling, exact),
A = D S D, and let column q be returned with ||e_q - S x_q||_2 <= rho_q (what judge b allows: tol + C_GAP gap_unit).
Then x_q - x_q* = -S^-1 r = -D A^-1 D r, so |x_q - x_q*|_r <= D_r ||A^-1||_2 ||D r||_2 <= D_r ||A^-1||_2 max(D) rho_q.
In 7l's sigma-units the entry (r, q) is divided by sqrt(X*_rr X*_qq) with X* the refined inverse.  An entry of C above
the diagonal of the chosen list is the mirror of the one below, so it carries the bound of the column it came from; the
judge allows every entry the larger of its two columns' bounds."""
import numpy as np

import cov_ref as cr
import freepcg_ref as fp
from freepcg_ref import LD, EPS, C_GAP  # noqa: F401

FAULTS = ("dead-placeholder", "no-mirror", "scale-cols")


def with_dead(S, dead, placeholder=1.0):
    """S with the rows and columns of `dead` zero off the diagonal and the placeholder on it (what a masked or held
    coordinate is in the assembled S)"""
    S = np.array(S, copy=True)
    S[dead, :] = 0.0
    S[:, dead] = 0.0
    S[dead, dead] = placeholder
    return S


def chosen_coords(sel, c):
    return (c * np.asarray(sel)[:, None] + np.arange(c)[None, :]).reshape(-1)


def solve_columns(S, n_cams, blocks, sel, live, tol, max_iter, c, dtype=np.float64):
    """(cols [n_sel c, nA] (a dead chosen coordinate: a zero row), iters, relres) by twin_pcg per live column"""
    q_of = chosen_coords(sel, c)
    nA = c * n_cams
    cols = np.zeros((q_of.size, nA))
    iters = np.zeros(q_of.size, dtype=np.int64)
    relres = np.zeros(q_of.size)
    for r, q in enumerate(q_of):
        if not live[q]:
            continue
        e = np.zeros(nA)
        e[q] = 1.0
        t = fp.twin_pcg(S, n_cams, blocks, e, tol, max_iter, c, dtype)
        cols[r], iters[r], relres[r] = t["x"], t["iters"], t["relres"]
    return cols, iters, relres


def assemble(cols, sel, live, scale, c, fault=None, placeholder=1.0):
    """(C [n_sel c, n_sel c], cols as returned) from the solved columns [n_sel c, nA] by the rule of the verb"""
    sel = np.asarray(sel)
    n = sel.size
    q_of = chosen_coords(sel, c)
    lv = np.asarray(live)[q_of]
    cols = np.where(lv[:, None] & np.asarray(live)[None, :], cols, 0.0)
    C = np.zeros((n * c, n * c))
    for b in range(n):
        for a in range(b, n):
            # T[i, nn] = x_(sel[b], nn)[coordinate (sel[a], i)]
            T = cols[c * b:c * b + c, c * sel[a]:c * sel[a] + c].T
            if a == b:
                T = np.tril(T) + np.tril(T, -1).T
            T = scale * T
            C[c * a:c * a + c, c * b:c * b + c] = T
            if fault == "no-mirror" and a != b:
                C[c * b:c * b + c, c * a:c * a + c] = scale * cols[c * a:c * a + c, c * sel[b]:c * sel[b] + c].T
            else:
                C[c * b:c * b + c, c * a:c * a + c] = T.T
    C = C + 0.0
    out = cols + 0.0                                 # (-0.0 + 0.0 = +0.0)
    if fault == "dead-placeholder":
        dead = np.flatnonzero(~lv)
        C[dead, dead] = scale / placeholder
    if fault == "scale-cols":
        out = scale * out
    return C, out


_BURST = {}


def burst_case_unit(name, k, c, q):
    """freepcg_ref.burst_case with the unit right-hand side e_q: a dominant(negative=True) system on which the long-double
    twin's relative residual of column q drops by >= 4x from iteration k - 1 to k (and is still >= 1e-14 there); tol =
    their geometric mean makes that column stop after exactly k iterations, and rounding cannot move the stop.  The
    first delta of BURST_DELTAS that qualifies, or None."""
    key = (name, k, c, q)
    if key not in _BURST:
        n_cams, blocks = fp.fpattern(name)
        e = np.zeros(c * n_cams)
        e[q] = 1.0
        found = None
        for delta in fp.BURST_DELTAS:
            S = fp.dominant(n_cams, blocks, delta, c, 0.0, 7, negative=True)
            h = fp.twin_pcg(S, n_cams, blocks, e, 0.0, k, c, LD)["hist"]
            if len(h) > k and h[k] >= 1e-14 and h[k - 1] >= 4.0 * h[k] and min(h[:k]) > np.sqrt(h[k - 1] * h[k]):
                found = dict(delta=delta, tol=float(np.sqrt(h[k - 1] * h[k])), S=S, hist=h)
                break
        _BURST[key] = found
    return _BURST[key]


# ---- judges ------------------------------------------------------------------------------------------------------------

def plus_zero(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return bool(np.all(a.view(np.int64) == 0))


def exact_parts(C, cols, sel, live, c):
    """list of what is wrong: C bit-symmetric, rows and columns of dead chosen coordinates +0.0 in C, their rows of cols
    +0.0, the dead rows' entries of every column +0.0"""
    q_of = chosen_coords(sel, c)
    lv = np.asarray(live)[q_of]
    bad = []
    Cb = np.ascontiguousarray(C, dtype=np.float64).view(np.int64)
    if not np.array_equal(Cb, Cb.T):
        bad.append("C is not bit-symmetric")
    if not (plus_zero(C[~lv, :]) and plus_zero(C[:, ~lv])):
        bad.append("a dead coordinate's row or column of C is not +0.0")
    if cols is not None:
        if not plus_zero(cols[~lv, :]):
            bad.append("a dead chosen coordinate's row of cols is not +0.0")
        if not plus_zero(cols[:, ~np.asarray(live)]):
            bad.append("a dead coordinate's entry of a column is not +0.0")
    return bad


def allowed_residual(S_abs_times_x_max, iters, tol):
    """tol + C_GAP gap_unit for a unit right-hand side (||b||_2 = ||b||_inf = 1)"""
    return tol + C_GAP * EPS * max(int(iters), 1) * S_abs_times_x_max


def column_residuals(S, cols, sel, live, iters, tol, c):
    """per live chosen coordinate (||e_q - S x_q||_2 in long double, the allowed tol + C_GAP gap_unit); dead: (0, 0).
    S dense [nA, nA]"""
    q_of = chosen_coords(sel, c)
    found, allowed = np.zeros(q_of.size), np.zeros(q_of.size)
    Sl, Sa = S.astype(LD), np.abs(S)
    for r, q in enumerate(q_of):
        if not live[q]:
            continue
        e = np.zeros(S.shape[0])
        e[q] = 1.0
        res = e.astype(LD) - Sl @ cols[r].astype(LD)
        found[r] = float(np.sqrt(res @ res))
        allowed[r] = tol + C_GAP * fp.gap_unit(S, cols[r], e, int(iters[r]))
        assert allowed[r] == allowed_residual(float((Sa @ np.abs(cols[r])).max()), iters[r], tol)
    return found, allowed


def c_error_and_bound(S, C, sel, live, rho, scale, c):
    """dict(found, allowed, ratio, kappa, Cref): found = max |C - C_ref|_rc / sqrt(C_ref,rr C_ref,cc) over the live chosen
    coordinates, C_ref = scale x cov_ref.refined_inverse of the scaled live part of S, exactly unscaled; allowed = the
    largest entry of the module docstring's bound from rho [n_sel c], the residual each column is allowed; ratio = the
    worst error / bound entry by entry (what is asserted <= 1); kappa = kappa_2 of the scaled live S"""
    live = np.asarray(live)
    idx = np.flatnonzero(live)
    pos = -np.ones(live.size, dtype=np.int64)
    pos[idx] = np.arange(idx.size)
    Sl = np.asarray(S, dtype=np.float64)[np.ix_(idx, idx)]
    assert np.array_equal(Sl, Sl.T)
    D = 2.0 ** np.round(-0.5 * np.log2(np.diag(Sl)))
    A = D[:, None] * Sl * D[None, :]
    assert np.array_equal(A / D[:, None] / D[None, :], Sl), "the scaling is not exact"
    ref, _ = cr.refined_inverse(A)
    ref = D.astype(LD)[:, None] * ref * D.astype(LD)[None, :]
    w = np.linalg.eigvalsh(A)
    inv_norm = 1.0 / float(w[0])
    q_of = chosen_coords(sel, c)
    lv = live[q_of]
    ql = pos[q_of[lv]]
    Cref = scale * ref[np.ix_(ql, ql)]
    sd = np.sqrt(np.diag(Cref).astype(np.float64))
    den = sd[:, None] * sd[None, :]
    got = np.asarray(C)[np.ix_(lv, lv)].astype(LD)
    err = np.abs(got - Cref).astype(np.float64) / den
    # |x_q - x_q*|_r <= D_r ||A^-1||_2 max(D) rho_q, times scale; entry (r, q) may be the mirror of (q, r)
    col_bound = scale * np.outer(D[ql], np.asarray(rho)[lv]) * inv_norm * float(D.max())
    bound = np.maximum(col_bound, col_bound.T) / den
    return dict(found=float(err.max()), allowed=float(bound.max()), ratio=float((err / bound).max()),
                kappa=float(w[-1] / w[0]), Cref=Cref.astype(np.float64))
