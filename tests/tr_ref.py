"""Host judges for the trust-region operators of kernels_tr.hip (no GPU): the modified Cholesky (k_cholmod,
k_cholmod_grid), J x and its three dot products (k_jmul).  All arithmetic in np.longdouble (80-bit, assembly_ref.LD_OK);
u = 2^-53 throughout; ratios are reported through assembly_ref.excess.

(a) apost(A, L, lam, delta, beta) -- reference-free, from A and the returned factor alone:
    1. the strict upper triangle of L is exactly zero;
    2. every strictly lower entry: |(L L^T - A)_ij| <= (min(i, j) + 4) u (|L| |L|^T)_ij.  Column j of either route is
       l_ij = (a_ij - sum_(k<j) l_ik l_jk) / l_jj with whatever l_jj the route chose (the block route's triangular
       solve against L_JJ is the same recurrence, columns J, J + 1, J + 2 in turn), so Higham's Lemma 8.4 gives
       a_ij - sum_(k<=j) l_ik l_jk = error with |error| <= gamma(j + 1) sum_(k<=j) |l_ik| |l_jk| (Thm 10.3), whatever
       the order of the sum and with or without fused multiply-adds;
    3. lambda: E_i = sum_(k<=i) L_ik^2 - A_ii in 80-bit from the returned L, |lam - |sum E| / n| <=
       n u sum_i (sum_k L_ik^2 + |A_ii|) / n (at most i + 2 roundings per E_i and n per term of the outer sum,
       counted as n for all);
    4. delta and beta against their 80-bit values within 4 u relative (delta: one add, one product; beta: n^2 - 1, a
       square root, a division, a square root).
(b) mirror(A, L, delta, beta) -- the branches, block column by block column.  From A and the returned columns < J the
    block column is rebuilt in 80-bit as k_cholmod does it: T_JJ and its 3 x 3 factor (a pivot <= 0 fails it), the rows
    below by the triangular solve, any entry > beta (compared without fabs) sends it to the one-column route; there
    l_jj = sqrt(max(|d_j|, delta)), and theta / beta (theta = max_i |c_ij|) when some c_ij / l_jj > beta.  That run
    decides the branch.  The returned diagonal entries are then judged under that branch from the returned entries
    to their left -- inside the block column those of the block column itself, the same recurrence --:
    |l_jj - sqrt(d_j)| <= (j + 4) u (sum_(k<=j) L_jk^2) / l_jj (bound (a) of the entry (j, j) over l_jj; max(|.|, delta)
    is 1-Lipschitz), and on the theta branch |l_jj - theta / beta| <= (j + 4) u max_i (|a_ij| + sum_(k<j) |l_ik| |l_jk|)
    / beta + 6 u l_jj (theta is a maximum of forward-rounded sums; the division, beta's own 4 u and one to spare).
    The strictly lower entries of the block column, divided by l_jj, are (a).2 again and are judged there.
    A comparison whose sides are within UNDECIDED = 1e-9 relative (a pivot: of the magnitude of its sum) is undecided:
    the block column then passes if it matches either branch, and the predicted count of one-column block columns is
    compared with the device's only when nothing was undecided.  The test matrices have no undecided comparison
    (tests/test_tr_ref.py asserts it).
(c) matrices(n): the seeded families spd, shift, over, theta per size.
(d) jx_ref: the 80-bit A_ij x_j + B_ij x_i of the dumped (whitened, weighted, masked) blocks; per entry
    (9 + 2) u sum |a_k x_k| (nine products, eight adds, with room for the order) plus the relative slack of recomputed
    blocks, assembly_ref.JACOBIAN_SLACK (k_jmul recomputes A and B as the default K3 does; under a robust loss
    assembly_ref.robust_jac_slack) -- no new constant.  dots_ref: the three dot products against the 80-bit dots of the
    device's own J x1, J x2: 2 nO u sum |terms| (2 nO terms in any order: lanes, waves, atomics).
cholmod_f64 is k_cholmod in plain fp64 numpy with optional injected faults (tests/test_tr_ref.py)."""
import numpy as np

import assembly_ref as ar

LD = ar.LD
LD_OK = ar.LD_OK
U = 2.0 ** -53
UNDECIDED = 1e-9
ROW_BLOCK = 96  # rows of L L^T per long-double product


def ld(x):
    return np.asarray(x).astype(LD)


# ---- (c) matrix families --------------------------------------------------------------------------------------------

def embed(A, n32):
    """A in the padded reduce buffer ((n32 + 1) x n32, identity padding), flat."""
    n = A.shape[0]
    buf = np.zeros((n32 + 1, n32))
    buf[:n, :n] = A
    buf[n:n32, n:] = np.eye(n32 - n)
    return buf.reshape(-1)


def _base(n, seed):
    B = np.random.default_rng(seed).normal(size=(n, n))
    return B @ B.T


def spd(n, seed):
    """B B^T + n I: no column is modified, L is the plain Cholesky factor."""
    return _base(n, seed) + n * np.eye(n)


def shift(n, s, seed):
    """B B^T - s I: indefinite, pivots away from zero."""
    return _base(n, seed) - s * np.eye(n)


def delta_beta(A):
    """(delta, beta) in extended precision."""
    n = A.shape[0]
    a = np.abs(np.asarray(A, dtype=np.float64))
    gamma = LD(np.diag(a).max())
    off = a.copy()
    np.fill_diagonal(off, 0.0)
    xi = LD(off.max())
    delta = LD(1e-15) * max(xi + gamma, LD(1.0))
    beta = np.sqrt(max(max(gamma, LD(1e-15)), xi / np.sqrt(LD(n) * LD(n) - LD(1.0))))
    return delta, beta


def over(n, Js, seed, factor=4.0):
    """spd, but the diagonal block of block column Js is scaled down (T_JJ -> eps T_JJ, still positive definite) until
    the largest entry of the rows below is factor * beta: the block column factors, is found above beta, is restored
    from its backup and retaken column by column.  Js = n - 3 has no rows below: nothing happens."""
    A = spd(n, seed)
    if Js + 3 >= n:
        return A
    _, beta = delta_beta(A)
    head = A[:Js, :Js]
    left = A[Js:, :Js]
    T = A[Js:, Js:Js + 3] - (left @ np.linalg.solve(head, left[:3].T) if Js else 0.0)
    X = np.linalg.solve(np.linalg.cholesky(T[:3]), T[3:].T).T  # the rows below on the block route
    eps = (X.max() / (factor * float(beta))) ** 2
    assert 0 < eps < 1
    D = (1.0 - eps) * T[:3]
    A[Js:Js + 3, Js:Js + 3] -= 0.5 * (D + D.T)
    return A


def theta(n, js, seed, frac=1e-6):
    """spd, but a_jj of column js is lowered until its pivot d_j is -frac * n: the 3 x 3 factor fails, the column's
    l_jj = sqrt(|d_j|) is small, c_ij / l_jj passes beta and l_jj = theta / beta replaces it."""
    A = spd(n, seed)
    d = A[js, js] - (A[js, :js] @ np.linalg.solve(A[:js, :js], A[:js, js]) if js else 0.0)
    A[js, js] -= d + frac * n
    return A


def matrices(n):
    """name -> (constructor, expectation): expectation 'none' (no block column on the one-column route), 'some',
    ('over', Js) (block column Js is the first to leave the block route, by the restore from the backup) or ('theta', js)."""
    mid = (n // 6) * 3
    if n == 1044:  # two matrices: the host-side 80-bit work is the cost
        return {"shift400": (lambda: shift(n, 400.0, 405), "some"),
                "over1026": (lambda: over(n, 1026, 7), ("over", 1026))}
    out = {"spd": (lambda: spd(n, 3), "none"), "shift3": (lambda: shift(n, 3.0, 14), "some")}
    if n >= 42:
        s = 40.0 if n == 42 else 400.0
        out[f"shift{int(s)}"] = (lambda: shift(n, s, int(s) + (11 if n == 42 else 5)), "some")
    for Js in (0, mid, n - 3):
        out[f"over{Js}"] = (lambda Js=Js: over(n, Js, 7 + Js), ("over", Js) if Js + 3 < n else "none")
    out["theta"] = (lambda: theta(n, mid + 1, 9), ("theta", mid + 1))
    return out


SIZES = {3: 18, 7: 42, 54: 324, 174: 1044}  # cameras -> n


# ---- (a) a posteriori -----------------------------------------------------------------------------------------------

def _lower_products(L):
    """(L L^T in extended precision, |L| |L|^T in double), lower triangles (row blocks; the rest is zero)."""
    n = L.shape[0]
    Lx, aL = ld(L), np.abs(np.asarray(L, dtype=np.float64))
    P = np.zeros((n, n), dtype=LD)
    E = np.zeros((n, n))
    for r0 in range(0, n, ROW_BLOCK):
        r1 = min(n, r0 + ROW_BLOCK)
        P[r0:r1, :r1] = Lx[r0:r1, :r1] @ Lx[:r1, :r1].T
        E[r0:r1, :r1] = aL[r0:r1, :r1] @ aL[:r1, :r1].T
    return P, E


def lambda_ratio(A, L, lam):
    """check (a).3 alone (the routes sum the E_i in different orders, so lambda may differ where L does not)"""
    A = np.asarray(A, dtype=np.float64)
    Lx = ld(np.tril(L))
    n = A.shape[0]
    sq = (Lx * Lx).sum(axis=1)
    Ei = sq - ld(np.diag(A))
    bound = n * U * float(np.sum(sq.astype(np.float64) + np.abs(np.diag(A)))) / n
    return ar.excess(np.array([lam]), np.array([np.abs(Ei.sum()) / n]), np.array([bound]))[0]


def apost(A, L, lam, delta, beta):
    """{quantity: worst bound ratio} of the four a posteriori checks ('upper': 0 or inf)."""
    A = np.asarray(A, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    n = A.shape[0]
    out = {"upper": 0.0 if not np.triu(L, 1).any() and np.isfinite(L).all() else np.inf}
    P, E = _lower_products(np.tril(L))
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    k = np.minimum.outer(np.arange(n), np.arange(n)) + 4
    out["LLt"] = ar.excess(P[low], ld(A)[low], (k * U * E)[low])[0]
    out["lambda"] = lambda_ratio(A, L, lam)
    dx, bx = delta_beta(A)
    out["delta"] = ar.excess(np.array([delta]), np.array([dx]), np.array([4 * U * float(dx)]))[0]
    out["beta"] = ar.excess(np.array([beta]), np.array([bx]), np.array([4 * U * float(bx)]))[0]
    return out


# ---- (b) the mirror -------------------------------------------------------------------------------------------------

def _cmp_gt(x, y, scale=None):
    """x > y as (decision, undecided)"""
    s = abs(y) if scale is None else scale
    return bool(x > y), bool(abs(x - y) <= UNDECIDED * s)


def _ratio(got, want, bound):
    err = abs(float(LD(got) - want))
    return err / bound if bound > 0 else (0.0 if err == 0 else np.inf)


def mirror(A, L, delta, beta):
    """dict(ratio: worst bound ratio of the diagonal entries, single: predicted block columns on the one-column route,
    undecided: block columns with an undecided comparison, log: [(J, 'fail' | 'over', [columns that took theta / beta])]
    for the predicted one-column block columns)."""
    A = np.asarray(A, dtype=np.float64)
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = A.shape[0]
    Ax, Lx, aA, aL = ld(A), ld(L), np.abs(A), np.abs(L)
    bx, dx = LD(beta), LD(delta)
    zero = LD(0.0)
    worst, single, undecided, log = 0.0, 0, [], []
    for J in range(0, n - 2, 3):
        T = Ax[J:, J:J + 3] - Lx[J:, :J] @ Lx[J:J + 3, :J].T
        envT = aA[J:, J:J + 3] + aL[J:, :J] @ aL[J:J + 3, :J].T
        # -- the branch: the 3 x 3 factor and the rows below, from the columns < J alone
        und = False
        fail = False
        l = np.zeros((3, 3), dtype=LD)
        for c in range(3):
            p = T[c, c] - sum((l[c, k] * l[c, k] for k in range(c)), zero)
            env = envT[c, c] + float(sum((l[c, k] * l[c, k] for k in range(c)), zero))
            f, u_ = _cmp_gt(zero, p, env)
            f = f or p == 0
            und |= u_
            if f:
                fail = True
                break
            l[c, c] = np.sqrt(p)
            for r in range(c + 1, 3):
                l[r, c] = (T[r, c] - sum((l[r, k] * l[c, k] for k in range(c)), zero)) / l[c, c]
        over_ = False
        if not fail and J + 3 < n:
            X = np.empty((n - J - 3, 3), dtype=LD)
            X[:, 0] = T[3:, 0] / l[0, 0]
            X[:, 1] = (T[3:, 1] - X[:, 0] * l[1, 0]) / l[1, 1]
            X[:, 2] = (T[3:, 2] - X[:, 0] * l[2, 0] - X[:, 1] * l[2, 1]) / l[2, 2]
            over_ = bool((X > bx).any())
            und |= bool((np.abs(X - bx) <= UNDECIDED * bx).any())
        pred_single = fail or over_
        # -- the returned diagonal entries under a branch, from the returned entries to their left
        def block_route():
            r = 0.0
            for c in range(3):
                j = J + c
                d = Ax[j, j] - Lx[j, :j] @ Lx[j, :j]
                if not (d > 0 and L[j, j] > 0):
                    return np.inf
                r = max(r, _ratio(L[j, j], np.sqrt(d), (j + 4) * U * float(aL[j, :j + 1] @ aL[j, :j + 1]) / L[j, j]))
            return r

        def single_route():
            r, thetas, und1 = 0.0, [], False
            for c in range(3):
                j = J + c
                d = Ax[j, j] - Lx[j, :j] @ Lx[j, :j]
                base = np.sqrt(max(abs(d), dx))
                r_base = _ratio(L[j, j], base, (j + 4) * U * float(aL[j, :j + 1] @ aL[j, :j + 1]) / L[j, j])
                if j + 1 == n:
                    r = max(r, r_base)
                    continue
                cij = Ax[j + 1:, j] - Lx[j + 1:, :j] @ Lx[j, :j]
                lij = cij / base
                ov = bool((lij > bx).any())
                u1 = bool((np.abs(lij - bx) <= UNDECIDED * bx).any())
                th = np.abs(cij).max()
                env = float((aA[j + 1:, j] + aL[j + 1:, :j] @ aL[j, :j]).max())
                r_theta = _ratio(L[j, j], th / bx, (j + 4) * U * env / float(bx) + 6 * U * L[j, j])
                if u1:
                    und1 = True
                    r = max(r, min(r_base, r_theta))
                else:
                    r = max(r, r_theta if ov else r_base)
                if ov:
                    thetas.append(j)
            return r, thetas, und1

        if und:
            rs, thetas, u1 = single_route()
            worst = max(worst, min(block_route(), rs))
            undecided.append(J)
        elif pred_single:
            rs, thetas, u1 = single_route()
            worst = max(worst, rs)
            if u1:
                undecided.append(J)
            single += 1
            log.append((J, "fail" if fail else "over", thetas))
        else:
            worst = max(worst, block_route())
    return dict(ratio=worst, single=single, undecided=undecided, log=log)


# ---- k_cholmod in fp64 numpy, with injected faults --------------------------------------------------------------------

def cholmod_f64(A, fault=None):
    """(L, lam, delta, beta, single) as k_cholmod computes them, in fp64.  fault: None, ("drop", i, j, k): the term k
    left out of the sum of entry (i, j); ("norestore", J): block column J (J = "all": every one) not restored from
    its backup before the single columns; ("fabs",): the comparisons with beta take |x|; ("upper", i, j, v): v left at (i, j), i < j."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    M = A.copy()
    a = np.abs(A)
    gamma = np.diag(a).max()
    off = a.copy()
    np.fill_diagonal(off, 0.0)
    xi = off.max()
    delta = 1e-15 * max(xi + gamma, 1.0)
    beta = np.sqrt(max(max(gamma, 1e-15), xi / np.sqrt(float(n) * n - 1.0)))
    kind = fault[0] if fault else None
    mag = np.abs if kind == "fabs" else (lambda v: v)
    drop = fault[1:] if kind == "drop" else None
    single = 0
    for J in range(0, n - 2, 3):
        bak = M[J:, J:J + 3].copy()
        T = M[J:, J:J + 3] - M[J:, :J] @ M[J:J + 3, :J].T
        if drop and J <= drop[1] < J + 3 and drop[2] < J:
            T[drop[0] - J, drop[1] - J] += M[drop[0], drop[2]] * M[drop[1], drop[2]]
        t = T[:3]
        ok = False
        with np.errstate(invalid="ignore", divide="ignore"):
            if np.isfinite(t[0, 0]) and t[0, 0] > 0:
                l00 = np.sqrt(t[0, 0]); l10 = t[1, 0] / l00; l20 = t[2, 0] / l00
                l11 = t[1, 1] - l10 * l10
                if np.isfinite(l11) and l11 > 0:
                    l11 = np.sqrt(l11)
                    l21 = (t[2, 1] - l20 * l10) / l11
                    l22 = t[2, 2] - l20 * l20 - l21 * l21
                    ok = bool(np.isfinite([l22, l10, l20, l21]).all() and l22 > 0)
        if ok:
            l22 = np.sqrt(l22)
            x0 = T[3:, 0] / l00
            x1 = (T[3:, 1] - x0 * l10) / l11
            x2 = (T[3:, 2] - x0 * l20 - x1 * l21) / l22
            X = np.stack([x0, x1, x2], 1)
            M[J + 3:, J:J + 3] = X
            if not (mag(X) > beta).any():
                M[J:J + 3, J:J + 3] = [[l00, 0, 0], [l10, l11, 0], [l20, l21, l22]]
                M[J:J + 3, J + 3:] = 0.0
                continue
        single += 1
        if not (kind == "norestore" and fault[1] in ("all", J)):
            M[J:, J:J + 3] = bak
        for j in range(J, J + 3):
            d = M[j, j] - M[j, :j] @ M[j, :j]
            ljj = np.sqrt(max(abs(d), delta))
            cij = M[j + 1:, j] - M[j + 1:, :j] @ M[j, :j]
            if drop and drop[1] == j and drop[2] < j:
                cij[drop[0] - j - 1] += M[drop[0], drop[2]] * M[j, drop[2]]
            M[j, j + 1:] = 0.0
            if cij.size and (mag(cij / ljj) > beta).any():
                ljj = np.abs(cij).max() / beta
            M[j + 1:, j] = cij / ljj
            M[j, j] = ljj
    if kind == "upper":
        M[fault[1], fault[2]] = fault[3]
    low = np.tril(M)
    e = (low * low).sum(1) - np.diag(A)
    return M, abs(e.sum()) / n, delta, beta, single


# ---- (d) J x --------------------------------------------------------------------------------------------------------

def jx_ref(JA, JB, x, iidx, jidx, nA, jac_slack=None, fixed=None):
    """(exact [2 nO], bound) of J x from the dumped blocks.  fixed: boolean [nT], entries of x the masked J never reads
    (their blocks are zero in the dump; x may hold anything there)."""
    A = np.asarray(JA, dtype=np.float64).reshape(-1, 2, 6)
    B = np.asarray(JB, dtype=np.float64).reshape(-1, 2, 3)
    x = np.array(x, dtype=np.float64)
    if fixed is not None:
        x[np.asarray(fixed, dtype=bool)] = 0.0
    iidx, jidx = np.asarray(iidx, dtype=np.int64), np.asarray(jidx, dtype=np.int64)
    xc, xp = x[:nA].reshape(-1, 6)[jidx], x[nA:].reshape(-1, 3)[iidx]
    exact = np.einsum("akc,ac->ak", ld(A), ld(xc)) + np.einsum("akc,ac->ak", ld(B), ld(xp))
    mag = np.einsum("akc,ac->ak", np.abs(A), np.abs(xc)) + np.einsum("akc,ac->ak", np.abs(B), np.abs(xp))
    s = np.broadcast_to(ar.JACOBIAN_SLACK if jac_slack is None else np.asarray(jac_slack, dtype=np.float64), (A.shape[0],))
    return exact.reshape(-1), (((9 + 2) * U + s)[:, None] * mag).reshape(-1)


def dots_ref(r1, r2):
    """(exact [3], bound [3]) of r1.r1, r1.r2, r2.r2 for the device's own r1 = J x1, r2 = J x2."""
    a, b = ld(r1).reshape(-1), ld(r2).reshape(-1)
    terms = [a * a, a * b, b * b]
    exact = np.array([t.sum() for t in terms], dtype=LD)
    bound = np.array([a.size * U * float(np.abs(t).sum()) for t in terms])
    return exact, bound
