"""Host reference for the dense solve S dpa = e_a (no GPU): seeded test matrices written straight into the padded
reduce buffer, residuals in extended precision, an iteratively refined reference solution and the normwise
backward error.

The reduce buffer (`red`) is (n32 + 1) x n32 doubles, n32 = n rounded up to 32: rows < n hold S,
rows n .. n32 - 1 the identity padding, row n32 the right-hand side e_a (its first n entries).

Extended precision is np.longdouble where its epsilon is at most 1.1e-19 (x86-64: 64-bit significand); elsewhere a
double-double evaluation (error-free products and sums, Dekker / Knuth) takes its place.  Either way the products are
formed in row chunks, so that a 12 000 x 12 000 matrix never needs a long-double copy of itself."""
import numpy as np

LD = np.longdouble
LD_OK = float(np.finfo(LD).eps) <= 1.1e-19
EPS = float(np.finfo(np.float64).eps)
CHUNK_ELEMS = 1 << 22  # elements of one row chunk (64 MB of long doubles)


def n32_of(n):
    return (n + 31) // 32 * 32


def new_buffer(n):
    """An empty padded buffer for an n x n matrix: zeros, identity padding rows."""
    n32 = n32_of(n)
    buf = np.zeros((n32 + 1, n32))
    buf[np.arange(n, n32), np.arange(n, n32)] = 1.0
    return buf


def matrix(buf, n):
    """The n x n matrix inside a buffer (a view)."""
    return buf[:n, :n]


def set_rhs(buf, n, b):
    buf[-1, :] = 0.0
    buf[-1, :n] = b


def _chunks(n, cols):
    step = max(1, CHUNK_ELEMS // max(cols, 1))
    for r0 in range(0, n, step):
        yield r0, min(n, r0 + step)


def symmetrize_from_lower(A):
    """Copy the strict lower triangle of the square A onto its upper triangle, in place and chunk by chunk."""
    n = A.shape[0]
    for r0, r1 in _chunks(n, n):
        D = A[r0:r1, r0:r1]
        A[r0:r1, r0:r1] = np.tril(D) + np.tril(D, -1).T
        A[r0:r1, r1:] = A[r1:, r0:r1].T


# ---- extended-precision residual ----------------------------------------------------------------------------------

def _split(a):
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _dd_rows(M, x, b):
    """b - M x for the rows of M as (hi, lo) pairs: every product and every pairwise sum error-free, the errors summed
    in double (their own rounding is of order eps^2 of the terms)."""
    P, E = _two_prod(M, -x[None, :])
    lo = E.sum(axis=1)
    hi = np.concatenate([b[:, None], P], axis=1)
    while hi.shape[1] > 1:
        if hi.shape[1] % 2:
            hi = np.concatenate([hi, np.zeros((hi.shape[0], 1))], axis=1)
        hi, e = _two_sum(hi[:, 0::2], hi[:, 1::2])
        lo += e.sum(axis=1)
    return hi[:, 0], lo


def residual(A, x, b, use_ld=None):
    """r = b - A x with the products and sums in extended precision, rounded once to double.  x is a double vector or
    a (hi, lo) pair of them (the refined reference solution), b a double vector."""
    use_ld = LD_OK if use_ld is None else use_ld
    n = A.shape[0]
    xh, xl = x if isinstance(x, tuple) else (np.asarray(x, dtype=np.float64), None)
    r = np.empty(n)
    if use_ld:
        xe = xh.astype(LD) if xl is None else xh.astype(LD) + xl.astype(LD)
        for r0, r1 in _chunks(n, A.shape[1]):
            acc = b[r0:r1].astype(LD) - A[r0:r1].astype(LD) @ xe
            r[r0:r1] = acc.astype(np.float64)
        return r
    for r0, r1 in _chunks(n, 2 * A.shape[1] + 1):
        hi, lo = _dd_rows(A[r0:r1], xh, b[r0:r1])
        if xl is not None:
            lo -= A[r0:r1] @ xl  # a correction term: double precision is enough
        r[r0:r1] = hi + lo
    return r


def matvec_ext(A, x, use_ld=None):
    """A x in extended precision, rounded once (b = A x* for a chosen x*)."""
    return -residual(A, x, np.zeros(A.shape[0]), use_ld)


def norm_inf_mat(A):
    m = 0.0
    for r0, r1 in _chunks(A.shape[0], A.shape[1]):
        m = max(m, float(np.abs(A[r0:r1]).sum(axis=1).max()))
    return m


def backward_error(A, x, b, Anorm=None):
    """eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), the residual in extended precision."""
    r = residual(A, x, b)
    xn = np.abs(x[0] + x[1]).max() if isinstance(x, tuple) else np.abs(x).max()
    Anorm = norm_inf_mat(A) if Anorm is None else Anorm
    den = Anorm * xn + np.abs(b).max()
    return float(np.abs(r).max() / den) if den > 0 else float(np.abs(r).max())


def refined_solution(A, b, steps=2):
    """One LAPACK solve, then `steps` refinement steps with the extended-precision residual.  Returns (hi, lo): the
    solution as an unevaluated sum of two doubles (one double cannot hold it to better than eps / 2)."""
    try:
        from scipy.linalg import lu_factor, lu_solve
        lu = lu_factor(A, check_finite=False)
        solve = lambda v: lu_solve(lu, v, check_finite=False)  # noqa: E731
    except ImportError:
        solve = lambda v: np.linalg.solve(A, v)  # noqa: E731
    hi = solve(b)
    lo = np.zeros_like(hi)
    for _ in range(steps):
        lo = lo + solve(residual(A, (hi, lo), b))
    return hi, lo


def forward_error(x, ref):
    """||x - ref||_inf / ||ref||_inf, ref a (hi, lo) pair."""
    hi, lo = ref
    return float(np.abs((x - hi) - lo).max() / np.abs(hi).max())


# ---- matrix families (all seeded; each returns the padded buffer) --------------------------------------------------

def lowrank_shift(n, kappa, seed, k=64):
    """alpha I + G G^T / k, G n x k Gaussian: every entry dense, O(n^2 k) to build.  alpha is chosen so that
    kappa_2 = (alpha + lambda_max(G^T G / k)) / alpha (k < n: the smallest eigenvalue is alpha; for n <= k the
    shift is taken from the smallest eigenvalue of G G^T / k instead)."""
    rng = np.random.default_rng([seed, n, 1])
    k = min(k, n)
    G = rng.standard_normal((n, k))
    w = np.linalg.eigvalsh(G.T @ G / k)
    if k < n:
        alpha = w[-1] / (kappa - 1.0)
    else:
        alpha = max((w[-1] - kappa * w[0]) / (kappa - 1.0), 0.0)
    buf = new_buffer(n)
    A = matrix(buf, n)
    for r0, r1 in _chunks(n, n):
        A[r0:r1, :r1] = (G[r0:r1] @ G[:r1].T) / k
    symmetrize_from_lower(A)
    A[np.arange(n), np.arange(n)] += alpha
    return buf


def spectrum(n, kappa, seed):
    """Q diag(lambda) Q^T with lambda geometric from 1 down to 1 / kappa: kappa_2 as asked (O(n^3): n <= 2048)."""
    rng = np.random.default_rng([seed, n, 2])
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    Q *= np.sign(np.diag(R))[None, :]
    lam = kappa ** (-np.arange(n) / max(n - 1, 1))
    buf = new_buffer(n)
    A = matrix(buf, n)
    A[:] = (Q * lam[None, :]) @ Q.T
    symmetrize_from_lower(A)
    return buf


def graded(n, seed, kappa_c=100.0, lo=-20, hi=20):
    """D C D, C = lowrank_shift(n, kappa_c), D = diag(2^e) with e uniform in [lo, hi]: the scale spread of a real S,
    where rotation and translation columns differ by orders of magnitude.  Returns (buffer of A, buffer of C, d).
    The scaling is exact (powers of two), so A x = b is C (D x) = D^-1 b."""
    rng = np.random.default_rng([seed, n, 3])
    d = np.ldexp(1.0, rng.integers(lo, hi + 1, size=n))
    cbuf = lowrank_shift(n, kappa_c, seed)
    buf = new_buffer(n)
    A, C = matrix(buf, n), matrix(cbuf, n)
    for r0, r1 in _chunks(n, n):
        A[r0:r1] = d[r0:r1, None] * C[r0:r1] * d[None, :]
    return buf, cbuf, d


def indefinite(n, k, seed, pivot=-1.0, kappa=100.0):
    """An SPD matrix with row and column k zeroed and A[k, k] = pivot (-1 or 0): the leading k x k block stays SPD and
    the elimination of the columns < k never touches row k, so pivot k is exactly `pivot` -- the first bad one."""
    buf = lowrank_shift(n, kappa, seed)
    A = matrix(buf, n)
    A[k, :] = 0.0
    A[:, k] = 0.0
    A[k, k] = pivot
    return buf


def first_bad_pivot(A):
    """Index of the first pivot <= 0 (or not finite) of an unpivoted host Cholesky, None if there is none."""
    L = np.array(A, dtype=np.float64)
    for j in range(L.shape[0]):
        d = L[j, j]
        if not (d > 0.0 and np.isfinite(d)):
            return j
        L[j:, j] /= np.sqrt(d)
        L[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return None


def cond2(A):
    """kappa_2 of a symmetric positive definite matrix (O(n^3))."""
    w = np.linalg.eigvalsh(A)
    return float(w[-1] / w[0])


# ---- right-hand sides ---------------------------------------------------------------------------------------------

def rhs_for(A, seed):
    """b = A x* for a seeded x* (entries of both signs over a few binades), in extended precision and rounded once."""
    rng = np.random.default_rng([seed, A.shape[0], 4])
    xs = rng.standard_normal(A.shape[0]) * np.ldexp(1.0, rng.integers(-4, 5, size=A.shape[0]))
    return matvec_ext(A, xs), xs


def rhs_last(n, value=1.0):
    """b with one non-zero entry, in the last real column."""
    b = np.zeros(n)
    b[n - 1] = value
    return b
