"""Host reference for the block-sparse route of the free-intrinsics camera blocks (psba_set_solver PSBA_SOLVER_SPARSE
under PSBA_CAMERA_FREE_K / PSBA_CAMERA_FREE_KD, kernels_free_pcg.hip; no GPU): the counterparts of tests/pcg_ref.py with
the block size c (11 or 16) as a parameter.  The patterns, the pattern problems, the stop-rule search grid and the
quality sweep are pcg_ref's own (imported, not copied); what depends on the block size is here -- the containers, the
seeded families, the transcription of k_fbsr_diag_inverse's loops, the twin of the conjugate gradients in float64 and
long double, the rounding bounds, and the numpy enumeration of the stored blocks and the row walk that
psba_blockprod_plan_rows must return.

A matrix lives here as the dense symmetric S [c nC, c nC] (n <= 4160); every matrix goes into a handle through
psba_set_sparse_S, so the geometry of a pattern problem plays no part."""
import numpy as np

import dense_ref as dr
import pcg_ref as pr
from pcg_ref import (LD, LD_OK, EPS, PATTERNS, QUALITY, TOL, MAXIT, BURST_DELTAS, pattern, pattern_problem,  # noqa: F401
                     row_lengths, lower_jk, next_pow2_above)

BLOCKS = (11, 16)
TRIP = 4  # FSPMV_TRIP of k_fpcg_spmv: blocks of a row whose loads are in flight together

# ---- measured constants (tests/test_freepcg_ref.py measures them again and holds them to these values) ---------------
# C_inv(c): as pcg_ref.C_INV -- the float64 transcription of the inverse kernel's loops (block_inverse) inside the
# float64 twin, one iteration on blockdiag(grade 0 and 5) over five / band43 / arrow257: the worst
# ||D (x_j - x_j*)||_inf / (kappa_2(B_j) eps ||D x_j*||_inf) is INV_RATIO[c]; C_inv = the next power of two above 4 x that.
INV_RATIO = {11: 1.432, 16: 1.381}
C_INV = {11: 8.0, 16: 8.0}
# C_gap(c): the float64 twin's own |true relative residual - recurred relative residual| over pcg_ref.QUALITY on every
# pattern of GAP_PATTERNS, in units of eps iters || |S| |x| ||_inf / ||b||_inf: the worst is GAP_RATIO[c]; C_gap the next
# power of two above 4 x that.  One constant serves both blocks: the larger of the two.
GAP_PATTERNS = ("one", "two", "three", "five", "band43", "rows", "hubs", "trip", "arrow257")
GAP_RATIO = {11: 0.540, 16: 0.312}
C_GAP = 4.0


# ---- a pattern for the product kernel's trip --------------------------------------------------------------------------

def _trip():
    """Ten leaves (cameras 0..9), then one hub per degree 2..8 (cameras 10..16) that shares with the first d leaves: the
    block rows k_fpcg_spmv walks have d + 1 = 3 .. 9 entries at the hubs -- one below, at and one above one and two trips
    of TRIP = 4 blocks (3, 4, 5 and 7, 8, 9) -- and 1 .. 8 at the leaves."""
    return [(10 + h, k) for h, d in enumerate(range(2, 9)) for k in range(d)]


PATTERNS_F = dict(PATTERNS)
PATTERNS_F["trip"] = (17, _trip())


def fpattern(name):
    n, blocks = PATTERNS_F[name]
    return n, sorted(blocks)


# ---- the stored blocks and the row walk (what psba_blockprod_plan_rows returns) --------------------------------------

def covisibility(n_cams, iidx, jidx):
    """Blocks (j, k), k <= j, with a product Y_a W_b^T: both observations of one point (a == b included)."""
    iidx, jidx = np.asarray(iidx), np.asarray(jidx)
    out = set()
    for i in np.unique(iidx):
        cams = jidx[iidx == i]
        out.update((int(j), int(k)) for j in cams for k in cams if k <= j)
    return sorted(out)


def rows_enumeration(n_cams, iidx, jidx):
    """dict(jk, added, diag_slot, rowptr, rowent): the co-visibility blocks plus the diagonal of every camera, ascending
    in (j, k); per block row the entries (slot, other | how << 28) ascending by slot -- how 0: the row's own stored
    block, 1: a block of a later row read transposed, 2: the diagonal block."""
    have = covisibility(n_cams, iidx, jidx)
    added = [j for j in range(n_cams) if (j, j) not in set(have)]
    jk = sorted(set(have) | {(j, j) for j in range(n_cams)})
    slot = {b: s for s, b in enumerate(jk)}
    rows = [[] for _ in range(n_cams)]
    for s, (j, k) in enumerate(jk):
        if j == k:
            rows[j].append((s, j | (2 << 28)))
        else:
            rows[j].append((s, k))
            rows[k].append((s, j | (1 << 28)))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    rowent = np.array([e for r in rows for e in sorted(r)], dtype=np.int32).reshape(-1, 2)
    return dict(jk=np.array(jk, dtype=np.int32), added=added, diag_slot=np.array([slot[(j, j)] for j in range(n_cams)],
                                                                               dtype=np.int32),
                rowptr=rowptr, rowent=rowent)


# ---- containers ------------------------------------------------------------------------------------------------------

def blocks_of(S, jk, c):
    jk = np.asarray(jk)
    val = np.empty((len(jk), c, c))
    for b, (j, k) in enumerate(jk):
        val[b] = S[c * j:c * j + c, c * k:c * k + c]
    return val


def dense_of(n_cams, jk, val, c):
    """The dense symmetric S of a block list; a diagonal block enters through its lower triangle."""
    S = np.zeros((c * n_cams, c * n_cams), dtype=np.asarray(val).dtype)
    for (j, k), B in zip(np.asarray(jk), val):
        if j == k:
            S[c * j:c * j + c, c * j:c * j + c] = np.tril(B) + np.tril(B, -1).T
        else:
            S[c * j:c * j + c, c * k:c * k + c] = B
            S[c * k:c * k + c, c * j:c * j + c] = B.T
    return S


def poison_upper(val, jk, c, value=np.nan):
    out = np.array(val, copy=True)
    iu = np.triu_indices(c, 1)
    for b, (j, k) in enumerate(np.asarray(jk)):
        if j == k:
            out[b][iu] = value
    return out


# ---- families (dense symmetric float64, seeded; pcg_ref's with the block size as a parameter) -------------------------

def dominant(n_cams, blocks, delta, c, grade=0.0, seed=0, negative=False):
    """pcg_ref.dominant on blocks of c.  negative: every off-diagonal entry is -|u| instead of u, so that S 1 = delta
    times the row sums -- kappa_2 grows like 1 / delta and the conjugate gradients need more iterations as delta falls
    (with mixed signs blocks of 11 and 16 converge by a factor of 8 to 10 per iteration whatever delta is)."""
    rng = np.random.default_rng([seed, n_cams, len(blocks), 11, c])
    n = c * n_cams
    S = np.zeros((n, n))
    for j, k in sorted(blocks):
        B = rng.uniform(-1.0, 1.0, (c, c))
        S[c * j:c * j + c, c * k:c * k + c] = B
        S[c * k:c * k + c, c * j:c * j + c] = B.T
    for j in range(n_cams):
        B = rng.uniform(-1.0, 1.0, (c, c))
        S[c * j:c * j + c, c * j:c * j + c] = np.tril(B, -1) + np.tril(B, -1).T
    if negative:
        S = -np.abs(S)
    S[np.arange(n), np.arange(n)] = np.abs(S).sum(axis=1) * (1.0 + delta)
    return pr._grade(S, grade, rng)


def blockdiag(n_cams, c, grade=0.0, seed=0):
    """Off-diagonal blocks exactly zero; diagonal blocks D B D, kappa_2(B) <= 100.  (S, kappa_2 of every B_j, diag D)."""
    rng = np.random.default_rng([seed, n_cams, 12, c])
    n = c * n_cams
    S = np.zeros((n, n))
    kap = np.empty(n_cams)
    for j in range(n_cams):
        Q, _ = np.linalg.qr(rng.standard_normal((c, c)))
        lam = rng.uniform(1.0, 99.0) ** (-np.arange(c) / (c - 1.0))
        B = (Q * lam[None, :]) @ Q.T
        B = np.tril(B) + np.tril(B, -1).T
        w = np.linalg.eigvalsh(B)
        kap[j] = w[-1] / w[0]
        S[c * j:c * j + c, c * j:c * j + c] = B
    S, d = pr._grade(S, grade, rng, True)
    return S, kap, d


def blockdiag_solution(S, d, b, c):
    n_cams = S.shape[0] // c
    dl = d.astype(LD)
    Bs = np.stack([S[c * j:c * j + c, c * j:c * j + c].astype(LD) / np.outer(dl[c * j:c * j + c], dl[c * j:c * j + c])
                   for j in range(n_cams)])
    M, bad = block_inverse(Bs, LD)
    assert not bad.any()
    y = np.einsum("jrc,jc->jr", M, (b.astype(LD) / dl).reshape(-1, c))
    return y / dl.reshape(-1, c)


def indefinite_pd_diag(n_cams, blocks, which, c, seed=0):
    """dominant(delta = 1) with one pair (j, k) given diagonal blocks I and the off-diagonal block 2 I: every diagonal
    block stays positive definite and v = e_j - e_k has v^T S v = -2 c / c.  Returns (S, (j, k))."""
    S = dominant(n_cams, blocks, 1.0, c, 0.0, seed)
    bl = sorted(blocks)
    j, k = bl[{"first": 0, "middle": len(bl) // 2, "last": len(bl) - 1}[which]]
    I = np.eye(c)
    S[c * j:c * j + c, c * j:c * j + c] = I
    S[c * k:c * k + c, c * k:c * k + c] = I
    S[c * j:c * j + c, c * k:c * k + c] = 2 * I
    S[c * k:c * k + c, c * j:c * j + c] = 2 * I
    return S, (j, k)


def bad_diag(n_cams, blocks, j, col, c, seed=0):
    """dominant(delta = 1) whose diagonal block j has row and column col zeroed inside the block and -1 on the diagonal
    there: the first non-positive pivot of the block's Cholesky is column col exactly."""
    S = dominant(n_cams, blocks, 1.0, c, 0.0, seed)
    B = S[c * j:c * j + c, c * j:c * j + c]
    B[col, :] = 0.0
    B[:, col] = 0.0
    B[col, col] = -1.0
    return S


def rhs(S, seed):
    return dr.rhs_for(S, seed)[0]


# ---- the kernels' arithmetic -----------------------------------------------------------------------------------------

def block_inverse(D, dtype=np.float64):
    """k_fbsr_diag_inverse's three loops for all blocks at once: D [nC, c, c] (only the lower triangles are read) ->
    (M [nC, c, c] = L^-T L^-1, bad [nC]: a pivot that is not > 0).  The sums run in the kernel's order (ascending k)."""
    a = np.asarray(D, dtype=dtype)
    nC, c = a.shape[0], a.shape[1]
    L = np.zeros((nC, c, c), dtype=dtype)
    X = np.zeros((nC, c, c), dtype=dtype)
    bad = np.zeros(nC, dtype=bool)
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        for col in range(c):
            v = a[:, col:, col].copy()                       # rows col .. c-1 of this column, every lane its own row
            for k in range(col):
                v = v - L[:, col:, k] * L[:, col, k][:, None]
            d = v[:, 0]
            bad |= ~(d > 0)
            s = np.sqrt(d)
            L[:, col, col] = s
            L[:, col + 1:, col] = v[:, 1:] * (one / s)[:, None]
        for col in range(c):
            for r in range(col, c):
                if r == col:
                    X[:, r, col] = one / L[:, r, r]
                else:
                    v = np.zeros(nC, dtype=dtype)
                    for k in range(col, r):
                        v = v - L[:, r, k] * X[:, k, col]
                    X[:, r, col] = v / L[:, r, r]
        M = np.zeros((nC, c, c), dtype=dtype)
        for r in range(c):
            for col in range(c):
                v = np.zeros(nC, dtype=dtype)
                for k in range(max(r, col), c):
                    v = v + X[:, k, r] * X[:, k, col]
                M[:, r, col] = v
    return M, bad


class BlockOp:
    """S as its symmetric list of c x c blocks in a dtype: products cost O(blocks), also in long double."""

    def __init__(self, S, n_cams, blocks, c, dtype=np.float64):
        self.n_cams, self.c, self.dtype = n_cams, c, dtype
        rows, cols, B = [], [], []
        for j in range(n_cams):
            rows.append(j), cols.append(j), B.append(S[c * j:c * j + c, c * j:c * j + c])
        for j, k in blocks:
            rows.append(j), cols.append(k), B.append(S[c * j:c * j + c, c * k:c * k + c])
            rows.append(k), cols.append(j), B.append(S[c * k:c * k + c, c * j:c * j + c])
        self.rows, self.cols = np.array(rows), np.array(cols)
        self.B = np.array(B).astype(dtype)
        self.diag = self.B[:n_cams]

    def times(self, x):
        prod = np.einsum("erc,ec->er", self.B, x.reshape(-1, self.c)[self.cols])
        y = np.zeros((self.n_cams, self.c), dtype=self.dtype)
        np.add.at(y, self.rows, prod)
        return y.reshape(-1)


def twin_pcg(S, n_cams, blocks, b, tol, max_iter, c, dtype=np.float64, keep_iterates=False):
    """pcg_ref.twin_pcg on blocks of c: the recurrences and the stop rule of kernels_free_pcg.hip (those of
    kernels_pcg.hip).  Returns the same dict."""
    op = BlockOp(S, n_cams, blocks, c, dtype)
    M, bad = block_inverse(op.diag, dtype)
    prec = lambda v: np.einsum("jrc,jc->jr", M, v.reshape(-1, c)).reshape(-1)  # noqa: E731
    b = np.asarray(b).astype(dtype)
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rz, bb = r @ z, b @ b
    out = dict(hist=[1.0], iterates=[], converged=False, failed=bool(bad.any()), exhausted=False)
    tol2 = dtype(tol) * dtype(tol)
    rr = None
    it = 0
    with np.errstate(all="ignore"):
        while not out["failed"]:
            if rz == 0 or (it > 0 and rr <= tol2 * bb):
                out["converged"] = True
                break
            if it == max_iter:
                break
            q = op.times(p)
            pq = p @ q
            if not pq > 0:
                out["failed"] = True
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            z = prec(r)
            rr, rzn = r @ r, r @ z
            p = z + (rzn / rz) * p
            rz = rzn
            it += 1
            out["hist"].append(float(np.sqrt(rr / bb)) if bb > 0 else 0.0)
            if keep_iterates:
                out["iterates"].append(x.astype(np.float64))
    out["exhausted"] = not out["converged"] and not out["failed"]
    out["iters"] = it
    out["x"] = x.astype(np.float64)
    out["relres"] = out["hist"][-1] if it > 0 else (0.0 if not bb > 0 or rz == 0 else 1.0)
    return out


# ---- bounds ----------------------------------------------------------------------------------------------------------

def entry_row_lengths(n_cams, blocks, c):
    return np.repeat(row_lengths(n_cams, blocks), c)


def spmv_exact(S, x):
    return S.astype(LD) @ np.asarray(x).astype(LD)


def spmv_bound(S, x, m, c):
    """A row with m block entries sums c m products in some order: |y_r - exact| <= c m eps sum_c |S_rc| |x_c|."""
    return float(c) * m * EPS * (np.abs(S) @ np.abs(x))


def true_relres(S, x, b):
    return float(np.linalg.norm(dr.residual(S, x, b)) / np.linalg.norm(b))


def gap_unit(S, x, b, iters):
    return EPS * max(iters, 1) * float((np.abs(S) @ np.abs(x)).max() / np.abs(b).max())


def product_vectors(n_cams, c, seed=0):
    n = c * n_cams
    rng = np.random.default_rng([seed, n, 13])
    out = [("ones", np.ones(n)), ("signs 1e+-8", rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 8, n))]
    for r in (0, c // 2, c - 1):
        e = np.zeros(n)
        e[n - c + r] = 1.0
        out.append((f"unit {r} of the last camera", e))
    return out


# ---- cached cases ----------------------------------------------------------------------------------------------------
_CACHE = {}


def blockdiag_case(name, grade, c, seed=3):
    key = ("blockdiag", name, grade, c, seed)
    if key not in _CACHE:
        n_cams, blocks = fpattern(name)
        S, kap, d = blockdiag(n_cams, c, grade, seed)
        b = rhs(S, seed + 1)
        _CACHE[key] = dict(n_cams=n_cams, blocks=blocks, S=S, kap=kap, d=d, b=b, xs=blockdiag_solution(S, d, b, c), c=c)
    return _CACHE[key]


def blockdiag_ratios(case, x):
    """Per camera ||D (x_j - x_j*)||_inf / (kappa_2(B_j) eps ||D x_j*||_inf)."""
    n, c = case["n_cams"], case["c"]
    D = case["d"].reshape(n, c).astype(LD)
    err = np.abs(D * (np.asarray(x).reshape(n, c).astype(LD) - case["xs"])).max(axis=1)
    return (err / (case["kap"] * EPS * np.abs(D * case["xs"]).max(axis=1))).astype(np.float64)


def quality_system(name, delta, grade, c, seed=0):
    """A dominant system on a named pattern, its right-hand side and the float64 twin's run at (TOL, MAXIT)."""
    key = ("quality", name, delta, grade, c, seed)
    if key not in _CACHE:
        n_cams, blocks = fpattern(name)
        S = dominant(n_cams, blocks, delta, c, grade, seed)
        b = rhs(S, seed + 1)
        _CACHE[key] = dict(name=name, n_cams=n_cams, blocks=blocks, S=S, b=b, c=c,
                           t64=twin_pcg(S, n_cams, blocks, b, TOL, MAXIT, c))
    return _CACHE[key]


BURST_EDGES = (7, 8, 9, 16, 17)


def burst_case(name, k, c):
    """pcg_ref.burst_case on blocks of c: a dominant(negative=True) system whose long-double twin's relative residual drops by >= 4x from
    iteration k - 1 to k (and is still >= 1e-14 there); tol = their geometric mean makes the solve stop after exactly k
    iterations, and rounding cannot move the stop.  The first delta of BURST_DELTAS that qualifies, or None."""
    key = ("burst", name, k, c)
    if key not in _CACHE:
        n_cams, blocks = fpattern(name)
        found = None
        for delta in BURST_DELTAS:
            S = dominant(n_cams, blocks, delta, c, 0.0, 7, negative=True)
            b = rhs(S, 8)
            h = twin_pcg(S, n_cams, blocks, b, 0.0, k, c, LD)["hist"]
            if len(h) > k and h[k] >= 1e-14 and h[k - 1] >= 4.0 * h[k] and min(h[:k]) > np.sqrt(h[k - 1] * h[k]):
                found = dict(delta=delta, tol=float(np.sqrt(h[k - 1] * h[k])), S=S, b=b, n_cams=n_cams, blocks=blocks,
                             hist=h)
                break
        _CACHE[key] = found
    return _CACHE[key]


# ---- a handle's block list as an operator (any size: no dense matrix) -------------------------------------------------

class ListOp:
    """The symmetric S of a block list (jk [nb, 2], val [nb, c, c]; a diagonal block through its lower triangle) in a
    dtype, and |S|: products cost O(blocks), so the 2050-camera scene is judged like the small ones."""

    def __init__(self, n_cams, jk, val, c, dtype=LD):
        jk, val = np.asarray(jk), np.asarray(val)
        self.n_cams, self.c, self.dtype = n_cams, c, dtype
        dg = jk[:, 0] == jk[:, 1]
        D = np.tril(val[dg]) + np.transpose(np.tril(val[dg], -1), (0, 2, 1))
        off = val[~dg]
        self.rows = np.concatenate([jk[dg, 0], jk[~dg, 0], jk[~dg, 1]])
        self.cols = np.concatenate([jk[dg, 1], jk[~dg, 1], jk[~dg, 0]])
        self.B = np.concatenate([D, off, np.transpose(off, (0, 2, 1))]).astype(dtype)

    def _times(self, B, x):
        prod = np.einsum("erc,ec->er", B, np.asarray(x).astype(self.dtype).reshape(-1, self.c)[self.cols])
        y = np.zeros((self.n_cams, self.c), dtype=self.dtype)
        np.add.at(y, self.rows, prod)
        return y.reshape(-1)

    def times(self, x):
        return self._times(self.B, x)

    def abs_times(self, x):
        return self._times(np.abs(self.B), np.abs(x))


def list_relres_and_gap(op, x, b, iters):
    """(||b - S x||_2 / ||b||_2 in the operator's dtype, gap_unit = eps iters || |S| |x| ||_inf / ||b||_inf)"""
    b = np.asarray(b)
    r = b.astype(op.dtype) - op.times(x)
    tr = float(np.sqrt(r @ r) / np.sqrt(b.astype(op.dtype) @ b.astype(op.dtype)))
    return tr, EPS * max(iters, 1) * float(op.abs_times(x).max() / np.abs(b).max())


def band_scene(n_cams, seed=17):
    """n_cams ring cameras, 2 n_cams points, each seen by 3 to 5 consecutive cameras (the first of them drawn uniformly):
    about 8 points per camera, a block band of half-width 4 -- freekd_twin._scene on that visibility table."""
    from freekd_twin import _scene
    rng = np.random.default_rng([seed, n_cams])
    n_pts = 2 * n_cams
    pts = rng.uniform(-1.0, 1.0, (n_pts, 3))
    keep = np.zeros((n_pts, n_cams), dtype=bool)
    first = rng.integers(0, n_cams - 4, n_pts)
    first[:n_cams - 4] = np.arange(n_cams - 4)     # every run of cameras starts at least one point: no camera is unseen
    for i, (f, k) in enumerate(zip(first, rng.integers(3, 6, n_pts))):
        keep[i, f:f + k] = True
    return _scene(rng, n_cams, pts, keep)
