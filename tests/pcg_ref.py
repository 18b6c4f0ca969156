"""Host reference for the block-sparse route (psba_set_solver PSBA_SOLVER_PCG, kernels_pcg.hip; no GPU): problems
whose lower block pattern is a chosen one, seeded matrix families on such a pattern, a twin of the kernels'
block-Jacobi conjugate gradients in float64 and long double, and the rounding bounds the GPU tests hold the kernels to.

Every matrix goes into a handle through psba_set_sparse_S, so the geometry of a pattern problem plays no part: it only
has to make psba_upload_problem produce the blocks.  A matrix lives here as the dense symmetric S [6 nC, 6 nC]
(n <= 1560 everywhere); blocks_of() cuts it into a handle's block list and dense_of() puts a block list back, a
diagonal block through its lower triangle -- the only half the kernels read.

Extended precision is np.longdouble where its epsilon is at most 1.1e-19 (LD_OK, as dense_ref / assembly_ref); the
tests that need it skip elsewhere.  dense_ref supplies the extended residual, the refined solution and the forward
error."""
import numpy as np

import dense_ref as dr

LD = np.longdouble
LD_OK = dr.LD_OK
EPS = dr.EPS

# ---- measured constants (tests/test_pcg_ref.py measures them again and holds them to these values) -----------------
# C_inv: the numpy float64 transcription of k_bsr_diag_inverse's three loops (block_inverse) inside the float64 twin,
# one iteration on blockdiag(grade 5) over five / band43 / arrow257: the worst
# ||x_j - x_j*||_inf / (kappa_2(B_j) eps ||x_j*||_inf) is INV_RATIO; C_inv = the next power of two above 4 x that
# (x 4: room for another multiply-add contraction than numpy's).  The norm is the graded one, ||D (x_j - x_j*)||_inf
# against ||D x_j*||_inf: that is where a Cholesky solve is invariant under the grading D B D (at grade 0 it is the plain
# norm).  In the plain norm the error of a graded block is not bounded by kappa_2(B_j) at all -- with b = S x* the
# float64 transcription itself is off by up to 3e8 kappa eps at grade 5 -- so no constant measured there would judge
# anything.
INV_RATIO = 1.09
C_INV = 8.0
# C_gap: the float64 twin's own |true relative residual - recurred relative residual| over the systems of the GPU
# module's solve-quality sweep, in units of eps iters || |S| |x| ||_inf / ||b||_inf: the worst is GAP_RATIO; C_gap the
# next power of two above 4 x that.
GAP_RATIO = 0.456
C_GAP = 2.0


# ---- patterns --------------------------------------------------------------------------------------------------------

def _full(n):
    return [(j, k) for j in range(n) for k in range(j)]


def _band(n, w):
    return [(j, k) for j in range(n) for k in range(max(0, j - w), j)]


def _rows(n=40, period=20):
    return [(j, k) for j in range(n) for k in range(j - j % period, j)]


def _arrow(n):
    return sorted(set([(j, 0) for j in range(1, n)] + [(j, j - 1) for j in range(1, n)]))


HUB_DEGREES = (6, 7, 8, 15, 16)


def _hubs():
    """16 leaves (cameras 0..15), one camera with no neighbour (16), five hubs (17..21) that share with the first
    6, 7, 8, 15, 16 leaves: the block rows the product kernel walks have 7, 8, 9, 16 and 17 entries at the hubs, 1 at
    camera 16 and 2..6 at the leaves -- both sides of its stride of eight and of sixteen."""
    return [(17 + h, k) for h, d in enumerate(HUB_DEGREES) for k in range(d)]


# name -> (cameras, off-diagonal blocks (j, k) with k < j).  `rows`: camera j shares with its j % 20 predecessors, so
# the STORED lower row of camera j has 1..20 blocks; the rows of the symmetric pattern, which k_pcg_spmv walks, all have
# 20 (two cliques of 20).  `hubs` is the pattern whose walked rows have the lengths 1, 7, 8, 9, 16, 17.
PATTERNS = {
    "one": (1, _full(1)),
    "two": (2, _full(2)),
    "three": (3, _full(3)),
    "five": (5, _full(5)),
    "band43": (43, _band(43, 3)),
    "rows": (40, _rows()),
    "hubs": (22, _hubs()),
    "arrow257": (257, _arrow(257)),
    "arrow260": (260, _arrow(260)),
}
SMALL = ("one", "two", "three", "five", "rows", "hubs")  # nA <= 256: one workgroup owns every sum of the solve


def pattern(name):
    n, blocks = PATTERNS[name]
    return n, sorted(blocks)


def row_lengths(n_cams, blocks):
    """Entries per block row of the full symmetric pattern (the diagonal block included)."""
    m = np.ones(n_cams, dtype=np.int64)
    for j, k in blocks:
        m[j] += 1
        m[k] += 1
    return m


def stored_row_lengths(n_cams, blocks):
    m = np.ones(n_cams, dtype=np.int64)
    for j, _ in blocks:
        m[j] += 1
    return m


def pattern_flags(n_cams, blocks):
    """What psba_sparse_pattern must say: one byte per block tri(j) + k of the lower block triangle."""
    f = np.zeros(n_cams * (n_cams + 1) // 2, dtype=np.uint8)
    for j in range(n_cams):
        f[j * (j + 1) // 2 + j] = 1
    for j, k in blocks:
        f[j * (j + 1) // 2 + k] = 1
    return f


def pattern_problem(n_cams, blocks):
    """A valid capi.Problem whose lower block pattern is exactly `blocks` plus the diagonal: one point per block
    (j, k), seen by cameras k and j; a camera without any block gets three points of its own (its diagonal block).  Cameras
    and K from synth.make_problem, observations = projections of the points."""
    import psba_amd.synth as synth
    from psba_amd.capi import Problem
    base = synth.make_problem(n_cams=max(n_cams, 2), n_pts=8, mean_track=2.0, seed=1000 + n_cams)
    K, q, cams = base["K"][:n_cams], base["initrot"][:n_cams], base["cams"][:n_cams]
    seen = np.zeros(n_cams, dtype=bool)
    tracks = []
    for j, k in sorted(blocks):
        assert 0 <= k < j < n_cams
        tracks.append((k, j))
        seen[j] = seen[k] = True
    tracks += [(j,) for j in np.flatnonzero(~seen) for _ in range(3)]
    rng = np.random.default_rng([n_cams, len(tracks), 5])
    M = rng.normal(size=(len(tracks), 3))
    M *= (0.9 * rng.random(len(tracks)) ** (1 / 3) / np.linalg.norm(M, axis=1))[:, None]
    iidx = np.array([i for i, t in enumerate(tracks) for _ in t], dtype=np.int32)
    jidx = np.array([c for t in tracks for c in t], dtype=np.int32)
    xy, depth = synth.project(K[jidx], q[jidx], cams[jidx], M[iidx])
    assert np.all(depth > 0)
    pts0 = M + rng.normal(0, 1e-2, M.shape)
    return Problem(K=K.copy(), initrot=q.copy(), cams=cams.copy(), pts=pts0, impts=xy + rng.normal(0, 1.0, xy.shape),
                   iidx=iidx, jidx=jidx, nC=n_cams, nP=len(tracks), nO=int(iidx.size))


# ---- containers ------------------------------------------------------------------------------------------------------

def blocks_of(S, jk):
    """val [nb, 6, 6] of a handle's block list jk [nb, 2] = (j, k), k <= j, cut out of the dense S (copies: a diagonal
    block comes with both triangles)."""
    jk = np.asarray(jk)
    val = np.empty((len(jk), 6, 6))
    for b, (j, k) in enumerate(jk):
        val[b] = S[6 * j:6 * j + 6, 6 * k:6 * k + 6]
    return val


def dense_of(n_cams, jk, val):
    """The dense symmetric S of a block list; a diagonal block enters through its lower triangle."""
    S = np.zeros((6 * n_cams, 6 * n_cams), dtype=np.asarray(val).dtype)
    for (j, k), B in zip(np.asarray(jk), val):
        if j == k:
            S[6 * j:6 * j + 6, 6 * j:6 * j + 6] = np.tril(B) + np.tril(B, -1).T
        else:
            S[6 * j:6 * j + 6, 6 * k:6 * k + 6] = B
            S[6 * k:6 * k + 6, 6 * j:6 * j + 6] = B.T
    return S


def poison_upper(val, jk, value=np.nan):
    """A copy of val with the strict upper triangle of every diagonal block overwritten."""
    out = np.array(val, copy=True)
    iu = np.triu_indices(6, 1)
    for b, (j, k) in enumerate(np.asarray(jk)):
        if j == k:
            out[b][iu] = value
    return out


def lower_jk(n_cams, blocks):
    """A block list in a canonical order (row by row, the diagonal block last in its row) for host-only use."""
    per = {j: [] for j in range(n_cams)}
    for j, k in sorted(blocks):
        per[j].append(k)
    return np.array([(j, k) for j in range(n_cams) for k in per[j] + [j]], dtype=np.int32)


# ---- families (dense symmetric float64, seeded) ---------------------------------------------------------------------

def _grade(S, grade, rng, want_d=False):
    d = np.ones(S.shape[0])
    if grade:
        d = 10.0 ** rng.uniform(-grade, grade, size=S.shape[0])
        S = d[:, None] * S * d[None, :]
        dr.symmetrize_from_lower(S)
    return (S, d) if want_d else S


def dominant(n_cams, blocks, delta, grade=0.0, seed=0):
    """Random blocks on the pattern (off-diagonal blocks non-symmetric), diagonal entries = the row's absolute sum times
    (1 + delta): positive definite by Gershgorin; then D S D with D = 10^uniform(+-grade)."""
    rng = np.random.default_rng([seed, n_cams, len(blocks), 11])
    n = 6 * n_cams
    S = np.zeros((n, n))
    for j, k in sorted(blocks):
        B = rng.uniform(-1.0, 1.0, (6, 6))
        S[6 * j:6 * j + 6, 6 * k:6 * k + 6] = B
        S[6 * k:6 * k + 6, 6 * j:6 * j + 6] = B.T
    for j in range(n_cams):
        B = rng.uniform(-1.0, 1.0, (6, 6))
        S[6 * j:6 * j + 6, 6 * j:6 * j + 6] = np.tril(B, -1) + np.tril(B, -1).T
    S[np.arange(n), np.arange(n)] = np.abs(S).sum(axis=1) * (1.0 + delta)
    return _grade(S, grade, rng)


def blockdiag(n_cams, grade=0.0, seed=0):
    """Off-diagonal blocks exactly zero; diagonal blocks D B D, B = Q diag(lambda) Q^T with kappa_2(B) <= 100.
    Returns (S, kappa_2 of every ungraded B_j, the diagonal of D)."""
    rng = np.random.default_rng([seed, n_cams, 12])
    n = 6 * n_cams
    S = np.zeros((n, n))
    kap = np.empty(n_cams)
    for j in range(n_cams):
        Q, R = np.linalg.qr(rng.standard_normal((6, 6)))
        lam = rng.uniform(1.0, 99.0) ** (-np.arange(6) / 5.0)
        B = (Q * lam[None, :]) @ Q.T
        B = np.tril(B) + np.tril(B, -1).T
        w = np.linalg.eigvalsh(B)
        kap[j] = w[-1] / w[0]
        S[6 * j:6 * j + 6, 6 * j:6 * j + 6] = B
    S, d = _grade(S, grade, rng, True)
    return S, kap, d


def blockdiag_solution(S, d, b):
    """The long-double solution of a blockdiag system, block by block on the ungraded form: B' = D^-1 S_j D^-1 (what the
    rounded grading left of B_j, kappa_2 <= 100), y = B'^-1 D^-1 b_j by a long-double Cholesky, x_j = D^-1 y."""
    n_cams = S.shape[0] // 6
    dl = d.astype(LD)
    Bs = np.stack([S[6 * j:6 * j + 6, 6 * j:6 * j + 6].astype(LD) / np.outer(dl[6 * j:6 * j + 6], dl[6 * j:6 * j + 6])
                   for j in range(n_cams)])
    M, bad = block_inverse(Bs, LD)
    assert not bad.any()
    y = np.einsum("jrc,jc->jr", M, (b.astype(LD) / dl).reshape(-1, 6))
    return y / dl.reshape(-1, 6)


def indefinite_pd_diag(n_cams, blocks, which, seed=0):
    """dominant(delta = 1) with one pair of cameras (j, k) -- the first, middle or last stored off-diagonal block --
    given diagonal blocks I and the off-diagonal block 2 I: every diagonal block stays positive definite and
    v = e_j - e_k has v^T S v = -2.  Returns (S, (j, k))."""
    S = dominant(n_cams, blocks, 1.0, 0.0, seed)
    bl = sorted(blocks)
    j, k = bl[{"first": 0, "middle": len(bl) // 2, "last": len(bl) - 1}[which]]
    I = np.eye(6)
    S[6 * j:6 * j + 6, 6 * j:6 * j + 6] = I
    S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = I
    S[6 * j:6 * j + 6, 6 * k:6 * k + 6] = 2 * I
    S[6 * k:6 * k + 6, 6 * j:6 * j + 6] = 2 * I
    return S, (j, k)


def bad_diag(n_cams, blocks, j, c, seed=0):
    """dominant(delta = 1) whose diagonal block j has row and column c zeroed (inside the block) and -1 on the
    diagonal there: its leading c x c part stays positive definite and eliminating the columns < c never touches row c,
    so the first non-positive pivot of the block's Cholesky is column c exactly."""
    S = dominant(n_cams, blocks, 1.0, 0.0, seed)
    B = S[6 * j:6 * j + 6, 6 * j:6 * j + 6]
    B[c, :] = 0.0
    B[:, c] = 0.0
    B[c, c] = -1.0
    return S


def plant_margin(S, row):
    """A copy of S whose Gershgorin margin is smallest, and negative, in `row`: its diagonal entry becomes half the
    row's off-diagonal absolute sum."""
    S = np.array(S, copy=True)
    off = np.abs(S[row]).sum() - abs(S[row, row])
    S[row, row] = 0.5 * off
    return S


def rhs(S, seed):
    """b = S x* for a seeded x* in extended precision, rounded once (dense_ref.rhs_for)."""
    return dr.rhs_for(S, seed)[0]


# ---- the kernels' arithmetic -----------------------------------------------------------------------------------------

def block_inverse(D, dtype=np.float64):
    """k_bsr_diag_inverse's three loops for all blocks at once: D [nC, 6, 6] (only the lower triangles are read) ->
    (M [nC, 6, 6] = L^-T L^-1, bad [nC]: a pivot that is not > 0).  The sums run in the kernel's order."""
    a = np.asarray(D, dtype=dtype)
    nC = a.shape[0]
    L = np.zeros((nC, 6, 6), dtype=dtype)
    X = np.zeros((nC, 6, 6), dtype=dtype)
    bad = np.zeros(nC, dtype=bool)
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        for c in range(6):
            d = a[:, c, c].copy()
            for k in range(c):
                d = d - L[:, c, k] * L[:, c, k]
            bad |= ~(d > 0)
            s = np.sqrt(d)
            inv = one / s
            L[:, c, c] = s
            for r in range(c + 1, 6):
                v = a[:, r, c].copy()
                for k in range(c):
                    v = v - L[:, r, k] * L[:, c, k]
                L[:, r, c] = v * inv
        for c in range(6):
            for r in range(c, 6):
                if r == c:
                    X[:, r, c] = one / L[:, r, r]
                else:
                    v = np.zeros(nC, dtype=dtype)
                    for k in range(c, r):
                        v = v - L[:, r, k] * X[:, k, c]
                    X[:, r, c] = v / L[:, r, r]
        M = np.zeros((nC, 6, 6), dtype=dtype)
        for r in range(6):
            for c in range(6):
                v = np.zeros(nC, dtype=dtype)
                for k in range(max(r, c), 6):
                    v = v + X[:, k, r] * X[:, k, c]
                M[:, r, c] = v
    return M, bad


class BlockOp:
    """S as its symmetric list of 6x6 blocks in a dtype: products cost O(blocks), also in long double."""

    def __init__(self, S, n_cams, blocks, dtype=np.float64):
        self.n_cams, self.dtype = n_cams, dtype
        rows, cols, B = [], [], []
        for j in range(n_cams):
            rows.append(j), cols.append(j), B.append(S[6 * j:6 * j + 6, 6 * j:6 * j + 6])
        for j, k in blocks:
            rows.append(j), cols.append(k), B.append(S[6 * j:6 * j + 6, 6 * k:6 * k + 6])
            rows.append(k), cols.append(j), B.append(S[6 * k:6 * k + 6, 6 * j:6 * j + 6])
        self.rows, self.cols = np.array(rows), np.array(cols)
        self.B = np.array(B).astype(dtype)
        self.diag = self.B[:n_cams]

    def times(self, x):
        prod = np.einsum("erc,ec->er", self.B, x.reshape(-1, 6)[self.cols])
        y = np.zeros((self.n_cams, 6), dtype=self.dtype)
        np.add.at(y, self.rows, prod)
        return y.reshape(-1)


def twin_pcg(S, n_cams, blocks, b, tol, max_iter, dtype=np.float64, keep_iterates=False):
    """Block-Jacobi PCG with the recurrences and the stop rule of kernels_pcg.hip: r.r <= tol^2 b.b is tested before an
    iteration on the previous iteration's r.r (and once more after the last one of the budget), r.z == 0 counts as
    converged, p.Sp that is not > 0 or a diagonal block without a Cholesky factor is a failure.  Returns a dict:
    x, hist (relative residual after every iteration carried out; hist[0] = 1 is the start), iters as psba_pcg_info
    counts them, converged / failed / exhausted, iterates (if asked)."""
    op = BlockOp(S, n_cams, blocks, dtype)
    M, bad = block_inverse(op.diag, dtype)
    prec = lambda v: np.einsum("jrc,jc->jr", M, v.reshape(-1, 6)).reshape(-1)  # noqa: E731
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

def entry_row_lengths(n_cams, blocks):
    """Block entries m of the block row of every unknown [6 nC]."""
    return np.repeat(row_lengths(n_cams, blocks), 6)


def spmv_exact(S, x):
    """S x in long double (not rounded)."""
    return S.astype(LD) @ np.asarray(x).astype(LD)


def spmv_bound(S, x, m):
    """A row with m block entries sums 6 m products in some order: |y_r - exact| <= 6 m eps sum_c |S_rc| |x_c|
    (first-order constant 6 m u with u = eps / 2, doubled: any order, fused multiply-adds or not)."""
    return 6.0 * m * EPS * (np.abs(S) @ np.abs(x))


def gershgorin_exact(S, m):
    """(margins d_r = S_rr - sum_{c != r} |S_rc| in long double, bound 6 m eps sum_c |S_rc| per row)."""
    A = np.abs(S).astype(LD)
    dg = np.diag(S).astype(LD)
    tot = A.sum(axis=1)
    return dg - (tot - np.abs(dg)), 6.0 * m * EPS * tot.astype(np.float64)


def true_relres(S, x, b):
    """||b - S x||_2 / ||b||_2 with the residual in extended precision."""
    return float(np.linalg.norm(dr.residual(S, x, b)) / np.linalg.norm(b))


def gap_unit(S, x, b, iters):
    """eps iters || |S| |x| ||_inf / ||b||_inf: the unit of the gap between a recurred and a true relative residual."""
    return EPS * max(iters, 1) * float((np.abs(S) @ np.abs(x)).max() / np.abs(b).max())


def cond2_or_inf(S):
    """kappa_2 of S where float64 eigenvalues can tell it (below 1e15), inf beyond: a bound that carries such a kappa
    says nothing, as it should."""
    w = np.linalg.eigvalsh(S)
    return float(w[-1] / w[0]) if w[0] > 0 and w[-1] < 1e15 * w[0] else float("inf")


def precond_cond(S, n_cams):
    """kappa_2 of the block-Jacobi preconditioned system L^-1 S L^-T (L: Cholesky factors of the diagonal blocks)."""
    Li = np.zeros_like(S)
    for j in range(n_cams):
        s = slice(6 * j, 6 * j + 6)
        Li[s, s] = np.linalg.inv(np.linalg.cholesky(S[s, s]))
    return dr.cond2(Li @ S @ Li.T)


# ---- the systems the GPU module solves (cached: both test modules and every test of one share them) ------------------

QUALITY = [(1.0, 0.0), (1e-2, 0.0), (1e-2, 4.0), (1e-4, 2.0)]  # (delta, grade) of the solve-quality sweep
TOL, MAXIT = 1e-10, 4000
_SYS = {}


def system(name, delta, grade, seed=0):
    """A dominant system on a named pattern with everything the checks need: S, b, kappa_2(S), the refined solution,
    and the float64 / long-double twins' runs at (TOL, MAXIT)."""
    key = (name, delta, grade, seed)
    if key not in _SYS:
        n_cams, blocks = pattern(name)
        S = dominant(n_cams, blocks, delta, grade, seed)
        b = rhs(S, seed + 1)
        t64 = twin_pcg(S, n_cams, blocks, b, TOL, MAXIT, np.float64)
        t80 = twin_pcg(S, n_cams, blocks, b, TOL, MAXIT, LD) if LD_OK else None
        _SYS[key] = dict(name=name, n_cams=n_cams, blocks=blocks, S=S, b=b, kappa=cond2_or_inf(S),
                         ref=dr.refined_solution(S, b), t64=t64, t80=t80)
    return _SYS[key]


BURST_EDGES = (1, 7, 8, 9, 16, 17)
BURST_DELTAS = tuple(2.0 ** (-e / 4.0) for e in range(-12, 41))  # 8 ... 2^-10, the search grid for a 4x step
_BURST = {}


def burst_reference(case):
    """kappa_2(S) and the refined solution of a burst case's system (shared by the cases of one delta)."""
    key = ("burst", case["n_cams"], len(case["blocks"]), case["delta"])
    if key not in _SYS:
        _SYS[key] = (dr.cond2(case["S"]), dr.refined_solution(case["S"], case["b"]))
    return _SYS[key]


def burst_case(name, k):
    """A dominant system on the pattern whose long-double twin's relative residual drops by >= 4x from iteration k - 1
    to k (and is still >= 1e-14 there: with kappa <= 100 a float64 recurrence gets there, and the test's bound on x carries
    1e-14 beside tol): tol = their geometric mean makes the
    solve stop after exactly k iterations, and rounding cannot move the stop.  The first delta of BURST_DELTAS that
    qualifies.  Returns dict(delta, tol, S, b, n_cams, blocks, hist) or None."""
    key = (name, k)
    if key not in _BURST:
        n_cams, blocks = pattern(name)
        found = None
        for delta in BURST_DELTAS:
            S = dominant(n_cams, blocks, delta, 0.0, 7)
            b = rhs(S, 8)
            h = twin_pcg(S, n_cams, blocks, b, 0.0, k, LD)["hist"]
            if len(h) > k and h[k] >= 1e-14 and h[k - 1] >= 4.0 * h[k] and min(h[:k]) > np.sqrt(h[k - 1] * h[k]):
                found = dict(delta=delta, tol=float(np.sqrt(h[k - 1] * h[k])), S=S, b=b, n_cams=n_cams, blocks=blocks,
                             hist=h)
                break
        _BURST[key] = found
    return _BURST[key]


def next_pow2_above(v):
    return float(2.0 ** np.ceil(np.log2(v)))


def product_vectors(n_cams, seed=0):
    """The x of the product test: ones; random signs with magnitudes 10^uniform(-8, 8); one unit vector per lane 0..5 of
    the last camera."""
    n = 6 * n_cams
    rng = np.random.default_rng([seed, n, 13])
    out = [("ones", np.ones(n)), ("signs 1e+-8", rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 8, n))]
    for r in range(6):
        e = np.zeros(n)
        e[n - 6 + r] = 1.0
        out.append((f"unit {r} of the last camera", e))
    return out


def blockdiag_case(name, grade, seed=3):
    """blockdiag on a named pattern with its right-hand side and the long-double block solves."""
    key = ("blockdiag", name, grade, seed)
    if key not in _SYS:
        n_cams, blocks = pattern(name)
        S, kap, d = blockdiag(n_cams, grade, seed)
        b = rhs(S, seed + 1)
        _SYS[key] = dict(n_cams=n_cams, blocks=blocks, S=S, kap=kap, d=d, b=b, xs=blockdiag_solution(S, d, b))
    return _SYS[key]


def blockdiag_ratios(case, x):
    """Per camera ||D (x_j - x_j*)||_inf / (kappa_2(B_j) eps ||D x_j*||_inf)."""
    n = case["n_cams"]
    D = case["d"].reshape(n, 6).astype(LD)
    err = np.abs(D * (np.asarray(x).reshape(n, 6).astype(LD) - case["xs"])).max(axis=1)
    return (err / (case["kap"] * EPS * np.abs(D * case["xs"]).max(axis=1))).astype(np.float64)


def judge_solve(sy, rc, x, iters, relres, what=""):
    """The solve-quality checks on one solution of a system(): rc OK, finite x, reported relres <= TOL, the true relative
    residual within gap = C_GAP eps iters || |S| |x| ||_inf / ||b||_inf of the reported one, the forward error within
    2 kappa_2(S) (TOL + gap), and no more iterations than the float64 twin's + 1 + 2 |count64 - count80|.  Returns the
    ratios (gap used / allowed, forward error / allowed, iterations - twin's)."""
    tag = f"{sy['name']} {what}"
    assert rc == 0, f"{tag}: rc {rc}"
    assert np.all(np.isfinite(x)), f"{tag}: non-finite x"
    assert relres <= TOL, f"{tag}: reported relres {relres:.3e}"
    gap = C_GAP * gap_unit(sy["S"], x, sy["b"], iters)
    tr = true_relres(sy["S"], x, sy["b"])
    assert abs(tr - relres) <= gap, f"{tag}: true relres {tr:.6e}, reported {relres:.6e}, gap allowed {gap:.3e}"
    fe = dr.forward_error(x, sy["ref"])
    fe_max = 2.0 * sy["kappa"] * (TOL + gap)
    assert fe <= fe_max, f"{tag}: forward error {fe:.3e} > {fe_max:.3e} (kappa {sy['kappa']:.2e})"
    n64 = sy["t64"]["iters"]
    n80 = sy["t80"]["iters"] if sy["t80"] is not None else n64
    assert iters <= n64 + 1 + 2 * abs(n64 - n80), f"{tag}: {iters} iterations, the float64 twin {n64}, long double {n80}"
    return dict(gap=abs(tr - relres) / gap, fwd=fe / fe_max, iters=iters - n64)
