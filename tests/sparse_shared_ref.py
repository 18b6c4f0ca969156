"""Host reference of intrinsics shared between cameras under the block-sparse solver
(psba_set_sparse_intrinsics_groups; kernels_free_pcg.hip; no GPU): tests/test_sparse_shared_ref.py applies it
to a float64 transcription and to injected faults, tests/test_gpu_sparse_shared.py to the kernels.

Model (shared_ref.py's, restated for a list of blocks).  The list keeps S0, the unfolded blocks WITHOUT damping.  With
phi the map of shared_ref.fold_map (a shared coordinate of a member goes to its representative's, every other one to
itself) and "away" its folded-away coordinates, the solve works on the embedded

    A = P^T S0 P + mu D   on the kept coordinates,        (P x)[t] = x[phi[t]],   (P^T q)[r] = sum over phi[t] = r of q[t]
    A[t][t] = coeff + mu D[t], zero elsewhere              at a folded-away coordinate t,

with mu added once, after the sum; e_a = P^T e_a on the kept coordinates and 0 at the folded-away ones.  Per-camera
masks enter through `free` [nC, 10] (rows equal inside a group); a global mask is the same row for every camera.

FoldedOp forms A x from the list in O(blocks): expand, the block product (freepcg_ref.ListOp), the sum over the members in
ascending camera order, then + mu D x -- the three steps of the kernels in their order (k_fpcg_spmv's order inside a block
row is the walk's; ListOp's is numpy's, and the bound below does not depend on it).

The bound of the fold product.  Row r of A x is one sum, in a fixed order, of
    m_r = sum over the members t with phi[t] = r of (c len(row of t's camera))   products S0[t][u] (P x)[u], each rounded,
          + the additions across the members (one per member)
          + 2 for mu D x (its product and its addition)
terms, so |found - exact| <= gamma(m_r) sum |terms| with the terms |S0| |P x| summed over the members and |mu D x|
(Higham, Accuracy and Stability, 3.1: any order of summation; the products' roundings take one factor each, which
gamma(m) with m counting products AND additions covers).  Derived, not fitted.  At a folded-away coordinate the kernels
form fl(fl(coeff + fl(mu D)) x): three roundings at most, and the test holds it to the bit.

The folded diagonal blocks (folded_blocks) are those of A: entry ((r, a), (r, b)) of P^T S0 P for the coordinates of
one camera.  The kernels build the block of a representative in two steps of fixed order; an entry is a sum of n source
entries (n - 1 additions, counted as n) plus mu D: |found - exact| <= gamma(n + 2) (sum |source entries| + |mu D|)
(block_bound).  The preconditioner inverts the found block B~ = B + E; with M = k_fbsr_diag_inverse(B~) the project's
constant says ||(M - B~^-1) b|| <= C_INV kappa eps ||B~^-1 b|| in the scaled infinity norm for every b
(freepcg_ref.C_INV), that is || M B~ - I || <= C_INV kappa eps; and M B - I = (M B~ - I) - M E, so in the Jacobi scaling
d = sqrt(diag B) (B_s = B / d d^T, M_s = d M d, E_s <= bound / d d^T):

    || M_s B_s - I ||_inf <= C_INV kappa_2(B_s) eps + || |B_s^-1| E_s ||_inf (1 + C_INV kappa_2(B_s) eps)

(precond_bound; |M_s| <= |B_s^-1| (1 + C_INV kappa eps) entry-wise up to terms of second order in E, which are below
1e-25 here and dropped).
"""
import numpy as np

import assembly_ref as ar
import freepcg_ref as fp
import shared_ref as sr

LD = ar.LD
EPS = fp.EPS
C = 16


def free_rows(n_cams, free):
    """free [10] (a global mask) or [nC, 10] (global & per-camera) -> bool [nC, 10]"""
    f = np.asarray(free) != 0
    return np.broadcast_to(f.reshape(-1, 10), (n_cams, 10)).copy()


def fold_map(rep, free):
    """shared_ref.fold_map with a row of free bits per camera: (phi [nA], away [nA]).  A coordinate is shared when its
    camera's bit is set (a camera alone is its own representative: phi is the identity there)"""
    rep = np.asarray(rep)
    n_cams = rep.size
    fr_ = free_rows(n_cams, free)
    assert np.array_equal(fr_, fr_[rep]), "the members of a group carry equal rows"
    shared = np.hstack([fr_, np.zeros((n_cams, 6), dtype=bool)]).reshape(-1)
    t = np.arange(C * n_cams)
    phi = np.where(shared, C * rep[t // C] + t % C, t)
    return phi, phi != t


def fold_vector(v, phi):
    """P^T v, the members in ascending camera order (numpy adds repeated indices in the order of the operands)"""
    out = np.zeros_like(v)
    np.add.at(out, phi, v)
    return out


def fold_ea(ea, phi, away):
    e = fold_vector(np.asarray(ea), phi)
    e[away] = 0.0
    return e


class FoldedOp:
    """A of the module docstring on a list of blocks (jk, val = S0) in a dtype.  D [nA] or None (identity)."""

    def __init__(self, n_cams, jk, val, rep, free, mu, D=None, coeff=1.0, dtype=LD):
        self.n_cams, self.dtype = n_cams, dtype
        self.n = C * n_cams
        self.op = fp.ListOp(n_cams, jk, val, C, dtype)
        self.phi, self.away = fold_map(rep, free)
        self.kept = ~self.away
        self.mu, self.coeff = mu, coeff
        self.D = np.ones(self.n) if D is None else np.asarray(D, dtype=np.float64)[:self.n]
        self.mud = (dtype(mu) * self.D.astype(dtype))
        self.rowlen = np.bincount(self.op.rows, minlength=n_cams)     # entries of each camera's block row

    def expand(self, x):
        return np.asarray(x)[self.phi]

    def times(self, x, solve=False, mu_per_member=False, skip_member=None):
        """A x.  solve: folded-away entries 0 (what the conjugate gradients see) instead of the placeholder's product.
        Injected faults: mu_per_member (mu D x added to every member's q before the sum), skip_member = camera left
        out of every sum over its group"""
        dt = self.dtype
        x = np.asarray(x).astype(dt)
        p = x[self.phi]
        q = self.op.times(p)
        if mu_per_member:
            q = q + self.mud * p
        if skip_member is not None:
            q = q.copy()
            t = C * skip_member + np.arange(C)
            q[t[self.away[t]]] = 0
        y = fold_vector(q, self.phi)
        if not mu_per_member:
            y = y + self.mud * x
        y[self.away] = 0 if solve else (dt(self.coeff) + self.mud[self.away]) * x[self.away]
        return y

    def abs_times(self, x):
        """sum |terms| of every row of A x (zero at the folded-away coordinates)"""
        x = np.abs(np.asarray(x).astype(self.dtype))
        y = fold_vector(self.op.abs_times(x[self.phi]), self.phi) + np.abs(self.mud) * x
        y[self.away] = 0
        return y

    def terms(self):
        """m_r of the module docstring for every coordinate"""
        per = (C * self.rowlen)[np.arange(self.n) // C] + 1              # a member's products and its addition
        return np.bincount(self.phi, weights=per, minlength=self.n) + 2

    def product_bound(self, x):
        b = ar.gamma(self.terms()) * self.abs_times(x).astype(np.float64)
        xa = np.abs(np.asarray(x, dtype=np.float64)[self.away])            # the placeholder's product: three roundings
        b[self.away] = ar.gamma(3) * (abs(self.coeff) + np.abs(self.mu * self.D[self.away])) * xa
        return b

    def placeholder_product(self, x):
        """fl(fl(coeff + fl(mu D)) x) at the folded-away coordinates, in float64"""
        x = np.asarray(x, dtype=np.float64)
        return (self.coeff + self.mu * self.D[self.away]) * x[self.away]


# ---- the folded diagonal blocks ------------------------------------------------------------------------------------

def _fold_blocks(op, phi, B):
    """sum of the list's entries (rows, cols, B) into the diagonal blocks of P^T . P: [nC, 16, 16]"""
    out = np.zeros((op.n_cams, C, C), dtype=B.dtype)
    a = np.arange(C)
    ta = phi[C * op.rows[:, None] + a[None, :]]                        # [E, 16] target coordinate of every row
    tb = phi[C * op.cols[:, None] + a[None, :]]
    same = (ta // C)[:, :, None] == (tb // C)[:, None, :]
    e, i, j = np.nonzero(same)
    np.add.at(out, (ta[e, i] // C, ta[e, i] % C, tb[e, j] % C), B[e, i, j])
    return out


def folded_blocks(fo, drop_cross=False):
    """(B [nC, 16, 16] the diagonal blocks of A in the operator's dtype, bound [nC, 16, 16] of the kernels' two-step sum).
    drop_cross (an injected fault): only the members' own diagonal blocks are summed"""
    op = fo.op
    B = op.B
    if drop_cross:
        B = np.where((op.rows == op.cols)[:, None, None], B, 0)
    out = _fold_blocks(op, fo.phi, B)
    mag = _fold_blocks(op, fo.phi, np.abs(op.B)).astype(np.float64)
    cnt = _fold_blocks(op, fo.phi, np.ones(op.B.shape))
    k = np.arange(C)
    mud = fo.mud.reshape(-1, C)
    out[:, k, k] += mud
    mag[:, k, k] += np.abs(mud.astype(np.float64))
    aw = fo.away.reshape(-1, C)
    j, a = np.nonzero(aw)
    assert np.all(out[j, a, :] == mud[j, a][:, None] * (k[None, :] == a[:, None])), "a folded-away row received a term"
    out[j, a, a] = fo.dtype(fo.coeff) + mud[j, a]
    bound = ar.gamma(cnt + 2) * mag
    bound[j, a, :] = 0.0
    bound[j, :, a] = 0.0
    bound[j, a, a] = 2 * ar.U * np.abs(out[j, a, a]).astype(np.float64)
    return out, bound


def precond_bound(B, E):
    """(kappa_2(B_s), the allowed || M_s B_s - I ||_inf) of one block B (long double) and its entry bound E"""
    d = np.sqrt(np.diag(B).astype(np.float64))
    Bs = (B / np.outer(d, d).astype(B.dtype)).astype(np.float64)
    w = np.linalg.eigvalsh(Bs)
    kappa = float(w[-1] / w[0])
    first = fp.C_INV[C] * kappa * EPS
    carried = float((np.abs(np.linalg.inv(Bs)) @ (E / np.outer(d, d))).sum(axis=1).max())
    return kappa, first + carried * (1.0 + first)


def precond_residual(M, B):
    """|| M_s B_s - I ||_inf in long double"""
    d = np.sqrt(np.diag(B)).astype(LD)
    R = (np.asarray(M).astype(LD) * np.outer(d, d)) @ (B.astype(LD) / np.outer(d, d)) - np.eye(C, dtype=LD)
    return float(np.abs(R).sum(axis=1).max())


# ---- the twin of the grouped conjugate gradients ---------------------------------------------------------------------

def twin_pcg(fo, b, tol, max_iter, M=None, keep_p=False, **faults):
    """freepcg_ref.twin_pcg on the embedded A: the same recurrences and stop rule, the search direction kept expanded
    (p = P z + beta p), q = A p with folded-away entries 0, every inner product over the kept coordinates (r, z and q
    are zero at the others).  M: the block inverses to precondition with (default: the kernels' loops on
    folded_blocks in the operator's dtype).  Returns freepcg_ref.twin_pcg's dict; x is the expanded step"""
    dt = fo.dtype
    if M is None:
        M, bad = fp.block_inverse(folded_blocks(fo)[0], dt)
    else:
        M, bad = np.asarray(M).astype(dt), np.zeros(1, dtype=bool)
    prec = lambda v: np.einsum("jrc,jc->jr", M, v.reshape(-1, C)).reshape(-1)  # noqa: E731
    b = np.asarray(b).astype(dt).copy()
    b[fo.away] = 0
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z[fo.phi]
    rz, bb = r @ z, b @ b
    out = dict(hist=[1.0], converged=False, failed=bool(bad.any()), exhausted=False, p=[])
    tol2 = dt(tol) * dt(tol)
    rr = None
    it = 0
    with np.errstate(all="ignore"):
        while not out["failed"]:
            if rz == 0 or (it > 0 and rr <= tol2 * bb):
                out["converged"] = True
                break
            if it == max_iter:
                break
            q = fo.times(p, solve=True, **faults)
            pq = p[fo.kept] @ q[fo.kept]
            if not pq > 0:
                out["failed"] = True
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            z = prec(r)
            rr, rzn = r @ r, r @ z
            p = z[fo.phi] + (rzn / rz) * p
            rz = rzn
            it += 1
            out["hist"].append(float(np.sqrt(rr / bb)) if bb > 0 else 0.0)
            if keep_p:
                out["p"].append(p.astype(np.float64))
    out["exhausted"] = not out["converged"] and not out["failed"]
    out["iters"] = it
    out["x"] = x.astype(np.float64)
    out["relres"] = out["hist"][-1] if it > 0 else (0.0 if not bb > 0 or rz == 0 else 1.0)
    return out


def relres_and_gap(fo, x, b, iters):
    """freepcg_ref.list_relres_and_gap against the folded operator: (||b - A x||_2 / ||b||_2 over the kept coordinates in
    the operator's dtype, gap_unit = eps iters || |A| |x| ||_inf / ||b||_inf).  x: the embedded or the expanded step (A
    reads the kept coordinates alone)"""
    b = np.asarray(b).astype(fo.dtype).copy()
    b[fo.away] = 0
    r = b - fo.times(x, solve=True)
    tr = float(np.sqrt(r @ r) / np.sqrt(b @ b))
    return tr, EPS * max(iters, 1) * float(fo.abs_times(x).max() / np.abs(b).max())


# ---- inputs -------------------------------------------------------------------------------------------------------------

def dense_blocks(rt, mu):
    """(jk, S0 blocks, unfolded e_a) of a SharedRoute's 80-bit per-camera Schur complement at mu (the points damped, the
    cameras' mu taken off again), every block of the lower block triangle kept: the list a host test folds when it has
    no handle"""
    S, ea = rt.twin.schur_blocks(mu)
    S = S.copy()
    k = np.arange(rt.nA)
    S[k, k] -= LD(mu)
    jk = np.array([(j, i) for j in range(rt.nC) for i in range(j + 1)], dtype=np.int32)
    return jk, fp.blocks_of(S, jk, C), ea


def interleaved(n_cams):
    """(problem, kc, labels j % 3) of freepcg_ref.band_scene(n_cams) with the members' intrinsics set to their
    representative's: three interleaved groups, no representative pattern contiguous"""
    from freekd_twin import start_kc
    lab = (np.arange(n_cams) % 3).astype(np.int32)
    p, kc = sr.share_problem(fp.band_scene(n_cams), start_kc(n_cams), lab)
    return p, kc, lab


_BURST = {}


def burst_case(name, k, labels, mu):
    """freepcg_ref.burst_case with groups, under its admission rule: S0 = dominant(negative=True) on the named pattern
    (every intrinsic free), A its fold under `labels` at mu; the long-double twin's relative residual drops by >= 4x
    from iteration k - 1 to k and is still >= 1e-14 there; tol = their geometric mean makes the solve stop after exactly
    k iterations.  The first delta of BURST_DELTAS that qualifies, or None"""
    key = (name, k, tuple(np.asarray(labels).tolist()), mu)
    if key not in _BURST:
        n_cams, blocks = fp.fpattern(name)
        jk = np.array(sorted([(j, j) for j in range(n_cams)] + list(blocks)), dtype=np.int32)
        rep = sr.representatives(labels)
        found = None
        for delta in fp.BURST_DELTAS:
            S = fp.dominant(n_cams, blocks, delta, C, 0.0, 7, negative=True)
            b = fp.rhs(S, 8)
            val = fp.blocks_of(S, jk, C)
            fo = FoldedOp(n_cams, jk, val, rep, np.ones(10), mu)
            h = twin_pcg(fo, b, 0.0, k)["hist"]                        # (e_a as psba_set_sparse_S takes it: 0 where folded away)
            if len(h) > k and h[k] >= 1e-14 and h[k - 1] >= 4.0 * h[k] and min(h[:k]) > np.sqrt(h[k - 1] * h[k]):
                found = dict(delta=delta, tol=float(np.sqrt(h[k - 1] * h[k])), val=val, b=b, jk=jk, hist=h, fo=fo)
                break
        _BURST[key] = found
    return _BURST[key]
