"""Host judges of the two free-intrinsics routes (PSBA_CAMERA_FREE_K, camera blocks of 11, and PSBA_CAMERA_FREE_KD,
blocks of 16) for one damping try, entry by entry (no GPU): tests/test_free_entrywise_ref.py applies them to a plain
fp64 numpy evaluation and to injected faults, tests/test_gpu_free_entrywise.py to the kernels.

The reference is the numpy twin tests/freekd_twin.py: its fp64 Jacobian blocks e, A, B with every sum in extended
precision (np.longdouble, assembly_ref.LD).  The 11-block route is TwinKD(p, None, K_ONLY) restricted to the columns
SEL11 = (0..4, 10..15) of every camera.  Notation, gamma(k) and u = 2^-53 + 2^-63 are assembly_ref's; every bound is
built from the entry's own terms, none from the maximum of an array, and no constant is fitted to a GPU result.

S and e_a (C1) use the scaled measure of test_gpu_freekd.py: |dS_rc| <= tol d_r d_c, |de_a,r| <= tol d_r sqrt(cost),
d = sqrt(diag N + mu), tol = scaled_tol(p) = 64 eps (largest observation count of one camera + 16).

dp_a (C2) is judged as a solve of the system it was computed from (the S and e_a read back from the device): with
D = diag(S)^-1/2 the normwise backward error of D^-1 dp_a for (D S D) y = D e_a must stay below
test_gpu_dense_solve.ETA_MAX.  An unpivoted Cholesky commutes with a diagonal scaling up to the roundings of the scaling
itself, so this is the backward error the factorization can be held to; in the unscaled system the focal-length rows
(1e12) would hide every other row.  The forward error against dense_ref.refined_solution of the scaled system is held
to 2 cond_2(D S D) 1e-14, the rule of test_gpu_dense_solve.py.

dp_b (C3) is judged per point as a residual: with the device's dp_a and dp_b, and V_i, W_a, g_b,i summed in extended
precision from the twin's blocks,
    r_i = (V_i + mu I) dp_b,i - (g_b,i - sum_a W_a^T dp_a,j(a)).
The kernel solves (V*_k + dV) dp_b = e_b,k with ITS V*_k and e_b,k, so r_i = (V* - V*_k) dp_b - dV dp_b + (e_b,k - e_b)
and every entry r of r_i is bounded by the sum of
  * the L D L^T solve: |dV| <= gamma(LDL_K) |L| |D| |L^T| (Higham, Thm 10.4: 3 n + 1 = 10 roundings for a Cholesky
    solve with n = 3; sym3_ldl / sym3_ldl_solve multiply by a stored reciprocal in six places where the theorem
    divides, one more rounding each: LDL_K = 16), and (|L| |D| |L^T|)_rc <= sqrt(V*_rr V*_cc) for a positive definite
    V* (Cauchy-Schwarz on the rows of D^1/2 L^T): gamma(16) sum_c sqrt(V*_rr V*_cc) |dp_b,c|;
  * env(V*)_rc |dp_b,c|, env(V*) = |c| gamma(n_i + 2) sum |B|^T |B| (assembly_ref's K1 rule for a sum of n_i terms in
    any order) + u |V*_rr| on the diagonal (the damping add) + the Jacobian slack below;
  * env(g_b)_r = |c_g| gamma(n_i + 2) sum |B|^T |e| + the slacks below;
  * e_b's own sum: cnp n_i products and the subtraction, gamma(cnp n_i + 2) (|g_b,r| + sum_a sum_k |W_a,kr| |dp_a,k|);
  * env(W_a)_kr |dp_a,k|, env(W) = |c| gamma(3) |A|^T |B| (two products, one add, the scaling) + the Jacobian slack.
Slacks.  The kernel and the twin are two fp64 evaluations of the same derivatives, the argument assembly_ref makes for
JACOBIAN_SLACK = 2^-40 and RESIDUAL_SLACK = 2^-44; both constants are taken from there unchanged.  Here the two
texts differ (the twin composes d(u, v)/dP with matrix products, the kernel expands it), so an entry that cancels in
one text need not in the other: the slack of an entry of A is 2^-40 times the LARGEST entry (both rows) of that
observation's Jacobian within the same parameter group -- intrinsics, distortion, rotation, translation -- and of an
entry of B 2^-40 times the largest entry of B_a; never the entry's own magnitude.  With sA, sB these slacks:
env(W) += |c| (sA^T |B| + |A|^T sB + sA^T sB), env(V) += |c| sum (sB^T |B| + |B|^T sB + sB^T sB),
env(g) += |c_g| sum (sJ^T (|e| + es) + |J|^T es), es = assembly_ref.residual_slack(m, proj).
This slack is an assumption nobody has measured against a GPU; it is about 1000 gamma, so it is the bound wherever it
applies (DESIGN 7d records the worst ratios found).

The four try scalars (C4) are assembly_ref.try_scalars' (it takes nA, not a block size): dp_l2, gain_den and newp_l2
from the device's own dp and proposal summed in extended precision, gain_den with env(g) above; new_cost against the
twin's residuals at the device's proposal, per observation gamma(2) s (+ gamma(8) s for the loss slot, the identity
here) and the residual slack rule.

Marquardt's damping (psba_set_damping): every judge takes a Rule (kind, dmin, dmax; identity is the default
and leaves each result bit for bit what it was).  N + mu D in the place of N + mu I, D_k = min(max(N_kk, dmin), dmax).
  * The reference D (damp_ref) is the clamp of the diagonal of the sums above in extended precision -- the placeholder
    coeff at a held coordinate -- rounded once.  The kernels clamp THEIR stored diagonal entry, a K1 sum of squares:
    it differs from the exact one by env(N_kk) = |c| gamma(n + 2) sum J_k^2 + the Jacobian slack (2 |J_k| s + s^2
    summed), and the clamp is 1-Lipschitz, so |D_device - D_ref| <= env(N_kk) + u D_ref (the reference's own
    rounding); 0 at a held coordinate.  envD is that envelope, and mu envD goes wherever mu D enters below.
  * C1: schur_blocks restates TwinKD.schur_blocks on the route's own columns with U_kk + mu D_k and
    V_i + mu diag(D_i); the scaled measure keeps its form with d_r = sqrt(N_rr + mu D_r) and tol = scaled_tol(p).
  * C3: V* = V_i + mu diag(D_i).  camera_model.h's damp_point_block forms each diagonal entry as
    fma(mu, clamp(v_rr), v_rr): ONE rounding per diagonal entry (the clamp is exact), the count the identity rule has
    for its add, so the diagonal of env(V*) is u |V*_rr| + mu envD_r + env(V)_rr.  k_free_Y and k_free_backsub_pts
    both come through that function with the same stored V_i, so the solve is against the V* Y was made with and the
    L D L^T term is unchanged.
  * C4: gain_den = sum dp g + sum (mu D) dp^2 with the DEVICE's D (psba_get_damping_diag; D itself is judged on its
    own, check_damp_diag) as weights.  kernels_free.hip forms mud = mu * D[t] (k_free_backsub_cams,
    k_kd_backsub_cams_groups) or mu * clamp(v_rr) (k_free_backsub_pts) and then d * (mud * d + g): one multiply more
    than under mu I, so the count of roundings before the sum goes from three to four (try_scalars' `extra`)."""
import collections

import numpy as np

import assembly_ref as ar
import dense_ref as dr
from freekd_twin import CNP, TwinKD, ldl_rows, obs_by_point, start_kc

LD = ar.LD
ALL = (1,) * 10
K_ONLY = (1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
SEL11 = np.r_[0:5, 10:16]
GROUPS = {16: (slice(0, 5), slice(5, 10), slice(10, 13), slice(13, 16)), 11: (slice(0, 5), slice(5, 8), slice(8, 11))}
LDL_K = 16
IDENTITY, MARQUARDT = 0, 1   # PSBA_DAMPING_IDENTITY, PSBA_DAMPING_MARQUARDT
DMIN, DMAX = 1e-6, 1e32      # the defaults of psba_set_damping


class Rule(collections.namedtuple("Rule", "kind dmin dmax")):
    """the damping rule of a try: N + mu I (identity, the default) or N + mu D, D = clamp(diag N, dmin, dmax)"""
    __slots__ = ()

    def __new__(cls, kind=IDENTITY, dmin=DMIN, dmax=DMAX):
        return super().__new__(cls, int(kind), float(dmin), float(dmax))

    @property
    def marquardt(self):
        return self.kind == MARQUARDT

    def clamp(self, x):
        return np.minimum(np.maximum(x, self.dmin), self.dmax)

    def halved(self):
        return Rule(self.kind, self.dmin / 2.0, self.dmax / 2.0)

    def __str__(self):
        return "identity" if not self.marquardt else f"marquardt({self.dmin:g}, {self.dmax:g})"


NO_RULE = Rule()


class Route:
    """cnp = 16: TwinKD(p, start_kc, free); cnp = 11: TwinKD(p, None, K_ONLY) and the columns SEL11"""

    def __init__(self, p, cnp, free=None):
        self.p, self.cnp = p, cnp
        self.nC, self.nP, self.nO = int(p["nC"]), int(p["nP"]), int(p["nO"])
        if cnp == 16:
            self.free = ALL if free is None else tuple(free)
            self.twin = TwinKD(p, start_kc(self.nC), self.free)
        else:
            self.free = K_ONLY
            self.twin = TwinKD(p, None, K_ONLY)
        self.i, self.j = self.twin.i, self.twin.j
        self.nA, self.nB = cnp * self.nC, 3 * self.nP
        self.nT = self.nA + self.nB
        # rows / columns of the twin's 16-wide camera part that this route has
        self.sel = np.arange(CNP) if cnp == 16 else SEL11
        self.rows = (CNP * np.arange(self.nC)[:, None] + self.sel[None, :]).reshape(-1)
        self.held = np.flatnonzero(~self.twin.free_a[self.rows])
        self.held_pts = np.zeros(self.nP, dtype=bool)        # (held_ref's routes hold points; schur_blocks skips them)

    def current(self):
        """the twin's current parameters as this route has them: (cams [nC, cnp], pts [nP, 3])"""
        return self.twin.cams[:, self.sel].copy(), self.twin.pts.copy()

    def schur_start(self, dtype, fault=None):
        """what schur_blocks adds the observations' sums to: (U, g_a, V, g_b), zero without priors"""
        return (np.zeros((self.nC, self.cnp, self.cnp), dtype), np.zeros((self.nC, self.cnp), dtype),
                np.zeros((self.nP, 3, 3), dtype), np.zeros((self.nP, 3), dtype))

    def cams16(self, cams):
        """[nC, cnp] of this route -> the twin's [nC, 16]"""
        cams = np.asarray(cams, dtype=np.float64).reshape(self.nC, self.cnp)
        if self.cnp == 16:
            return cams
        out = np.zeros((self.nC, CNP))
        out[:, SEL11] = cams
        return out

    def blocks(self):
        """e [nO, 2], A [nO, 2, cnp], B [nO, 2, 3], proj [nO, 2] at the start"""
        e, A, B = self.twin.linearize()
        return e, A[:, :, self.sel], B, self.twin.t.m - e

    def residuals(self, cams, pts):
        """fp64 residuals [nO, 2] and projections at (cams [nC, cnp], pts)"""
        e = self.twin.residual(self.cams16(cams), pts)
        self.twin._set(None, None)
        return e, self.twin.t.m - e

    def pick(self, S, ea):
        """the twin's 16-wide S, e_a restricted to this route"""
        return S[np.ix_(self.rows, self.rows)], ea[self.rows]

    def pick_full(self, N, g):
        """the twin's dense N, g (cameras then points) restricted to this route"""
        idx = np.r_[self.rows, CNP * self.nC + np.arange(self.nB)]
        return N[np.ix_(idx, idx)], g[idx]


def group_slack(A, groups):
    """JACOBIAN_SLACK times the largest entry (both rows) of each observation's block within the parameter group"""
    s = np.zeros(A.shape)
    a = np.abs(A)
    for g in groups:
        s[:, :, g] = a[:, :, g].max(axis=(1, 2))[:, None, None]
    return ar.JACOBIAN_SLACK * s


def sums(rt, coeff=1.0, coeff_g=1.0):
    """V [nP,3,3], W [nO,cnp,3], g [nT] of the route summed in extended precision from the twin's blocks, with the
    envelopes of the module docstring; also diagU [nA] (the fp64 diagonal of U with the placeholder) and cost."""
    e, A, B, proj = rt.blocks()
    i, j, nC, nP = rt.i, rt.j, rt.nC, rt.nP
    AL, BL, eL = ar.ld(A), ar.ld(B), ar.ld(e)
    aA, aB, ae = np.abs(A), np.abs(B), np.abs(e)
    sA, sB = group_slack(A, GROUPS[rt.cnp]), group_slack(B, (slice(0, 3),))
    es = ar.residual_slack(rt.twin.t.m, proj)
    c, cg = abs(coeff), abs(coeff_g)
    W = LD(coeff) * np.einsum("ark,arc->akc", AL, BL)
    envW = c * (ar.gamma(3) * np.einsum("ark,arc->akc", aA, aB) + np.einsum("ark,arc->akc", sA, aB + sB)
                + np.einsum("ark,arc->akc", aA, sB))
    Vx, n_i = ar._segsum(np.einsum("ari,ark->aik", BL, BL), i, nP)
    Va, _ = ar._segsum(np.einsum("ari,ark->aik", aB, aB), i, nP)
    Vs, _ = ar._segsum(np.einsum("ari,ark->aik", sB, 2 * aB + sB), i, nP)
    envV = c * (ar.gamma(n_i + 2)[:, None, None] * Va + Vs)
    gbx, _ = ar._segsum(np.einsum("ari,ar->ai", BL, eL), i, nP)
    gba, _ = ar._segsum(np.einsum("ari,ar->ai", aB, ae), i, nP)
    gbs, _ = ar._segsum(np.einsum("ari,ar->ai", sB, ae + es) + np.einsum("ari,ar->ai", aB, es), i, nP)
    gax, n_j = ar._segsum(np.einsum("ari,ar->ai", AL, eL), j, nC)
    gaa, _ = ar._segsum(np.einsum("ari,ar->ai", aA, ae), j, nC)
    gas, _ = ar._segsum(np.einsum("ari,ar->ai", sA, ae + es) + np.einsum("ari,ar->ai", aA, es), j, nC)
    g = LD(coeff_g) * np.concatenate([gax.reshape(-1), gbx.reshape(-1)])
    envg = cg * np.concatenate([(ar.gamma(n_j + 2)[:, None] * gaa + gas).reshape(-1),
                                (ar.gamma(n_i + 2)[:, None] * gba + gbs).reshape(-1)])
    diagU, _ = ar._segsum((A * A).sum(axis=1), j, nC)
    diagU = coeff * diagU.reshape(-1)
    diagU[rt.held] = coeff
    diagV, _ = ar._segsum((B * B).sum(axis=1), i, nP)
    # the same diagonal in extended precision with its K1 envelope (what damp_ref clamps)
    dUx, _ = ar._segsum((AL * AL).sum(axis=1), j, nC)
    dUa, _ = ar._segsum((aA * aA).sum(axis=1), j, nC)
    dUs, _ = ar._segsum((sA * (2 * aA + sA)).sum(axis=1), j, nC)
    diagUx = LD(coeff) * dUx.reshape(-1)
    envdU = c * (ar.gamma(n_j + 2)[:, None] * dUa + dUs).reshape(-1)
    diagUx[rt.held] = LD(coeff)
    envdU[rt.held] = 0.0
    k3 = np.arange(3)
    return dict(W=W, envW=envW, V=LD(coeff) * Vx, envV=envV, g=g, envg=envg, n_i=n_i, n_j=n_j, diagU=diagU,
                diagV=coeff * diagV.reshape(-1), cost=float(np.sum(eL * eL)), A=A, B=B, e=e, diagUx=diagUx, envdU=envdU,
                diagVx=(LD(coeff) * Vx)[:, k3, k3].reshape(-1), envdV=envV[:, k3, k3].reshape(-1), coeff=float(coeff))


def damp_ref(rt, sm, rule=NO_RULE):
    """(D [nT], envD [nT]) of the module docstring: the clamp of the extended-precision diagonal rounded once, and the
    envelope |D_device - D| must stay inside.  Identity: (ones, zeros), so that mu D is mu exactly."""
    if not rule.marquardt:
        return np.ones(rt.nT), np.zeros(rt.nT)
    D = rule.clamp(np.concatenate([sm["diagUx"], sm["diagVx"]])).astype(np.float64)
    env = np.concatenate([sm["envdU"], sm["envdV"]])
    free = np.ones(rt.nT, dtype=bool)
    free[rt.held] = False
    return D, np.where(free, env + ar.U * D, 0.0)


def check_damp_diag(D, sm_diag, envN, rule, held, coeff=1.0):
    """The device's D [n] against the clamp of the extended-precision diagonal sm_diag [n] (envelope envN [n], held:
    indices whose entry is the placeholder coeff).  Returns the worst |D - D_ref| / (envN + u D_ref) over the entries
    that have an envelope; asserts the exact parts: the clamp itself where the reference lies beyond it by more than
    its envelope, clamp(coeff) at held coordinates.  Also returns the counts (at dmin, at dmax) of such entries."""
    D = np.asarray(D, dtype=np.float64)
    want = rule.clamp(sm_diag).astype(np.float64)
    x = sm_diag.astype(np.float64)
    low, high = x + envN < rule.dmin * (1.0 - ar.U), x - envN > rule.dmax * (1.0 + ar.U)
    assert np.all(D[low] == rule.dmin), "an entry below dmin by more than its envelope is not dmin itself"
    assert np.all(D[high] == rule.dmax), "an entry above dmax by more than its envelope is not dmax itself"
    assert np.all(D[held] == min(max(coeff, rule.dmin), rule.dmax)), "D of a held coordinate is not clamp(coeff)"
    assert np.all((D >= rule.dmin) & (D <= rule.dmax))
    bound = envN + ar.U * want
    bound[held] = 0.0
    ratio, k = ar.excess(D, ar.ld(want), bound)
    return ratio, k, int(low.sum()), int(high.sum())


def block_diagonal(U):
    """[nA, nA] with the blocks U [nC, cnp, cnp] on its diagonal, in U's dtype"""
    nC, cnp, _ = U.shape
    S = np.zeros((nC * cnp, nC * cnp), U.dtype)
    for j in range(nC):
        S[cnp * j:cnp * j + cnp, cnp * j:cnp * j + cnp] = U[j]
    return S


def schur_blocks(rt, mu, D, camera=True, dtype=np.longdouble, coeff=1.0, fault=None):
    """TwinKD.schur_blocks restated on the route's own columns for N + mu diag(D): S [nA, nA] and e_a with every sum in
    `dtype` (80-bit), U_kk + mu D_k (camera=False: the camera diagonal is left undamped, for the fold of shared_ref)
    and V_i + mu diag(D_i); the placeholder coeff at held coordinates.  The one restatement for every route of the
    free-intrinsics references; what differs is asked of the route: rt.held_pts (a held point is skipped: its W is
    zero, so it contributes nothing, and at mu = 0 its V is singular) and rt.schur_start (the prior terms the sums start
    from, with prior_ref's faults).  Under the identity rule D is all ones and mu D is mu exactly."""
    e, A, B, _ = rt.blocks()
    e, A, B = e.astype(dtype), A.astype(dtype), B.astype(dtype)
    cnp, nA = rt.cnp, rt.nA
    D = np.asarray(D, dtype=np.float64).astype(dtype)
    mu = dtype(mu)
    U, ga, V, gb = rt.schur_start(dtype, fault)
    np.add.at(U, rt.j, np.einsum("nri,nrk->nik", A, A))
    np.add.at(ga, rt.j, np.einsum("nri,nr->ni", A, e))
    np.add.at(V, rt.i, np.einsum("nri,nrk->nik", B, B))
    np.add.at(gb, rt.i, np.einsum("nri,nr->ni", B, e))
    W = np.einsum("nri,nrk->nik", A, B)
    S = block_diagonal(U)
    S[rt.held, rt.held] = dtype(coeff)
    if camera:
        S[np.arange(nA), np.arange(nA)] += mu * D[:nA]
    ea = ga.reshape(-1).copy()
    for i, obs in obs_by_point(rt.i, rt.nP):
        if rt.held_pts[i]:
            continue
        Wi = W[obs].reshape(-1, 3)
        Yi = ldl_rows(V[i] + np.diag(mu * D[nA + 3 * i:nA + 3 * i + 3]), Wi)
        rows = (cnp * rt.j[obs][:, None] + np.arange(cnp)[None, :]).reshape(-1)
        S[np.ix_(rows, rows)] -= Yi @ Wi.T
        ea[rows] -= Yi @ gb[i]
    return S, ea


def schur_ref(rt, sm, mu, rule=NO_RULE):
    """S and e_a of the route in 80-bit, rounded once to double (identity: TwinKD.schur_blocks, as it always was)"""
    if not rule.marquardt:
        S, ea = rt.pick(*rt.twin.schur_blocks(mu))
    else:
        S, ea = schur_blocks(rt, mu, damp_ref(rt, sm, rule)[0])
    return S.astype(np.float64), ea.astype(np.float64)


def scale_diag(rt, sm, mu, rule=NO_RULE):
    """d [nA] of the scaled measure: sqrt(N_rr + mu D_r) (identity: sqrt(N_rr + mu))"""
    return np.sqrt(sm["diagU"] + mu * damp_ref(rt, sm, rule)[0][:rt.nA])


def check_exact_parts(rt, S, ea, mu, rule=NO_RULE, coeff=1.0):
    """C1's exact checks: a held coordinate has a zero row, e_a = 0 and coeff + mu clamp(coeff) on the diagonal; the
    block of a camera without observations is fl(mu dmin) on its free coordinates (mu under the identity rule), that
    placeholder on held ones, zero elsewhere, and its off-diagonal blocks and e_a are zero."""
    cnp, nC, held = rt.cnp, rt.nC, rt.held
    dh = mu * float(rule.clamp(coeff)) if rule.marquardt else mu
    off = S[held].copy()
    off[np.arange(held.size), held] = 0.0
    assert np.all(off == 0.0) and np.all(ea[held] == 0.0), "a held row is not clear"
    assert np.all(S[held, held] == coeff + dh), "the diagonal of a held coordinate"
    empty = np.flatnonzero(np.bincount(rt.j, minlength=nC) == 0)
    for j in empty:
        rows = np.arange(cnp * j, cnp * j + cnp)
        want = (mu * rule.dmin if rule.marquardt else mu) * np.eye(cnp)
        hj = held[(held >= rows[0]) & (held <= rows[-1])] - rows[0]
        want[hj, hj] = coeff + dh
        assert np.array_equal(S[np.ix_(rows, rows)], want), f"the block of camera {j}, which has no observation"
        assert np.all(np.delete(S[rows], rows, axis=1) == 0.0) and np.all(ea[rows] == 0.0)
    return empty


def dpb_residual(rt, sm, dp, mu, rule=NO_RULE):
    """(r [nB], bound [nB]) of the module docstring from the step dp [nT] (cameras then points) being judged"""
    cnp, nA = rt.cnp, rt.nA
    dpa = np.asarray(dp[:nA], dtype=np.float64).reshape(-1, cnp)
    dpb = np.asarray(dp[nA:], dtype=np.float64).reshape(-1, 3)
    Vs = sm["V"].copy()
    k = np.arange(3)
    if rule.marquardt:
        D, envD = damp_ref(rt, sm, rule)
        Vs[:, k, k] += LD(mu) * ar.ld(D[nA:].reshape(-1, 3))
    else:
        Vs[:, k, k] += LD(mu)
    dL, ad = ar.ld(dpa)[rt.j], np.abs(dpa)[rt.j]
    t, n_i = ar._segsum(np.einsum("akc,ak->ac", sm["W"], dL), rt.i, rt.nP)
    gb = sm["g"][nA:].reshape(-1, 3)
    r = np.einsum("irc,ic->ir", Vs, ar.ld(dpb)) - (gb - t)
    aW = np.abs(sm["W"].astype(np.float64))
    wd, _ = ar._segsum(np.einsum("akc,ak->ac", aW, ad), rt.i, rt.nP)
    wenv, _ = ar._segsum(np.einsum("akc,ak->ac", sm["envW"], ad), rt.i, rt.nP)
    Vd = Vs.astype(np.float64)
    dg = np.sqrt(Vd[:, k, k])
    envV = sm["envV"].copy()
    envV[:, k, k] += ar.U * Vd[:, k, k]
    if rule.marquardt:
        envV[:, k, k] += abs(mu) * envD[nA:].reshape(-1, 3)
    ab = np.abs(dpb)
    bound = (ar.gamma(LDL_K) * dg * (dg * ab).sum(axis=1)[:, None] + np.einsum("irc,ic->ir", envV, ab)
             + sm["envg"][nA:].reshape(-1, 3) + ar.gamma(cnp * n_i + 2)[:, None] * (np.abs(gb.astype(np.float64)) + wd)
             + wenv)
    return r.reshape(-1), bound.reshape(-1)


def scalars(rt, sm, dp, newcams, newpts, mu, D=None):
    """assembly_ref.try_scalars for this route: {name: (exact, bound)} from the step and proposal being judged.
    D [nT]: the weights of Marquardt's rule, gain_den = sum dp g + sum (mu D) dp^2 (the device's own D)"""
    e_new, proj = rt.residuals(newcams, newpts)
    newp = np.concatenate([np.asarray(newcams).reshape(-1), np.asarray(newpts).reshape(-1)])
    if D is None:
        return ar.try_scalars(dp, newp, mu, sm["g"], rt.nA, (e_new * e_new).sum(axis=1),
                              e_slack=ar.residual_slack(rt.twin.t.m, proj), envg=sm["envg"])
    return ar.try_scalars(dp, newp, LD(mu) * ar.ld(D), sm["g"], rt.nA, (e_new * e_new).sum(axis=1),
                          e_slack=ar.residual_slack(rt.twin.t.m, proj), envg=sm["envg"], extra=1)


def solve_judge(S, ea, dpa):
    """(backward error of D^-1 dp_a for (D S D) y = D e_a, its forward error against the refined solution,
    cond_2(D S D)), D = diag(S)^-1/2"""
    S = np.asarray(S, dtype=np.float64)
    d = 1.0 / np.sqrt(np.diag(S))
    A = d[:, None] * S * d[None, :]
    y, b = np.asarray(dpa) / d, d * np.asarray(ea)
    return dr.backward_error(A, y, b), dr.forward_error(y, dr.refined_solution(A, b)), dr.cond2(A)


# ---- plain fp64 evaluations (what the kernels compute, in numpy): the judges' own test ---------------------------------

def ldl_solve(v, w):
    """camera_model.h's sym3_ldl / sym3_ldl_solve in fp64 numpy: v [n, 3, 3], w [n, m, 3] -> y with (v) y = w per row"""
    i0 = 1.0 / v[:, 0, 0]
    l10, l20 = v[:, 0, 1] * i0, v[:, 0, 2] * i0
    d1 = v[:, 1, 1] - l10 * v[:, 0, 1]
    i1 = 1.0 / d1
    l21 = (v[:, 1, 2] - l20 * v[:, 0, 1]) * i1
    i2 = 1.0 / (v[:, 2, 2] - l20 * v[:, 0, 2] - l21 * l21 * d1)
    b = lambda x: x[:, None]  # noqa: E731
    z1 = w[:, :, 1] - b(l10) * w[:, :, 0]
    z2 = w[:, :, 2] - b(l20) * w[:, :, 0] - b(l21) * z1
    y2 = z2 * b(i2)
    y1 = z1 * b(i1) - b(l21) * y2
    y0 = w[:, :, 0] * b(i0) - b(l10) * y1 - b(l20) * y2
    return np.stack([y0, y1, y2], axis=2)


def closed_form_solve(v, w):
    """w times camera_model.h's sym3_inverse (adjugate over T = -det) in fp64 numpy"""
    a11, a12, a13, a22, a23, a33 = v[:, 0, 0], v[:, 0, 1], v[:, 0, 2], v[:, 1, 1], v[:, 1, 2], v[:, 2, 2]
    T = a33 * a12 * a12 - 2.0 * a12 * a13 * a23 + a22 * a13 * a13 + a11 * a23 * a23 - a11 * a22 * a33
    iT = -1.0 / T
    X = np.empty_like(v)
    X[:, 0, 0] = (a22 * a33 - a23 * a23) * iT
    X[:, 0, 1] = X[:, 1, 0] = (a13 * a23 - a12 * a33) * iT
    X[:, 0, 2] = X[:, 2, 0] = (a12 * a23 - a13 * a22) * iT
    X[:, 1, 1] = (a11 * a33 - a13 * a13) * iT
    X[:, 1, 2] = X[:, 2, 1] = (a12 * a13 - a11 * a23) * iT
    X[:, 2, 2] = (a11 * a22 - a12 * a12) * iT
    return w @ X


def plain_damp_diag(rt, U, V, rule, fault=None):
    """k_free_damp_diag in fp64 numpy: D [nT] from the stored diagonals of U [nC, cnp, cnp] (placeholder 1 at held
    coordinates) and V [nP, 3, 3].  Faults for test_free_entrywise_ref.py: "no-low-clamp" (D = min(N_kk, dmax)),
    "cam-mod-64" (camera j reads the entries of camera j mod 64)."""
    k, k3 = np.arange(rt.cnp), np.arange(3)
    n = np.concatenate([U[:, k, k].reshape(-1), V[:, k3, k3].reshape(-1)])
    n[rt.held] = 1.0
    D = np.minimum(n, rule.dmax) if fault == "no-low-clamp" else rule.clamp(n)
    if fault == "cam-mod-64":
        D[:rt.nA] = D[:rt.nA].reshape(-1, rt.cnp)[np.arange(rt.nC) % 64].reshape(-1)
    return D


def plain_sums(rt, e, A, B, prior=None):
    """K1 in fp64 numpy: U [nC, cnp, cnp], g_a, V [nP, 3, 3], g_b and W [nO, cnp, 3] of the blocks; prior = (L, L d, G,
    G d) is added to the four sums (prior_ref)"""
    U = np.zeros((rt.nC, rt.cnp, rt.cnp))
    np.add.at(U, rt.j, np.einsum("ari,ark->aik", A, A))
    ga = np.zeros((rt.nC, rt.cnp))
    np.add.at(ga, rt.j, np.einsum("ari,ar->ai", A, e))
    V = np.zeros((rt.nP, 3, 3))
    np.add.at(V, rt.i, np.einsum("ari,ark->aik", B, B))
    gb = np.zeros((rt.nP, 3))
    np.add.at(gb, rt.i, np.einsum("ari,ar->ai", B, e))
    if prior is not None:
        U += prior[0]
        ga += prior[1]
        V += prior[2]
        gb += prior[3]
    return U, ga, V, gb, np.einsum("ark,arc->akc", A, B)


def plain_scatter(rt, U, dU, ga, V, gb, W, mu, D, point_solve=ldl_solve, camera=True):
    """The Schur assembly in fp64 numpy: V* = V + mu diag(D_b), Y = W V*^-1 by `point_solve`, S from the blocks U with
    dU + mu D_a on its diagonal (dU [nA]: the stored diagonal, placeholders included; camera=False: dU alone), then
    Y W^T and Y g_b of every point taken off S and e_a.  numpy rounds the product mu D_r and the sum where
    damp_point_block has one fma.  Returns (S, e_a, V*)."""
    cnp, nA = rt.cnp, rt.nA
    k3 = np.arange(3)
    Vs = V.copy()
    Vs[:, k3, k3] += mu * D[nA:].reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        Y = point_solve(Vs[rt.i], W)
    S = block_diagonal(U)
    S[np.arange(nA), np.arange(nA)] = dU + mu * D[:nA] if camera else dU
    ea = ga.reshape(-1).copy()
    for i, obs in obs_by_point(rt.i, rt.nP):
        rows = (cnp * rt.j[obs][:, None] + np.arange(cnp)[None, :]).reshape(-1)
        S[np.ix_(rows, rows)] -= Y[obs].reshape(-1, 3) @ W[obs].reshape(-1, 3).T
        ea[rows] -= Y[obs].reshape(-1, 3) @ gb[i]
    return S, ea, Vs


def plain_solve(S, ea, fallback=False):
    """dp_a of S dp_a = e_a by a Cholesky factorization of S scaled by its own diagonal (fallback: by LU where a
    faulted S is not positive definite)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 / np.sqrt(np.diag(S))
        try:
            L = np.linalg.cholesky(d[:, None] * S * d[None, :])
        except np.linalg.LinAlgError:
            if not fallback:
                raise
            return np.linalg.solve(S, ea)
    return d * np.linalg.solve(L.T, np.linalg.solve(L, d * ea))


def plain_finish(rt, S, ea, pc, dpa, mu, D, hold_b=None, keep=None, gain_den=None):
    """The rest of a try from the camera step dpa [nA] (per camera, the held entries cleared by the caller): dp_b by
    L D L^T against pc["Vs"] (zero at the points hold_b), the proposal and the four sums.  keep: the mask of the
    parameters that count in dp_l2 and newp_l2 (shared_ref: every distinct one once); gain_den(dp, counted dp): the
    caller's own sum where dp . (mu D dp + g) is not it."""
    cnp, nA = rt.cnp, rt.nA
    eb = pc["g"][nA:].reshape(-1, 3).copy()
    np.subtract.at(eb, rt.i, np.einsum("akc,ak->ac", pc["W"], dpa.reshape(-1, cnp)[rt.j]))
    dpb = ldl_solve(pc["Vs"], eb[:, None, :])[:, 0, :]
    if hold_b is not None:
        dpb[hold_b] = 0.0
    dp = np.concatenate([dpa, dpb.reshape(-1)])
    cams, pts = rt.current()
    newcams, newpts = cams + dpa.reshape(-1, cnp), pts + dpb
    e_new, _ = rt.residuals(newcams, newpts)
    newp = np.concatenate([newcams.reshape(-1), newpts.reshape(-1)])
    dr_, nr_ = (dp, newp) if keep is None else (dp[keep], newp[keep])
    gd = dp @ ((mu * D) * dp + pc["g"]) if gain_den is None else gain_den(dp, dr_)
    sc = dict(dp_l2=float(dr_ @ dr_), gain_den=float(gd), newp_l2=float(nr_ @ nr_),
              new_cost=float((e_new * e_new).sum()))
    return dict(S=S, ea=ea, dp=dp, newcams=newcams, newpts=newpts, sc=sc)


def plain_schur(rt, mu, point_solve=ldl_solve, rule=NO_RULE, fault=None, camera=True):
    """S [nA, nA], e_a, and the pieces in fp64 from the twin's blocks, Y = W V*^-1 by `point_solve`: V* (Vs), V, W, g,
    D (plain_damp_diag under Marquardt's rule, ones under the identity: mu D is mu exactly) and the stored diagonal dU
    of U (placeholder 1 at held coordinates).  camera=False leaves U_kk undamped, for shared_ref's fold."""
    U, ga, V, gb, W = plain_sums(rt, *rt.blocks()[:3])
    D = plain_damp_diag(rt, U, V, rule, fault) if rule.marquardt else np.ones(rt.nT)
    k = np.arange(rt.cnp)
    dU = U[:, k, k].reshape(-1)
    dU[rt.held] = 1.0
    S, ea, Vs = plain_scatter(rt, U, dU, ga, V, gb, W, mu, D, point_solve, camera)
    return S, ea, dict(Vs=Vs, V=V, W=W, g=np.concatenate([ga.reshape(-1), gb.reshape(-1)]), D=D, dU=dU)


def plain_try(rt, mu, rule=NO_RULE, fault=None):
    """One damping try in plain fp64: dp [nT] (dp_a by a Cholesky of the scaled S, dp_b by L D L^T), the proposal and
    the four sums.  Under Marquardt's rule also D; fault "backsub-identity": dp_b solved with V + mu I while Y was
    made with V + mu D (the others are plain_damp_diag's)."""
    S, ea, pc = plain_schur(rt, mu, rule=rule, fault=fault)
    dpa = plain_solve(S, ea)
    dpa[rt.held] = 0.0
    if fault == "backsub-identity":
        pc["Vs"] = pc["V"] + mu * np.eye(3)[None]
    out = plain_finish(rt, S, ea, pc, dpa, mu, pc["D"])
    return dict(out, D=pc["D"]) if rule.marquardt else out
