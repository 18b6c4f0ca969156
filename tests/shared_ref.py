"""Host reference of intrinsics shared between cameras on the 16-block route (psba_set_intrinsics_groups, DESIGN 7e;
no GPU): tests/test_shared_ref.py applies it to a plain fp64 evaluation and to injected faults,
tests/test_gpu_shared_intrinsics.py to the kernels.

Model.  The cameras are partitioned into groups, rep(j) is the lowest camera index of j's group, and P maps the reduced
parameters to the per-camera ones: a free intrinsic coordinate k < 10 of a member j takes the value of coordinate k of
rep(j).  J_shared = J P; the points are untouched by P, so
    S_shared = P^T (U - W (V + mu I)^-1 W^T) P + mu I,   e_a,shared = P^T e_a.
The kernels keep the full-size system ("embedded"): a folded-away coordinate -- a free intrinsic coordinate of a
non-representative -- has a zero row and column, the placeholder coeff + mu on the diagonal and e_a = 0; dp is expanded
after the solve (a member's entry is a copy of its representative's).

The reference is TwinKD with the members' K and kc set to their representative's (share_problem):
  * SharedTwin.jacobian_shared builds J P in the REDUCED numbering (folded-away columns removed), and
    SharedTwin.levmar_shared is TwinKD.levmar (lm_loop.cpp restated) on it, through the methods that loop asks for --
    formulated differently from the kernels on purpose;
  * fold(S, ea, ...) folds TwinKD.schur_blocks(mu) (80-bit) in 80-bit, embedded;
  * reduce_sums reduces free_ref.sums (g and its envelope folded; dp and the proposal with the folded-away entries
    dropped), so that assembly_ref.try_scalars, free_ref.dpb_residual (with the expanded dp_a) and free_ref.solve_judge
    apply unchanged.

Measure and tolerance of S and e_a: the scaled measure of free_ref / DESIGN 7d with the FOLDED diagonal,
|dS_rc| <= tol d_r d_c, |de_a,r| <= tol d_r sqrt(cost), d = sqrt(folded diag N + mu), and
tol = shared_tol = 64 eps (largest observation count of one GROUP + 16): the existing rule applied to the length of the
sum that is now formed.  Not fitted to a result.

The fold alone (fold_bound) is judged entry by entry against the 80-bit fold of the SAME handle's unfolded buffer M
(lower triangle; the upper must be an exact copy).  The kernels sum t_m = fl(s_m + u_m) over the n = n_r n_c source
entries (n - 1 additions) and add mu once on the diagonal (one more); the unfolded buffer holds d_m = fl(t_m + mu) on
its diagonal, so the host's term d_m - mu differs from t_m by at most u |d_m|.  Together:
|found - exact| <= gamma(n_r n_c + 2) sum |terms|, the terms being the source entries as the buffer holds them and,
on the diagonal, mu once per source entry.

Under Marquardt's damping (psba_set_damping; free_ref.Rule) the section "Marquardt's damping with groups"
below gives D of the embedded system, its envelope, the 80-bit S and e_a with mu D added once after the fold, and the
plain fp64 evaluation with its injected fault.
"""
import numpy as np

import assembly_ref as ar
import free_ref as fr
from freekd_twin import CNP, TwinKD, cholesky_solve, start_kc

LD = ar.LD
EPS = np.finfo(np.float64).eps


# ---- labels, representatives, the index maps ---------------------------------------------------------------------

def representatives(labels):
    """rep [nC]: the lowest camera index that carries the same label"""
    labels = np.asarray(labels).reshape(-1)
    first = {}
    rep = np.empty(labels.size, dtype=np.int64)
    for j, g in enumerate(labels.tolist()):
        rep[j] = first.setdefault(g, j)
    return rep


def share_problem(p, kc, labels):
    """(problem, kc) with the members' K and kc set to their representative's"""
    rep = representatives(labels)
    K = np.asarray(p["K"], dtype=np.float64).reshape(-1, 5)[rep].copy()
    return dict(p, K=K), np.asarray(kc, dtype=np.float64).reshape(-1, 5)[rep].copy()


def fold_map(rep, free):
    """(phi [nA], away [nA]): coordinate t of the camera part is summed into coordinate phi[t]; away[t]: t is a free
    intrinsic coordinate of a non-representative (folded away)"""
    rep = np.asarray(rep)
    nC = rep.size
    free = np.asarray(free).reshape(10) != 0
    k = np.tile(np.arange(CNP), nC)
    j = np.repeat(np.arange(nC), CNP)
    shared = np.r_[free, np.zeros(6, dtype=bool)][k]
    phi = np.where(shared, CNP * rep[j] + k, CNP * j + k)
    return phi, phi != np.arange(CNP * nC)


def group_obs_max(p, labels):
    rep = representatives(labels)
    return int(np.bincount(rep[np.asarray(p["jidx"])], minlength=rep.size).max())


def shared_tol(p, labels):
    """64 eps (largest observation count of one group + 16)"""
    return 64 * EPS * (group_obs_max(p, labels) + 16)


def wide_labels(nC):
    """the labelling of wide_problem(64 / 65) in the GPU tests: cameras {0, 1, 2} one group (64 + 65 + 63
    observations), 3 alone (one observation), {4, 20, 40} (the representative has no observation), 5 alone, the rest
    by j % 7"""
    lab = 1000 + np.arange(nC) % 7
    lab[[0, 1, 2]] = 0
    lab[3] = 1
    lab[[4, 20, 40]] = 2
    lab[5] = 3
    return lab


# ---- the fold (any dtype) ---------------------------------------------------------------------------------------

def fold(S, ea, rep, free, mu, coeff=1.0):
    """The embedded fold of S (damped: mu on its diagonal, as TwinKD.schur_blocks returns it) and e_a in their own
    dtype: rows, then columns summed into the representatives', mu once, folded-away coordinates cleared to
    (zero, coeff + mu, e_a = 0)."""
    dt = S.dtype.type
    phi, away = fold_map(rep, free)
    nA = phi.size
    S0 = S.copy()
    S0[np.arange(nA), np.arange(nA)] -= dt(mu)
    rows = np.zeros_like(S0)
    np.add.at(rows, phi, S0)
    out = np.zeros_like(S0)
    np.add.at(out.T, phi, rows.T)
    out[np.arange(nA), np.arange(nA)] += dt(mu)
    out[away, away] = dt(coeff) + dt(mu)
    e = np.zeros_like(ea)
    np.add.at(e, phi, ea)
    return out, e


def fold_bound(M, rep, free, mu):
    """(exact [nA, nA] 80-bit, bound [nA, nA], exact e_a, bound e_a) of the fold of an UNFOLDED reduce buffer's
    S = M[:nA, :nA] (lower triangle, mirrored) and e_a: the module docstring's gamma(n_r n_c + 2) sum |terms|"""
    phi, away = fold_map(rep, free)
    nA = phi.size
    n32 = M.shape[1]
    L = np.tril(M[:nA, :nA])
    sym = L + np.tril(L, -1).T
    S, ea = fold(ar.ld(sym), ar.ld(M[n32, :nA]), rep, free, mu)
    terms = np.abs(sym)
    terms[np.arange(nA), np.arange(nA)] += abs(mu)
    one = np.ones((nA, nA))

    def both(x):
        rows = np.zeros_like(x)
        np.add.at(rows, phi, x)
        out = np.zeros_like(x)
        np.add.at(out.T, phi, rows.T)
        return out
    mag, cnt = both(terms), both(one)
    bound = ar.gamma(cnt + 2) * mag
    aw = np.flatnonzero(away)
    bound[aw, aw] = ar.U * (1.0 + abs(mu))                  # the placeholder 1 + mu: one rounding (no source entry)
    cnt_e = np.bincount(phi, minlength=nA)
    mag_e = np.bincount(phi, weights=np.abs(M[n32, :nA]), minlength=nA)
    return S, bound, ea, ar.gamma(cnt_e + 2) * mag_e, away


# ---- structure checks of an embedded system (used on the host and on the GPU) ------------------------------------------

def check_embedded(S, ea, away, diag_value):
    """folded-away coordinates: zero off the diagonal (row and column), diag_value on it, e_a = 0"""
    idx = np.flatnonzero(away)
    off = S[idx].copy()
    off[np.arange(idx.size), idx] = 0.0
    assert np.all(off == 0.0), "a folded-away row is not clear"
    col = S[:, idx].copy()
    col[idx, np.arange(idx.size)] = 0.0
    assert np.all(col == 0.0), "a folded-away column is not clear"
    assert np.all(S[idx, idx] == diag_value), "placeholder of a folded-away coordinate"
    assert np.all(ea[idx] == 0.0), "e_a of a folded-away coordinate"


def check_mirror(S):
    assert np.array_equal(S, S.T), "the upper triangle is not an exact copy of the lower"


def scaled_errors(S, ea, S_want, ea_want, d, cost):
    return (float((np.abs(S - S_want) / np.outer(d, d)).max()),
            float((np.abs(ea - ea_want) / (d * np.sqrt(cost))).max()))


# ---- the route and its sums --------------------------------------------------------------------------------------

class SharedRoute(fr.Route):
    """free_ref.Route (16 wide) of a problem whose groups share K and kc; kc defaults to start_kc"""

    def __init__(self, p, labels, free=None, kc=None):
        self.labels = np.asarray(labels).reshape(-1)
        self.rep = representatives(self.labels)
        ps, kcs = share_problem(p, start_kc(int(p["nC"])) if kc is None else kc, self.labels)
        super().__init__(ps, 16, free)
        self.kc = kcs
        self.twin = TwinKD(ps, kcs, self.free)
        self.phi, self.away = fold_map(self.rep, self.free)
        self.keep = np.r_[~self.away, np.ones(self.nB, dtype=bool)]     # the distinct parameters among the nT
        self.tol = shared_tol(ps, self.labels)

    def expand(self, dpa):
        """the embedded dp_a (zero at folded-away coordinates) -> the per-camera step"""
        return np.asarray(dpa)[self.phi]

    def folded_diag(self, sm):
        """diag of the folded N over all nT coordinates (placeholder 1 at held and folded-away ones) and the mask of
        its free entries"""
        dU = sm["diagU"].copy()
        dU[self.held] = 0.0
        f = np.bincount(self.phi, weights=dU, minlength=self.nA)
        f[self.held] = 1.0
        f[self.away] = 1.0
        free = np.ones(self.nT, dtype=bool)
        free[self.held] = False
        free[np.flatnonzero(self.away)] = False
        return np.concatenate([f, sm["diagV"]]), free


def reduce_sums(rt, sm):
    """g and its envelope folded and restricted to the distinct parameters (for assembly_ref.try_scalars)"""
    nA = rt.nA
    g = np.zeros(nA, dtype=LD)
    np.add.at(g, rt.phi, sm["g"][:nA])
    env = np.bincount(rt.phi, weights=sm["envg"][:nA], minlength=nA)
    return np.concatenate([g, sm["g"][nA:]])[rt.keep], np.concatenate([env, sm["envg"][nA:]])[rt.keep]


def scalars(rt, sm, dp, newcams, newpts, mu, D=None):
    """free_ref.scalars on the reduced vectors: {name: (exact, bound)}.  D [nT] (embedded): Marquardt's weights; a
    folded-away coordinate contributes nothing, a shared one once with the D of its representative"""
    e_new, proj = rt.residuals(newcams, newpts)
    newp = np.concatenate([np.asarray(newcams).reshape(-1), np.asarray(newpts).reshape(-1)])
    g, envg = reduce_sums(rt, sm)
    if D is None:
        return ar.try_scalars(np.asarray(dp)[rt.keep], newp[rt.keep], mu, g, int((~rt.away).sum()),
                              (e_new * e_new).sum(axis=1), e_slack=ar.residual_slack(rt.twin.t.m, proj), envg=envg)
    return ar.try_scalars(np.asarray(dp)[rt.keep], newp[rt.keep], LD(mu) * ar.ld(np.asarray(D)[rt.keep]), g,
                          int((~rt.away).sum()), (e_new * e_new).sum(axis=1),
                          e_slack=ar.residual_slack(rt.twin.t.m, proj), envg=envg, extra=1)


# ---- Marquardt's damping with groups (psba_set_damping) ------------------------------------------------------
# D of the embedded system: at a representative's shared coordinate the clamp of the sum of its members' diagonal
# entries (k_free_damp_diag sums them in ascending camera order), clamp(coeff) at a folded-away or held coordinate,
# the points as without groups.  The envelope of the sum is the members' K1 envelopes added (free_ref.damp_ref: the
# rule of shared_tol, every observation of the group once) plus gamma(n_g - 1) of the sum for the n_g - 1 additions
# of the member sum.  mu D is added once, after the fold (k_kd_fold_finish).

def folded_damp_diag(rt, sm):
    """(the folded diagonal [nT] in extended precision with the placeholder 1 at held and folded-away coordinates,
    its envelope [nT], the indices whose entry is a placeholder)"""
    nA = rt.nA
    x = sm["diagUx"].copy()
    x[rt.held] = 0
    f = np.zeros(nA, dtype=LD)
    np.add.at(f, rt.phi, x)
    cnt = np.bincount(rt.phi, minlength=nA)
    env = (np.bincount(rt.phi, weights=sm["envdU"], minlength=nA)
           + ar.gamma(np.maximum(cnt - 1, 0)) * np.abs(f.astype(np.float64)))
    fixed = np.union1d(rt.held, np.flatnonzero(rt.away))
    f[fixed] = 1
    env[fixed] = 0.0
    return np.concatenate([f, sm["diagVx"]]), np.concatenate([env, sm["envdV"]]), fixed


def damp_ref(rt, sm, rule=fr.NO_RULE):
    """free_ref.damp_ref of the embedded system: (D [nT], envD [nT])"""
    if not rule.marquardt:
        return np.ones(rt.nT), np.zeros(rt.nT)
    x, env, fixed = folded_damp_diag(rt, sm)
    D = rule.clamp(x).astype(np.float64)
    env = env + ar.U * D
    env[fixed] = 0.0
    return D, env


def schur_ref(rt, sm, mu, rule):
    """S and e_a of the embedded system under Marquardt's rule in 80-bit, rounded once: the point blocks damped with
    mu D_i, the fold of the undamped camera part, then mu D once on the diagonal (1 + mu clamp(1) where folded away)"""
    D = damp_ref(rt, sm, rule)[0]
    S, ea = fold(*fr.schur_blocks(rt, mu, D, camera=False), rt.rep, rt.free, 0.0)
    k = np.arange(rt.nA)
    S[k, k] += LD(mu) * ar.ld(D[:rt.nA])
    return S.astype(np.float64), ea.astype(np.float64)


def plain_try_damped(rt, mu, rule, fault=None):
    """plain_try under Marquardt's rule.  fault "rep-own-diag": D of a representative from its own U_kk instead of
    the members' sum"""
    S1, ea1, pc = fr.plain_schur(rt, mu, rule=rule, camera=False)
    S, ea = plain_fold(S1, ea1, rt.rep, rt.free, 0.0)
    nA = rt.nA
    dU = pc["dU"].copy()
    own = dU.copy()
    dU[rt.held] = 0.0
    f = np.bincount(rt.phi, weights=dU, minlength=nA)
    if fault == "rep-own-diag":
        f = own
    fixed = np.union1d(rt.held, np.flatnonzero(rt.away))
    f[fixed] = 1.0
    D = np.concatenate([rule.clamp(f), pc["D"][nA:]])
    S[np.arange(nA), np.arange(nA)] += mu * D[:nA]
    return dict(_finish(rt, S, ea, pc, mu, D, lambda dp, dr_: dp @ pc["g"] + dr_ @ ((mu * D[rt.keep]) * dr_)), D=D)


# ---- a plain fp64 evaluation (what the kernels compute, in numpy) ----------------------------------------------------

def plain_fold(S, ea, rep, free, mu, coeff=1.0, mu_per_member=False, skip=None, mirror=True, clear=True):
    """The kernels' fold in fp64: from the damped S of free_ref.plain_schur (its lower triangle), a row pass and a column pass in ascending
    camera order, mu once, the mirror, the clearing.  The switches inject the faults of test_shared_ref.py:
    mu_per_member (mu counted n_g times), skip = (camera, k) left out of every sum, mirror / clear off."""
    phi, away = fold_map(rep, free)
    nA = phi.size
    k = np.arange(nA)
    S0 = np.tril(S) + np.tril(S, -1).T                      # the lower triangle is the matrix (k_kd_finalize_sym)
    if not mu_per_member:
        S0[k, k] -= mu
    src = np.ones(nA, dtype=bool)
    if skip is not None:
        src[CNP * skip[0] + skip[1]] = False
    rows = np.zeros_like(S0)
    np.add.at(rows, phi[src], S0[src])
    out = np.zeros_like(S0)
    np.add.at(out.T, phi[src], rows.T[src])
    if not mu_per_member:
        out[k, k] += mu
    e = np.zeros_like(ea)
    np.add.at(e, phi[src], ea[src])
    if clear:
        out[away, :] = 0.0
        out[:, away] = 0.0
        out[away, away] = coeff + mu
        e[away] = 0.0
    else:                                                   # the members' rows stay as they were
        out[away, :] = S[away, :]
    if mirror:
        out = np.tril(out) + np.tril(out, -1).T
    return out, e


def _finish(rt, S, ea, pc, mu, D, gain_den):
    """free_ref's solve and finish on the folded system: the embedded step cleared at held and folded-away
    coordinates and expanded, the sums over the distinct parameters"""
    dpe = fr.plain_solve(S, ea)
    dpe[rt.held] = 0.0
    dpe[rt.away] = 0.0
    out = fr.plain_finish(rt, S, ea, pc, rt.expand(dpe), mu, D, keep=rt.keep, gain_den=gain_den)
    return dict(out, dp_embedded=dpe)


def plain_try(rt, mu):
    """free_ref.plain_try with the fold: dp [nT] expanded, the proposal, the four sums over the distinct parameters"""
    S1, ea1, pc = fr.plain_schur(rt, mu)
    S, ea = plain_fold(S1, ea1, rt.rep, rt.free, mu)
    return _finish(rt, S, ea, pc, mu, pc["D"], lambda dp, dr_: dp @ pc["g"] + mu * (dr_ @ dr_))


# ---- the dense twin in the reduced numbering ------------------------------------------------------------------------

class SharedTwin(TwinKD):
    """TwinKD of the shared problem with J P, the normal equations and the LM in the REDUCED numbering: the
    folded-away columns do not exist there."""

    def __init__(self, p, labels, kc=None, free=None):
        self.rep = representatives(labels)
        ps, kcs = share_problem(p, np.zeros((int(p["nC"]), 5)) if kc is None else kc, labels)
        super().__init__(ps, kcs, free)
        self.phi, self.away = fold_map(self.rep, self.free)
        self.keep = np.r_[~self.away, np.ones(self.nB, dtype=bool)]
        self.col = np.cumsum(self.keep) - 1                 # full coordinate -> reduced column (where kept)
        self.free_r = np.r_[self.free_a, np.ones(self.nB, dtype=bool)][self.keep]

    def jacobian_shared(self):
        """(e, J P [2 nO, nR]): a shared column is the sum of its members' columns"""
        e, J = self.jacobian()
        JP = np.zeros((J.shape[0], int(self.keep.sum())))
        src = np.r_[self.phi, self.nA + np.arange(self.nB)]
        for t in range(self.nT):
            JP[:, self.col[src[t]]] += J[:, t]
        return e, JP

    def normal_shared(self):
        e, JP = self.jacobian_shared()
        N = JP.T @ JP
        held = np.flatnonzero(~self.free_r)
        N[held, held] = 1.0
        return float((e * e).sum()), N, JP.T @ e.reshape(-1)

    def max_diag_shared(self, N):
        d = np.diag(N).copy()
        d[~self.free_r] = 0.0
        return float(d.max())

    def embed(self, N, g, placeholder=1.0):
        """the reduced N, g in the full numbering: folded-away coordinates decoupled, the placeholder on the diagonal"""
        idx = np.flatnonzero(self.keep)
        Nf = np.zeros((self.nT, self.nT))
        Nf[np.ix_(idx, idx)] = N
        aw = np.flatnonzero(self.away)
        Nf[aw, aw] = placeholder
        gf = np.zeros(self.nT)
        gf[idx] = g
        return Nf, gf

    def expand(self, dp_r):
        """reduced step -> (dp cams [nC, 16], dp pts [nP, 3])"""
        src = np.r_[self.phi, self.nA + np.arange(self.nB)]
        full = np.asarray(dp_r)[self.col[src]]
        return full[:self.nA].reshape(self.nC, CNP), full[self.nA:].reshape(self.nP, 3)

    # TwinKD.levmar in the reduced numbering: N, g, D and dp have one entry per distinct parameter
    system = normal_shared

    def start_mu(self, tau, N):
        return tau * self.max_diag_shared(N)

    def solve_step(self, N, g, mu, D):
        dp = cholesky_solve(N + mu * np.diag(D), g)
        if dp is not None:
            dp[~self.free_r] = 0.0
        return dp

    def proposal(self, dp):
        dc, dq = self.expand(dp)
        return self.cams + dc, self.pts + dq

    def norm2(self, cams, pts):
        pr = np.r_[cams.reshape(-1), pts.reshape(-1)][self.keep]
        return float(pr @ pr)

    def levmar_shared(self, max_iter=20, init_mu=0.0, stop_small=True):
        """TwinKD.levmar (lm_loop.cpp restated) on the reduced system: dp_l2, the gain denominator and newp_l2 count
        every distinct parameter once"""
        return self.levmar(max_iter, init_mu, stop_small)


def shared_ring(labels, seed=7):
    """ring_problem's scene (the same draws in the same order) with the true K and kc shared by the groups: members
    take the representative's draw; exact projections of that truth; the start is ring_problem's (fu x 1.03, kc = 0,
    its perturbed poses and points).  Returns (start, kc0, K_true, kc_true); with every camera alone it is
    ring_problem itself."""
    import lens_twin
    from freekd_twin import _rot_to_quat
    rep = representatives(labels)
    rng = np.random.default_rng(seed)
    nC, nP = 6, 120
    assert rep.size == nC
    pts = rng.uniform(-1.0, 1.0, (nP, 3))
    q0, t = np.zeros((nC, 4)), np.zeros((nC, 3))
    for j in range(nC):
        th = 2.0 * np.pi * j / nC
        centre = 5.0 * np.array([np.cos(th), 0.0, np.sin(th)])
        z = -centre / np.linalg.norm(centre)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        q0[j] = _rot_to_quat(R)
        t[j] = -R @ centre
    K = np.zeros((nC, 5))
    K[:, 0] = 800.0 * (1.0 + 0.05 * rng.standard_normal(nC))
    K[:, 3] = 1.0
    kc = np.array([-0.05, 0.01, 0.0, 0.0, 0.0]) * (1.0 + 0.2 * rng.standard_normal((nC, 5)))
    K, kc = K[rep].copy(), kc[rep].copy()
    keep = rng.uniform(size=(nP, nC)) >= 0.3
    keep[:, :2] = True
    iidx, jidx = np.nonzero(keep)
    cams = np.hstack([np.zeros((nC, 3)), t])
    true = dict(K=K, initrot=q0, cams=cams, pts=pts, impts=np.zeros((iidx.size, 2)), iidx=iidx.astype(np.int32),
                jidx=jidx.astype(np.int32), nC=nC, nP=nP, nO=int(iidx.size))
    impts = lens_twin.Twin(true, kc).project()
    Ks = K.copy()
    Ks[:, 0] *= 1.03
    cs = cams.copy()
    cs[:, :3] += 0.005 * rng.standard_normal((nC, 3))
    cs[:, 3:] += 0.02 * rng.standard_normal((nC, 3))
    start = dict(true, K=Ks, cams=cs, pts=pts + 0.02 * rng.standard_normal((nP, 3)), impts=impts)
    return start, np.zeros((nC, 5)), K, kc


def dampings(rt, sm):
    """(mu = 1e-3 max over the free entries of the folded diagonal, mu = 1e-6 median diag N of the per-camera
    system, as test_gpu_free_entrywise.py takes it) and the folded diagonal"""
    fdiag, free = rt.folded_diag(sm)
    return {"big": 1e-3 * float(fdiag[free].max()),
            "small": 1e-6 * float(np.median(np.concatenate([sm["diagU"], sm["diagV"]])))}, fdiag
