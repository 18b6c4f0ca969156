"""Host reference of Gaussian priors on cameras and points of the free-intrinsics routes (psba_set_priors, DESIGN 7j;
no GPU): tests/test_prior_ref.py applies it to plain fp64 evaluations and injected faults, tests/test_gpu_priors.py to
the kernels.  In the manner of held_ref.py on free_ref.py: their judges and constants are taken as they are, and no
constant is fitted to a GPU result.

Model.  A camera j may carry a mean m_j [cnp] and an information matrix L_j [cnp, cnp], a point i n_i [3] and G_i
[3, 3]; with d = m - p the cost is F = sum |e_a|^2 + sum d_j^T L_j d_j + sum d_i^T G_i d_i.  The priors are extra
residual rows R d with L = R^T R appended to the twin's blocks:
    U_j = coeff (sum A^T A + L_j),  g_a,j = coeff_g (sum A^T e + L_j d_j),  the same for V_i and g_b,i with G_i.
A held coordinate (intrinsics mask, psba_set_held) has its column deleted from the prior rows as well: row and column
of L (G) are dropped from U (V), g stays 0 there, the gradient of a free coordinate keeps the whole d, and the cost
counts the whole quadratic form.  A coordinate folded away by the groups is not held at this stage: U carries L and the
fold sums the members' rows and columns.

PriorRoute is held_ref.HeldRoute with a Priors; sums() is held_ref.sums with the prior terms added in extended
precision to U's diagonal, V, g and the cost, so that every judge of free_ref.py (damp_ref, scale_diag, dpb_residual,
scalars, solve_judge, check_exact_parts) and of held_ref.py applies unchanged.  schur_blocks IS
free_ref.schur_blocks: the route's schur_start hands it L for U, G for V and (L d)_free, (G d)_free for g to start the
sums from; plain_try is assembled from free_ref's plain_sums, plain_scatter, plain_solve and plain_finish around its own
fault switches; PriorTwin overrides HeldTwin's cost and normal equations and nothing of the loop.
The envelopes grow by the prior's own roundings, counted from the order of the kernels' sums (kernels_free.hip:
prior_row forms t_r = sum_c L_rc (m_c - p_c) from zero in ascending c, then s + t_r; an entry of U or V takes s + L_rc):
  * u |d_c| for each subtraction m_c - p_c, through |L_rc|;
  * gamma(n + 2) sum_c |L_rc| |d_c| for the product row (n = cnp, 3 for a point: n products, n additions);
  * one more rounding, u |s + t|, for the add into s (U, V: u |s_rc + L_rc|).
The prior cost q = sum_r d_r t_r of a block repeats the row and adds n products and n additions:
gamma(2 n + 6) sum_rc |d_r| |L_rc| |d_c| per block, and the blocks are that many more terms of the cost's sum."""
import numpy as np

import assembly_ref as ar
import free_ref as fr
import held_ref as hr
import shared_ref as sr
from freekd_twin import CNP

LD = ar.LD


class Priors:
    """cam_mean [nC, cnp], cam_info [nC, cnp, cnp], pt_mean [nP, 3], pt_info [nP, 3, 3]; an all-zero block = none"""

    def __init__(self, nC, cnp, nP):
        self.cam_mean, self.cam_info = np.zeros((nC, cnp)), np.zeros((nC, cnp, cnp))
        self.pt_mean, self.pt_info = np.zeros((nP, 3)), np.zeros((nP, 3, 3))

    def counts(self):
        return (int(np.any(self.cam_info != 0.0, axis=(1, 2)).sum()), int(np.any(self.pt_info != 0.0, axis=(1, 2)).sum()))

    def args(self):
        return dict(cam_mean=self.cam_mean, cam_info=self.cam_info, pt_mean=self.pt_mean, pt_info=self.pt_info)

    def copy(self):
        out = Priors(*self.cam_mean.shape, self.pt_mean.shape[0])
        for k in ("cam_mean", "cam_info", "pt_mean", "pt_info"):
            setattr(out, k, getattr(self, k).copy())
        return out


class _Prior:
    """mixin over a held route: the priors and the masks that delete held columns from the prior rows"""

    def _prior(self, pri):
        self.pri = pri
        hc = np.zeros(self.nA, dtype=bool)
        hc[self.held] = True
        self.free_c = ~hc.reshape(self.nC, self.cnp)          # (a folded-away coordinate counts as free here)
        self.free_p = ~self.held_pts

    def info_eff(self, fault=None):
        """(L with the held rows and columns dropped [nC, cnp, cnp], G with those of held points dropped).  Fault
        "held-row": the rows of held coordinates are left in (the columns dropped)."""
        f = self.free_c.astype(np.float64)
        rows = np.ones_like(f) if fault == "held-row" else f
        L = self.pri.cam_info * rows[:, :, None] * f[:, None, :]
        G = self.pri.pt_info * self.free_p.astype(np.float64)[:, None, None]
        return L, G

    def schur_start(self, dtype, fault=None):
        """what free_ref.schur_blocks adds the observations' sums to: (L, (L d)_free, G, (G d)_free)"""
        L, G = self.info_eff(fault)
        _, LdC, _, GdP = deviations(self)
        return (L.astype(dtype), np.where(self.free_c, LdC, LD(0)).astype(dtype),
                G.astype(dtype), np.where(self.free_p[:, None], GdP, LD(0)).astype(dtype))


class PriorRoute(_Prior, hr.HeldRoute):
    shared = False

    def __init__(self, p, cnp, pri, free=None, poses=None, pts=None):
        super().__init__(p, cnp, free, poses, pts)
        self._prior(pri)


class PriorSharedRoute(_Prior, hr.HeldSharedRoute):
    shared = True

    def __init__(self, p, labels, pri, free=None, kc=None, poses=None, pts=None):
        super().__init__(p, labels, free, kc, poses, pts)
        self._prior(pri)


def deviations(rt, cams=None, pts=None, sign=1.0):
    """d = m - p in extended precision at (cams [nC, cnp], pts), default the route's start: (dC, L dC, dP, G dP) with
    the FULL information matrices (the held deviations included)"""
    c0, p0 = rt.current()
    cams = c0 if cams is None else np.asarray(cams, dtype=np.float64).reshape(rt.nC, rt.cnp)
    pts = p0 if pts is None else np.asarray(pts, dtype=np.float64).reshape(rt.nP, 3)
    dC = LD(sign) * (ar.ld(rt.pri.cam_mean) - ar.ld(cams))
    dP = LD(sign) * (ar.ld(rt.pri.pt_mean) - ar.ld(pts))
    return (dC, np.einsum("jrc,jc->jr", ar.ld(rt.pri.cam_info), dC), dP, np.einsum("irc,ic->ir", ar.ld(rt.pri.pt_info), dP))


def prior_cost(rt, cams=None, pts=None):
    """the two prior sums at (cams, pts) in extended precision with their bounds: (qC, bound, qP, bound)"""
    dC, LdC, dP, GdP = deviations(rt, cams, pts)
    out = []
    for d, Ld, info, n in ((dC, LdC, rt.pri.cam_info, rt.cnp), (dP, GdP, rt.pri.pt_info, 3)):
        q = (d * Ld).sum(axis=1)
        ad = np.abs(d.astype(np.float64))
        mag = np.einsum("br,brc,bc->b", ad, np.abs(info), ad)
        nb = int(np.any(info != 0.0, axis=(1, 2)).sum())
        out += [q.sum(), float(ar.gamma(2 * n + 6) * mag.sum() + ar.gamma(nb + 12) * np.abs(q.astype(np.float64)).sum())]
    return tuple(out)


def sums(rt, coeff=1.0, coeff_g=1.0):
    """held_ref.sums with the priors: g, the diagonal of U, V, their envelopes and the cost (module docstring)"""
    sm = hr.sums(rt, coeff, coeff_g)
    nA, cnp = rt.nA, rt.cnp
    cg = abs(coeff_g)
    L, G = rt.info_eff()
    dC, LdC, dP, GdP = deviations(rt)
    fC, fP = rt.free_c, np.repeat(rt.free_p[:, None], 3, axis=1)
    # ---- g
    for lo, d, Ld, info, f, n in ((0, dC, LdC, rt.pri.cam_info, fC, cnp), (nA, dP, GdP, rt.pri.pt_info, fP, 3)):
        t = np.where(f, Ld, LD(0)).reshape(-1)
        mag = np.where(f, np.einsum("brc,bc->br", np.abs(info), np.abs(d.astype(np.float64))), 0.0).reshape(-1)
        has = mag > 0.0
        sl = slice(lo, lo + t.size)
        sm["g"][sl] += LD(coeff_g) * t
        sm["envg"][sl] += cg * (ar.U + ar.gamma(n + 2)) * mag + np.where(has, ar.U * np.abs(sm["g"][sl].astype(np.float64)), 0.0)
    # ---- the diagonal of U (what damp_ref, scale_diag and max_diag read)
    k = np.arange(cnp)
    dL = L[:, k, k].reshape(-1)
    sm["diagU"] = sm["diagU"] + coeff * dL
    sm["diagUx"] = sm["diagUx"] + LD(coeff) * ar.ld(dL)
    sm["envdU"] = sm["envdU"] + np.where(dL != 0.0, ar.U * np.abs(sm["diagUx"].astype(np.float64)), 0.0)
    # ---- V
    sm["V"] = sm["V"] + LD(coeff) * ar.ld(G)
    sm["envV"] = sm["envV"] + np.where(G != 0.0, ar.U * np.abs(sm["V"].astype(np.float64)), 0.0)
    k3 = np.arange(3)
    sm["diagV"] = sm["diagV"] + coeff * G[:, k3, k3].reshape(-1)
    sm["diagVx"] = sm["V"][:, k3, k3].reshape(-1).copy()
    sm["diagVx"][rt.held_b] = LD(coeff)
    sm["envdV"] = sm["envV"][:, k3, k3].reshape(-1).copy()
    # ---- F
    qC, bC, qP, bP = prior_cost(rt)
    sm["cost_obs"] = sm["cost"]
    sm["cost"] = float(LD(sm["cost"]) + qC + qP)
    sm["prior"] = (qC, bC, qP, bP)
    return sm


schur_blocks = fr.schur_blocks      # (the prior terms come in through the route's schur_start)


def damp_ref(rt, sm, rule=fr.NO_RULE):
    return sr.damp_ref(rt, sm, rule) if rt.shared else hr.damp_ref(rt, sm, rule)


def schur_ref(rt, sm, mu, rule=fr.NO_RULE):
    """S and e_a of the embedded system in 80-bit, rounded once (either rule; with groups: the point blocks damped, the
    fold of the undamped camera part, then mu D once on the diagonal, as held_ref.shared_schur_ref)"""
    D = damp_ref(rt, sm, rule)[0]
    if not rt.shared:
        S, ea = schur_blocks(rt, mu, D)
    else:
        S, ea = sr.fold(*schur_blocks(rt, mu, D, camera=False), rt.rep, rt.free, 0.0)
        k = np.arange(rt.nA)
        S[k, k] += LD(mu) * ar.ld(D[:rt.nA])
    return S.astype(np.float64), ea.astype(np.float64)


def scale_diag(rt, sm, mu, rule=fr.NO_RULE):
    """d [nA] of C1's scaled measure: sqrt(N_rr + mu D_r) with the priors in N (the folded diagonal with groups)"""
    D = damp_ref(rt, sm, rule)[0][:rt.nA]
    diag = rt.folded_diag(sm)[0][:rt.nA] if rt.shared else sm["diagU"]
    return np.sqrt(diag + mu * D)


def free_diag(rt, sm):
    """(the diagonal of N [nT] as stored, folded with groups; the mask of its free entries)"""
    if rt.shared:
        d, f = rt.folded_diag(sm)
        f = f.copy()
        f[rt.nA + rt.held_b] = False
        return d, f
    return np.concatenate([sm["diagU"], sm["diagV"]]), rt.free_all


def cost_judge(rt, sm, cams, pts):
    """F at (cams, pts) with its bound, and the prior parts: (F, bound, (qC, bound, qP, bound)).  The observations'
    part is free_ref.scalars' new_cost at that parameter set; the prior blocks are that many more terms of its sum."""
    sc = (sr.scalars if rt.shared else fr.scalars)(rt, sm, np.zeros(rt.nT), cams, pts, 0.0)
    x, b = sc["new_cost"]
    qC, bC, qP, bP = prior_cost(rt, cams, pts)
    nb = sum(rt.pri.counts())
    F = x + qC + qP
    return F, float(b + bC + bP + ar.gamma(nb + 12) * abs(float(F))), (qC, bC, qP, bP)


def judge(rt, sm, mu, rule, got, tol, eta_max, coeff=1.0):
    """Every quantity of one damping try against the reference: {name: found / allowed}; the exact parts are asserted
    here.  got: S, ea, dp, cams, pts, newcams, newpts, sc (dp_l2, gain_den, newp_l2, new_cost) and optionally g,
    max_diag, D, cost, prior_cur, prior_new, cost_new (psba_residual / psba_prior_cost at both sets).  tol: C1's
    scaled_tol (shared_tol with groups); eta_max: test_gpu_dense_solve.ETA_MAX."""
    nA, out = rt.nA, {}
    cost = sm["cost"]
    S, ea, dp = got["S"], got["ea"], got["dp"]
    # ---- C1
    S_want, ea_want = schur_ref(rt, sm, mu, rule)
    eS, ee = sr.scaled_errors(S, ea, S_want, ea_want, scale_diag(rt, sm, mu, rule), cost)
    out["S"], out["e_a"] = eS / tol, ee / tol
    blk = np.arange(nA) // rt.cnp
    upper = blk[:, None] < blk[None, :]
    assert np.array_equal(S[upper], S.T[upper]), "the blocks above the diagonal are not copies of those below"
    hr.check_held_system(rt, S, ea, mu, rule, coeff)
    if rt.shared:
        dh = mu * float(rule.clamp(coeff)) if rule.marquardt else mu
        sr.check_embedded(S, ea, rt.away, coeff + dh)
        sr.check_mirror(S)
    hr.check_held_step(rt, got.get("g"), dp, hr.flat(got["cams"], got["pts"]), hr.flat(got["newcams"], got["newpts"]))
    # ---- g, max diag, D
    if got.get("g") is not None:
        out["g"] = ar.excess(got["g"], sm["g"], sm["envg"])[0]
    diag, free = free_diag(rt, sm)
    if got.get("max_diag") is not None:
        want = float(diag[free].max())
        out["max_diag"] = abs(got["max_diag"] - want) / (1e-11 * want)      # (the rule of held_ref.check_max_diag)
    D = got.get("D")
    if rule.marquardt and D is not None:
        if rt.shared:
            x, env, fixed = sr.folded_damp_diag(rt, sm)
            fixed = np.union1d(fixed, rt.nA + rt.held_b).astype(np.int64)
        else:
            x, env, fixed = np.concatenate([sm["diagUx"], sm["diagVx"]]), np.concatenate([sm["envdU"], sm["envdV"]]), rt.held_all
        out["D"] = fr.check_damp_diag(D, x, env, rule, fixed, coeff)[0]
    # ---- C2
    dpa = np.asarray(dp[:nA], dtype=np.float64).copy()
    if rt.shared:
        dpa[rt.away] = 0.0                                   # (the embedded step: dp itself is expanded to every member)
    eta, fe, kappa = fr.solve_judge(S, ea, dpa)
    out["dp_a eta"], out["dp_a forward"] = eta / eta_max, fe / (2 * kappa * 1e-14)
    # ---- C3
    dpe = dp if not rt.shared else np.r_[rt.expand(dp[:nA]), dp[nA:]]
    r, bound = fr.dpb_residual(rt, sm, dpe, mu, rule)
    out["dp_b"] = ar.excess(r, np.zeros(r.shape, LD), bound)[0]
    # ---- C4
    sc = (sr.scalars if rt.shared else fr.scalars)(rt, sm, dp, got["newcams"], got["newpts"], mu, D=D if rule.marquardt else None)
    F_new, b_new, parts_new = cost_judge(rt, sm, got["newcams"], got["newpts"])
    sc["new_cost"] = (F_new, b_new)
    for what, (x, b) in sc.items():
        out[what] = float(abs(LD(got["sc"][what]) - x) / b)
    # ---- psba_residual and psba_prior_cost at both sets
    F_cur, b_cur, parts_cur = cost_judge(rt, sm, got["cams"], got["pts"])
    for key, F, b in (("cost", F_cur, b_cur), ("cost_new", F_new, b_new)):
        if got.get(key) is not None:
            out["residual " + key] = float(abs(LD(got[key]) - F) / b)
    for key, parts in (("prior_cur", parts_cur), ("prior_new", parts_new)):
        if got.get(key) is not None:
            for k, name in enumerate(("cams", "pts")):
                x, b = parts[2 * k], parts[2 * k + 1]
                err = float(abs(LD(got[key][k]) - x))
                out[f"{key} {name}"] = err / b if b > 0 else (0.0 if err == 0.0 else np.inf)
    return out


# ---- dense statements (fp64) -------------------------------------------------------------------------------------------

def dense_system(rt):
    """(N + Lambda, g + Lambda d, F) over all nT coordinates of the unheld blocks: the augmented normal equations,
    before any column is deleted"""
    N, g = hr.dense_normal(rt, rt.unheld_blocks())
    dC, LdC, dP, GdP = deviations(rt)
    nA, cnp = rt.nA, rt.cnp
    for j in range(rt.nC):
        N[cnp * j:cnp * j + cnp, cnp * j:cnp * j + cnp] += rt.pri.cam_info[j]
    for i in range(rt.nP):
        N[nA + 3 * i:nA + 3 * i + 3, nA + 3 * i:nA + 3 * i + 3] += rt.pri.pt_info[i]
    g = g + np.concatenate([LdC.reshape(-1), GdP.reshape(-1)]).astype(np.float64)
    return N, g


def augmented_jacobian(rt):
    """J with the prior rows R appended (L = R^T R by an eigendecomposition, so that a rank-deficient block serves) and
    the residual vector with R d appended"""
    e, A, B, _ = rt.unheld_blocks()
    J = np.zeros((2 * rt.nO, rt.nT))
    for a in range(rt.nO):
        J[2 * a:2 * a + 2, rt.cnp * rt.j[a]:rt.cnp * rt.j[a] + rt.cnp] = A[a]
        J[2 * a:2 * a + 2, rt.nA + 3 * rt.i[a]:rt.nA + 3 * rt.i[a] + 3] = B[a]
    dC, _, dP, _ = deviations(rt)
    rows, res = [J], [e.reshape(-1)]
    for info, d, lo, n in ((rt.pri.cam_info, dC, 0, rt.cnp), (rt.pri.pt_info, dP, rt.nA, 3)):
        for b in np.flatnonzero(np.any(info != 0.0, axis=(1, 2))):
            w, Q = np.linalg.eigh(info[b])
            R = np.sqrt(np.maximum(w, 0.0))[:, None] * Q.T
            blk = np.zeros((n, rt.nT))
            blk[:, lo + n * b:lo + n * b + n] = R
            rows.append(blk)
            res.append(R @ d[b].astype(np.float64))
    return np.vstack(rows), np.concatenate(res)


def reduced_solve(rt, mu, scaled=False):
    """the held columns deleted from the augmented system, (N_ff + mu I) x = g_f solved, scattered back with zeros"""
    N, g = dense_system(rt)
    f = rt.free_all
    Nf, gf = N[np.ix_(f, f)] + mu * np.eye(int(f.sum())), g[f]
    d = 1.0 / np.sqrt(np.diag(Nf)) if scaled else np.ones(gf.size)
    dp = np.zeros(rt.nT)
    dp[f] = d * np.linalg.solve(d[:, None] * Nf * d[None, :], d * gf)
    return dp


def total_cost(rt, cams, pts):
    """F in fp64 at (cams [nC, cnp], pts)"""
    e, _ = rt.residuals(cams, pts)
    qC, _, qP, _ = prior_cost(rt, cams, pts)
    return float((e * e).sum() + float(qC) + float(qP))


# ---- a plain fp64 evaluation with the faults the judges must reject -----------------------------------------------------

FAULTS = ("g-dropped", "sign", "held-row", "no-new-cost")


def plain_try(rt, mu, rule=fr.NO_RULE, fault=None):
    """held_ref.plain_try with the priors, from free_ref's pieces: one damping try in plain fp64 (what the kernels
    compute).  Faults: "g-dropped" (the prior kept in U and V, dropped from g), "sign" (d = p - m), "held-row" (a held
    row of L left in U), "no-new-cost" (the prior missing from the proposal's cost)."""
    e, A, B, _ = rt.blocks()
    cnp, nA = rt.cnp, rt.nA
    cams, pts = rt.current()
    L, G = rt.info_eff(fault)
    sg = -1.0 if fault == "sign" else 1.0
    dC, dP = sg * (rt.pri.cam_mean - cams), sg * (rt.pri.pt_mean - pts)
    LdC = np.where(rt.free_c, np.einsum("jrc,jc->jr", rt.pri.cam_info, dC), 0.0)
    GdP = np.where(rt.free_p[:, None], np.einsum("irc,ic->ir", rt.pri.pt_info, dP), 0.0)
    if fault == "g-dropped":
        LdC, GdP = 0.0 * LdC, 0.0 * GdP
    U, ga, V, gb, W = fr.plain_sums(rt, e, A, B, prior=(L, LdC, G, GdP))
    hq = np.flatnonzero(rt.held_pts)
    V[hq] = np.eye(3)
    gb[hq] = 0.0
    k, k3 = np.arange(cnp), np.arange(3)
    dU = U[:, k, k].reshape(-1)
    dU[rt.held] = 1.0
    diag = np.concatenate([dU, V[:, k3, k3].reshape(-1)])
    max_diag = float(diag[rt.free_all].max())
    D = rule.clamp(diag) if rule.marquardt else np.ones(rt.nT)
    if fault != "held-row":                                  # the held rows and columns of U's blocks are clear
        hj, hk = rt.held // cnp, rt.held % cnp
        U[hj, hk, :] = 0.0
        U[hj, :, hk] = 0.0
    S, ea, Vs = fr.plain_scatter(rt, U, dU, ga, V, gb, W, mu, D)
    g = np.concatenate([ga.reshape(-1), gb.reshape(-1)])
    blk = np.arange(nA) // cnp
    upper = blk[:, None] < blk[None, :]
    S[upper] = S.T[upper]                                    # (the mirror of k_free_finalize)
    dpa = fr.plain_solve(S, ea, fallback=True)               # (a faulted system need not be positive definite)
    dpa[rt.held] = 0.0
    out = fr.plain_finish(rt, S, ea, dict(Vs=Vs, W=W, g=g), dpa, mu, D, hold_b=hq)

    def quad(c, p):
        a, b = rt.pri.cam_mean - c, rt.pri.pt_mean - p
        return (float(np.einsum("jr,jrc,jc->", a, rt.pri.cam_info, a)), float(np.einsum("ir,irc,ic->", b, rt.pri.pt_info, b)))
    prior_cur, prior_new = quad(cams, pts), quad(out["newcams"], out["newpts"])
    out["sc"]["new_cost"] += 0.0 if fault == "no-new-cost" else sum(prior_new)
    return dict(out, g=g, cams=cams, pts=pts, D=D, max_diag=max_diag, cost=float((e * e).sum()) + sum(prior_cur),
                prior_cur=prior_cur, prior_new=prior_new)


def plain_shared_system(rt, mu, fault=None):
    """S and e_a with groups in plain fp64: the unfolded damped system with L in U, then shared_ref.plain_fold.  Fault
    "shared-once": only the representative's prior on a shared intrinsic is counted."""
    pri = rt.pri
    if fault == "shared-once":
        rt.pri = pri.copy()
        for j in np.flatnonzero(rt.rep != np.arange(rt.nC)):
            sh = np.flatnonzero(np.asarray(rt.free) != 0)
            rt.pri.cam_info[j][sh, :] = 0.0
            rt.pri.cam_info[j][:, sh] = 0.0
    try:
        S, ea = schur_blocks(rt, mu, np.ones(rt.nT), dtype=np.float64)   # (damped: what plain_fold takes)
    finally:
        rt.pri = pri
    S, ea = sr.plain_fold(S, ea, rt.rep, rt.free, mu)
    return S, ea


# ---- the priors of the tests, drawn with a fixed seed ---------------------------------------------------------------------

def draw_priors(rt0, seed=3, n_pts=3):
    """Priors for a route without priors rt0 (a HeldRoute or HeldSharedRoute): by camera j mod 4 a full positive
    definite block, a diagonal block, none, a rank-deficient positive semi-definite block (rank 2); a camera without
    observations gets none (its block of S stays the exact placeholder free_ref.check_exact_parts asserts).  Points:
    one seen by three cameras with a full block, then diagonal and rank-1 blocks on the first points.  The weights span
    10^-3 .. 10^3 times the diagonal of J^T J, the means lie up to three sigma off the start."""
    rng = np.random.default_rng(seed)
    sm = hr.sums(rt0)
    nC, nP, cnp = rt0.nC, rt0.nP, rt0.cnp
    pri = Priors(nC, cnp, nP)
    cams, pts = rt0.current()
    dU, dV = sm["diagU"].reshape(nC, cnp), sm["diagV"].reshape(nP, 3)
    seen = np.bincount(rt0.j, minlength=nC) > 0

    def block(diag, kind, n):
        w = np.sqrt(np.where(diag > 0.0, diag, 1.0) * 10.0 ** rng.uniform(-3.0, 3.0, n))
        if kind == "diag":
            M = np.eye(n)
        elif kind == "full":
            u = rng.standard_normal(n)
            u /= np.linalg.norm(u)
            M = 0.7 * np.eye(n) + 0.3 * n * np.outer(u, u)
        else:                                                # rank 2 (rank 1 for a point)
            a, b = rng.standard_normal(n), rng.standard_normal(n)
            M = np.outer(a, a) + (np.outer(b, b) if n > 3 else 0.0)
        info = np.outer(w, w) * M                           # (bit for bit symmetric)
        sig = 1.0 / np.sqrt(np.where(np.diag(info) > 0.0, np.diag(info), 1.0))
        return info, sig * rng.uniform(-3.0, 3.0, n)
    kinds = ("full", "diag", "none", "rank") if nC >= 4 else ("full", "rank")
    for j in range(nC):
        kind = kinds[j % len(kinds)]
        if kind != "none" and seen[j]:
            pri.cam_info[j], off = block(dU[j], kind, cnp)
            pri.cam_mean[j] = cams[j] + off
    chosen = [hr.point_with_views(rt0.p, min(3, nC))] + [i for i in range(nP) if i != hr.point_with_views(rt0.p, min(3, nC))]
    for i, kind in zip(chosen[:n_pts], ("full", "diag", "rank")):
        pri.pt_info[i], off = block(dV[i], kind, 3)
        pri.pt_mean[i] = pts[i] + off
    return pri


# ---- a dense LM with the priors: HeldTwin.levmar on the augmented normal equations ------------------------------------------

class PriorTwin(hr.HeldTwin):
    """HeldTwin (TwinKD's dense LM, lm_loop.cpp restated, on the columns that are left) whose cost is F and whose
    normal equations carry the prior rows: pri is a Priors of 16-wide camera blocks"""

    def __init__(self, prob, pri, kc=None, free=None, poses=None, pts=None):
        super().__init__(prob, kc, free, poses, pts)
        self.pri = pri

    def _quad(self, cams, pts):
        a, b = self.pri.cam_mean - cams, self.pri.pt_mean - pts
        return (float(np.einsum("jr,jrc,jc->", a, self.pri.cam_info, a)) + float(np.einsum("ir,irc,ic->", b, self.pri.pt_info, b)),
                np.concatenate([np.einsum("jrc,jc->jr", self.pri.cam_info, a).reshape(-1),
                                np.einsum("irc,ic->ir", self.pri.pt_info, b).reshape(-1)]))

    def cost(self, cams=None, pts=None):
        c = self.cams if cams is None else np.asarray(cams, dtype=np.float64).reshape(self.nC, CNP)
        q = self.pts if pts is None else np.asarray(pts, dtype=np.float64).reshape(self.nP, 3)
        return super().cost(cams, pts) + self._quad(c, q)[0]

    def normal(self):
        """(F, N + Lambda with 1 on the diagonal of masked coordinates, g + Lambda d); levmar deletes the held rows
        and columns, so a free coordinate's gradient keeps the held deviations"""
        ex, N, g = super().normal()
        q, Ld = self._quad(self.cams, self.pts)
        nA = self.nA
        for j in range(self.nC):
            N[CNP * j:CNP * j + CNP, CNP * j:CNP * j + CNP] += self.pri.cam_info[j]
        for i in range(self.nP):
            N[nA + 3 * i:nA + 3 * i + 3, nA + 3 * i:nA + 3 * i + 3] += self.pri.pt_info[i]
        held = np.flatnonzero(~self.free_a)
        N[held, held] = 1.0
        return ex + q, N, g + Ld


def ring_priors(w_f=1.0 / (0.03 * 800.0) ** 2, w_k=1.0 / 0.02 ** 2, w_rot=1.0 / 1e-3 ** 2, w_t=1.0 / 1e-3 ** 2, f_off=1e-3):
    """held_ref.held_ring (the true poses of cameras 0 and 1 written into the start) with priors in the place of the
    holds: on {f, k1, k2} of every camera about the true values (f: the true value times 1 + f_off, so that a strong
    prior and the observations disagree) and on the poses of cameras 0 and 1 about the start, which is the truth.
    Returns (start problem, start kc, Priors of 16-wide blocks)."""
    from freekd_twin import ring_problem
    start, kc0, _ = hr.held_ring()
    _, _, K, kc = ring_problem()
    pri = Priors(6, CNP, int(start["nP"]))
    pri.cam_mean[:, 0] = K[:, 0] * (1.0 + f_off)
    pri.cam_mean[:, 5:7] = kc[:, :2]
    pri.cam_info[:, 0, 0] = w_f
    pri.cam_info[:, 5, 5] = pri.cam_info[:, 6, 6] = w_k
    cams = np.asarray(start["cams"], dtype=np.float64)
    pri.cam_mean[:2, 10:] = cams[:2]
    for k in range(3):
        pri.cam_info[:2, 10 + k, 10 + k] = w_rot
        pri.cam_info[:2, 13 + k, 13 + k] = w_t
    return start, kc0, pri
