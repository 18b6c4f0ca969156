"""Host reference of the observation weighting on the free-intrinsics routes (psba_set_obs_weighting; no
GPU): tests/test_weight_ref.py applies it to plain fp64 evaluations and injected faults, tests/test_gpu_weighting.py to
the kernels.  In the manner of prior_ref.py on held_ref.py on free_ref.py: their judges, constants, scaled_tol and
ETA_MAX are taken as they are, and no constant is fitted to a GPU result.  Nothing of their arithmetic is repeated here:
the Schur restatement is free_ref.schur_blocks and the plain try prior_ref.plain_try, both on the weighted blocks, and
WeightTwin overrides HeldTwin's cost and Jacobian and nothing of TwinKD's LM loop.

Model.  Observation a may carry a standard deviation sigma_a > 0 (none: 1) and a loss (kind, c) may be set, the kinds
and formulas of camera_model.h's robust_eval (assembly_ref.rho_ext).  With e_a the route's residual,
    s_a = |e_a / sigma_a|^2,   F = sum_a rho(s_a) + the priors' two sums,   omega_a = sqrt(rho'(s_a)),
and the kernel multiplies e, A and B first by 1 / sigma_a (the fp64 reciprocal the setter stores: isig below) and then
by omega_a.  Everything behind the blocks is unchanged.

WeightRoute is prior_ref.PriorRoute whose blocks() are the twin's fp64 e, A, B multiplied by isig and by omega in
extended precision and rounded once; WeightSharedRoute the same on PriorSharedRoute.  prior_ref's sums, schur_ref,
damp_ref, scale_diag, judge and plain_try then run on the weighted blocks.  What is new in the bounds:
  * Two more roundings per entry of e, A, B for the two multiplications, and one for the reference's own rounding of
    the product: gamma(3) relative, added to the relative slack of every entry.
  * The weight moves with the residual it is taken from.  The kernel's e and the twin's differ by
    es = assembly_ref.residual_slack, so e / sigma by es / sigma, and per observation
    assembly_ref.robust_jac_slack(es / sigma, c) = JACOBIAN_SLACK + |es / sigma|_2 / c replaces the bare JACOBIAN_SLACK
    in the slacks of A and B (free_ref's rule: times the largest entry of the parameter group).  The weighted residual
    omega(r) q, q = e / sigma, r = |q|, moves by omega dq + q d omega: omega es / sigma per component plus the same
    relative term times |omega q|.
    free_ref.sums forms its envelopes from the slacks JACOBIAN_SLACK gmax|A|, JACOBIAN_SLACK max|B| and
    residual_slack(m, proj); sums() below adds the difference of those same slack terms (_slack_parts restates them)
    between the slacks above and the ones free_ref.sums used.
  * Costs: assembly_ref.try_scalars(..., loss=(kind, c)) on s_a of the twin's residuals, its gamma(2) s + gamma(8)
    rho_abs per observation plus the residual slack divided by sigma; the priors' part as prior_ref.cost_judge has it.
  * psba_get_obs_weights: s against the twin's s within gamma(4) s + 2 sqrt(2 s) es / sigma + 2 (es / sigma)^2 (two
    products, one add, the scaling; the slack as try_scalars takes it); w against omega / sigma in extended precision
    within gamma(8) w + w |dr| / c, |dr| the 2-norm of es / sigma (robust_eval's at most six roundings, the product
    with isig, the reference's own)."""
import contextlib

import numpy as np

import assembly_ref as ar
import free_ref as fr
import held_ref as hr
import prior_ref as pr

LD = ar.LD
NONE, HUBER, CAUCHY, SOFT_L1 = 0, 1, 2, 3   # PSBA_LOSS_*
BLOCK_FAULTS = ("B-unweighted", "omega-unwhitened", "rho-prime", "sigma-twice")
FAULTS = BLOCK_FAULTS + ("cost-s", "prior-weighted", "ahead-current")


def omega_ext(s, kind, c):
    """omega = sqrt(rho'(s)) of camera_model.h's robust_eval in extended precision"""
    sL = ar.ld(s)
    cL, c2 = LD(c), LD(c) * LD(c)
    if kind == HUBER:
        return np.where(sL <= c2, LD(1), np.sqrt(cL / np.sqrt(np.where(sL > 0, sL, LD(1)))))
    if kind == CAUCHY:
        return 1 / np.sqrt(1 + sL / c2)
    if kind == SOFT_L1:
        return 1 / np.sqrt(np.sqrt(1 + sL / c2))
    return np.ones(sL.shape, LD)


def robust_eval64(s, kind, c):
    """(rho, omega) of robust_eval in plain fp64 numpy, its own text"""
    s = np.asarray(s, dtype=np.float64)
    c2, ic2 = c * c, 1.0 / (c * c)
    if kind == HUBER:
        r = np.sqrt(s)
        inside = s <= c2
        with np.errstate(divide="ignore"):
            return np.where(inside, s, 2.0 * c * r - c2), np.where(inside, 1.0, np.sqrt(c / np.where(inside, 1.0, r)))
    if kind == CAUCHY:
        return c2 * np.log1p(s * ic2), 1.0 / np.sqrt(1.0 + s * ic2)
    if kind == SOFT_L1:
        r = np.sqrt(1.0 + s * ic2)
        return 2.0 * s / (r + 1.0), 1.0 / np.sqrt(r)
    return s.copy(), np.ones(s.shape)


class _Weighted:
    """mixin over a prior route: the loss, sigma [nO] (None: ones) and the weighted blocks"""
    _fault = None          # a fault of BLOCK_FAULTS for test_weight_ref.py (set by plain_try)
    _weights_from = None   # fp64 residuals [nO, 2] the weights are taken from in the place of the blocks' own

    def _weigh(self, kind, c, sigma):
        self.kind, self.c = int(kind), float(c)
        self.has_sigma = sigma is not None
        self.sigma = np.ones(self.nO) if sigma is None else np.asarray(sigma, dtype=np.float64).reshape(self.nO).copy()
        self.isig = 1.0 / self.sigma                         # what the setter stores
        self.weighted = self.kind != NONE or self.has_sigma

    @property
    def loss(self):
        return self.kind, self.c

    def s_omega(self, e, fault=None):
        """(s [nO], omega [nO]) of fp64 residuals e [nO, 2] in extended precision"""
        q = ar.ld(e) * ar.ld(self.isig)[:, None]
        s = (q * q).sum(axis=1)
        om = omega_ext((ar.ld(e) ** 2).sum(axis=1) if fault == "omega-unwhitened" else s, self.kind, self.c)
        return s, om * om if fault == "rho-prime" else om

    def _apply(self, e, A, B, proj, fault=None):
        _, om = self.s_omega(e if self._weights_from is None else self._weights_from, fault)
        isg = ar.ld(self.isig)
        w = om * (isg * isg if fault == "sigma-twice" else isg)
        wB = np.ones(w.shape, LD) if fault == "B-unweighted" else w
        return ((ar.ld(e) * w[:, None]).astype(np.float64), (ar.ld(A) * w[:, None, None]).astype(np.float64),
                (ar.ld(B) * wB[:, None, None]).astype(np.float64), proj)

    def blocks(self, fault=None):
        """the held route's blocks times 1 / sigma and omega, rounded once; proj stays the projection"""
        return self._apply(*super().blocks(), fault=self._fault if fault is None else fault)

    def unheld_blocks(self):
        return self._apply(*super().unheld_blocks())

    def raw_residuals(self):
        """the twin's fp64 residuals and projections at its current parameters"""
        e, _, _, proj = super().blocks()
        return e, proj


class WeightRoute(_Weighted, pr.PriorRoute):
    def __init__(self, p, cnp, pri, loss=(NONE, 1.0), sigma=None, free=None, poses=None, pts=None):
        super().__init__(p, cnp, pri, free, poses, pts)
        self._weigh(loss[0], loss[1], sigma)


class WeightSharedRoute(_Weighted, pr.PriorSharedRoute):
    def __init__(self, p, labels, pri, loss=(NONE, 1.0), sigma=None, free=None, kc=None, poses=None, pts=None):
        super().__init__(p, labels, pri, free, kc, poses, pts)
        self._weigh(loss[0], loss[1], sigma)


@contextlib.contextmanager
def moved(rt, cams, pts):
    """the route with its twin at (cams [nC, cnp], pts): blocks(), sums() and the priors' deviations are taken there"""
    t = rt.twin
    keep = t.cams, t.pts
    t.cams, t.pts = rt.cams16(cams).copy(), np.asarray(pts, dtype=np.float64).reshape(rt.nP, 3).copy()
    t._set(None, None)
    try:
        yield rt
    finally:
        t.cams, t.pts = keep
        t._set(None, None)


def draw_weighting(rt0, kind, seed=5):
    """(sigma [nO], c) for a route rt0 of any kind: sigma log-uniform in [0.5, 2] from a seeded generator,
    c = sqrt(median of the twin's s) with those sigmas, so that about half of the observations lie on each side of c^2
    (asserted: at least a quarter on each)"""
    rng = np.random.default_rng(seed)
    sigma = np.exp(rng.uniform(np.log(0.5), np.log(2.0), rt0.nO))
    e = fr.Route.blocks(rt0)[0]
    s = ((e / sigma[:, None]) ** 2).sum(axis=1)
    c = float(np.sqrt(np.median(s)))
    lo, hi = int((s < c * c).sum()), int((s > c * c).sum())
    assert 4 * lo >= rt0.nO and 4 * hi >= rt0.nO, (lo, hi, rt0.nO)
    return sigma, c


# ---- the sums with the weighting's slacks ------------------------------------------------------------------------------

def _slack_parts(aA, aB, ae, sA, sB, es, i, j, nC, nP):
    """the slack terms of free_ref.sums' envelopes (its docstring) for slacks sA, sB, es: (W, V, g, diag U)"""
    W = np.einsum("ark,arc->akc", sA, aB + sB) + np.einsum("ark,arc->akc", aA, sB)
    V, _ = ar._segsum(np.einsum("ari,ark->aik", sB, 2 * aB + sB), i, nP)
    gb, _ = ar._segsum(np.einsum("ari,ar->ai", sB, ae + es) + np.einsum("ari,ar->ai", aB, es), i, nP)
    ga, _ = ar._segsum(np.einsum("ari,ar->ai", sA, ae + es) + np.einsum("ari,ar->ai", aA, es), j, nC)
    dU, _ = ar._segsum((sA * (2 * aA + sA)).sum(axis=1), j, nC)
    return W, V, np.concatenate([ga.reshape(-1), gb.reshape(-1)]), dU.reshape(-1)


def slacks(rt):
    """(sA, sB, es, the slacks free_ref.sums used) of the weighted blocks (module docstring)"""
    e, A, B, proj = rt.blocks()
    e_raw, _ = rt.raw_residuals()
    old = (fr.group_slack(A, fr.GROUPS[rt.cnp]), fr.group_slack(B, (slice(0, 3),)), ar.residual_slack(rt.twin.t.m, proj))
    esw = old[2] * rt.isig[:, None]                          # the slack of e / sigma
    rel = ar.gamma(3) + (ar.robust_jac_slack(esw, rt.c) - ar.JACOBIAN_SLACK if rt.kind != NONE else 0.0) * np.ones(rt.nO)
    k = 1.0 + rel / ar.JACOBIAN_SLACK
    _, om = rt.s_omega(e_raw)
    es = om.astype(np.float64)[:, None] * esw + rel[:, None] * np.abs(e)
    return old[0] * k[:, None, None], old[1] * k[:, None, None], es, old


def sums(rt, coeff=1.0, coeff_g=1.0):
    """prior_ref.sums on the weighted blocks, its envelopes with the weighting's slacks in the place of free_ref's, and
    the cost F = sum rho(s) + the priors' sums in extended precision.  Also the weighted B and e with their slacks
    (psba_get_free_obs_blocks) and s, omega / sigma of the start."""
    sm = pr.sums(rt, coeff, coeff_g)
    e, A, B, _ = rt.blocks()
    e_raw, _ = rt.raw_residuals()
    s, om = rt.s_omega(e_raw)
    if rt.weighted:
        sA, sB, es, old = slacks(rt)
        aA, aB, ae = np.abs(A), np.abs(B), np.abs(e)
        new = _slack_parts(aA, aB, ae, sA, sB, es, rt.i, rt.j, rt.nC, rt.nP)
        was = _slack_parts(aA, aB, ae, *old, rt.i, rt.j, rt.nC, rt.nP)
        c, cg = abs(coeff), abs(coeff_g)
        sm["envW"] = sm["envW"] + c * (new[0] - was[0])
        sm["envV"] = sm["envV"] + c * (new[1] - was[1])
        sm["envg"] = sm["envg"] + cg * (new[2] - was[2])
        sm["envdU"] = sm["envdU"] + c * (new[3] - was[3])
        sm["envdU"][rt.held] = 0.0
        k3 = np.arange(3)
        sm["envdV"] = sm["envdV"] + c * (new[1] - was[1])[:, k3, k3].reshape(-1)
        sm["envg"][rt.nA + rt.held_b] = 0.0
        sm["envdV"][rt.held_b] = 0.0
    else:
        sB, es = fr.group_slack(B, (slice(0, 3),)), ar.residual_slack(rt.twin.t.m, rt.twin.t.m - e_raw)
    qC, _, qP, _ = sm["prior"]
    sm["cost_obs"] = float(ar.rho_ext(s.astype(np.float64), *rt.loss)[0].sum())
    sm["cost"] = float(LD(sm["cost_obs"]) + qC + qP)
    sm.update(Bw=B, ew=e, sB=sB, es=es, s=s, w=om * ar.ld(rt.isig))
    return sm


# ---- the judges ---------------------------------------------------------------------------------------------------------

def cost_judge(rt, sm, cams, pts):
    """F = sum rho(s) + the priors' sums at (cams, pts) with its bound: (F, bound)"""
    e, proj = rt.residuals(cams, pts)
    q = e * rt.isig[:, None]
    es = ar.residual_slack(rt.twin.t.m, proj) * rt.isig[:, None]
    x, b = ar.try_scalars(np.zeros(rt.nT), np.zeros(rt.nT), 0.0, sm["g"], rt.nA, (q * q).sum(axis=1), e_slack=es,
                          loss=rt.loss)["new_cost"]
    qC, bC, qP, bP = pr.prior_cost(rt, cams, pts)
    nb = sum(rt.pri.counts())
    F = x + qC + qP
    return F, float(b + bC + bP + ar.gamma(nb + 12) * abs(float(F)))


def weights_judge(rt, cams, pts, s_got, w_got):
    """psba_get_obs_weights at (cams, pts): (worst found / allowed of s, of w)"""
    e, proj = rt.residuals(cams, pts)
    s, om = rt.s_omega(e)
    esw = ar.residual_slack(rt.twin.t.m, proj) * rt.isig[:, None]
    sd = s.astype(np.float64)
    es1 = esw.max(axis=1)
    bs = ar.gamma(4) * sd + 2 * np.sqrt(2 * sd) * es1 + 2 * es1 * es1
    w = om * ar.ld(rt.isig)
    wd = w.astype(np.float64)
    bw = ar.gamma(8) * wd + (wd * np.sqrt((esw * esw).sum(axis=1)) / rt.c if rt.kind != NONE else 0.0)
    return ar.excess(s_got, s, bs)[0], ar.excess(w_got, w, bw)[0]


def blocks_judge(rt, sm, W, B, e):
    """psba_get_free_obs_blocks against the weighted blocks: {W, B, e: found / allowed}"""
    return {"W": ar.excess(W, sm["W"], sm["envW"])[0], "B": ar.excess(B, ar.ld(sm["Bw"]), sm["sB"])[0],
            "e": ar.excess(e, ar.ld(sm["ew"]), sm["es"])[0]}


def judge(rt, sm, mu, rule, got, tol, eta_max, coeff=1.0):
    """prior_ref.judge on the weighted blocks, with the costs judged as F = sum rho(s) + priors (new_cost of the try,
    psba_residual at both sets), psba_get_obs_weights at both sets (got: w_cur, w_new = (s, w)) and, when given, the
    gradient of the look-ahead linearization (got: g_ahead, taken at the proposal)."""
    out = pr.judge(rt, sm, mu, rule, got, tol, eta_max, coeff)
    F_new, b_new = cost_judge(rt, sm, got["newcams"], got["newpts"])
    out["new_cost"] = float(abs(LD(got["sc"]["new_cost"]) - F_new) / b_new)
    F_cur, b_cur = cost_judge(rt, sm, got["cams"], got["pts"])
    for key, F, b in (("cost", F_cur, b_cur), ("cost_new", F_new, b_new)):
        if got.get(key) is not None:
            out["residual " + key] = float(abs(LD(got[key]) - F) / b)
    for key, cams, pts in (("w_cur", got["cams"], got["pts"]), ("w_new", got["newcams"], got["newpts"])):
        if got.get(key) is not None:
            out[f"{key} s"], out[f"{key} w"] = weights_judge(rt, cams, pts, *got[key])
    if got.get("g_ahead") is not None:
        with moved(rt, got["newcams"], got["newpts"]):
            sm2 = sums(rt, coeff)
        out["g ahead"] = ar.excess(got["g_ahead"], sm2["g"], sm2["envg"])[0]
    return out


# ---- dense statements (fp64) --------------------------------------------------------------------------------------------

def total_cost(rt, cams, pts):
    """F in fp64 at (cams [nC, cnp], pts)"""
    e, _ = rt.residuals(cams, pts)
    q = e * rt.isig[:, None]
    qC, _, qP, _ = pr.prior_cost(rt, cams, pts)
    return float(robust_eval64((q * q).sum(axis=1), *rt.loss)[0].sum() + float(qC) + float(qP))


# ---- a plain fp64 evaluation with the faults the judges must reject -----------------------------------------------------

def plain_weights(rt, cams, pts):
    """(s, w, rho) in plain fp64 at (cams, pts): what k_free_obs_weights and the cost kernels compute"""
    e, _ = rt.residuals(cams, pts)
    q = e * rt.isig[:, None]
    s = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]
    rho, om = robust_eval64(s, *rt.loss)
    return s, om * rt.isig, rho


def plain_try(rt, mu, rule=fr.NO_RULE, fault=None):
    """prior_ref.plain_try on the weighted blocks with the costs, the weights at both sets and the gradient of the
    look-ahead linearization.  Faults: "B-unweighted", "omega-unwhitened" (omega from |e|^2), "rho-prime" (rho' in the
    place of its root), "sigma-twice" (1 / sigma applied twice), "cost-s" (the costs sum s), "prior-weighted" (the
    priors' sums through rho), "ahead-current" (the look-ahead set weighted with the current parameters' omega)."""
    rt._fault = fault if fault in BLOCK_FAULTS else None
    try:
        got = pr.plain_try(rt, mu, rule)
        prior = {"cur": got["prior_cur"], "new": got["prior_new"]}

        def F(cams, pts, which):
            s, w, rho = plain_weights(rt, cams, pts)
            q = prior[which]
            if fault == "prior-weighted":
                q = tuple(float(v) for v in robust_eval64(np.asarray(q), *rt.loss)[0])
            return float((s if fault == "cost-s" else rho).sum()) + sum(q), (s, w)
        got["cost"], got["w_cur"] = F(got["cams"], got["pts"], "cur")
        got["cost_new"], got["w_new"] = F(got["newcams"], got["newpts"], "new")
        got["sc"]["new_cost"] = got["cost_new"]
        e_cur, _ = rt.raw_residuals()
        with moved(rt, got["newcams"], got["newpts"]):
            rt._weights_from = e_cur if fault == "ahead-current" else None
            got["g_ahead"] = pr.plain_try(rt, mu, rule)["g"]
    finally:
        rt._fault = rt._weights_from = None
    return got


# ---- a dense LM with the weighting: HeldTwin.levmar on the IRLS normal equations -------------------------------------------

class WeightTwin(hr.HeldTwin):
    """HeldTwin (TwinKD's dense LM, lm_loop.cpp restated, on the columns that are left) whose cost is sum rho(s) and
    whose Jacobian rows and residuals are multiplied by omega / sigma"""

    def __init__(self, prob, loss=(NONE, 1.0), sigma=None, kc=None, free=None, poses=None, pts=None):
        super().__init__(prob, kc, free, poses, pts)
        self.loss = (int(loss[0]), float(loss[1]))
        self.isig = np.ones(self.nO) if sigma is None else 1.0 / np.asarray(sigma, dtype=np.float64).reshape(self.nO)

    def s(self, cams=None, pts=None):
        q = self.residual(cams, pts) * self.isig[:, None]
        self._set(None, None)
        return (q * q).sum(axis=1)

    def cost(self, cams=None, pts=None):
        return float(robust_eval64(self.s(cams, pts), *self.loss)[0].sum())

    def jacobian(self, masked=True):
        e, J = super().jacobian(masked)
        q = e * self.isig[:, None]
        w = robust_eval64((q * q).sum(axis=1), *self.loss)[1] * self.isig
        return e * w[:, None], J * np.repeat(w, 2)[:, None]

    def normal(self):
        _, N, g = super().normal()
        return self.cost(), N, g


def contaminated_ring(n_bad=45, seed=3):
    """held_ref.held_ring with n_bad observations moved by 20 to 50 pixels in a random direction: each belongs to a
    different point and none to camera 0 or 1.  Returns (start problem, start kc, held pose flags, the moved set)."""
    start, kc0, poses = hr.held_ring()
    rng = np.random.default_rng(seed)
    i, j = np.asarray(start["iidx"]), np.asarray(start["jidx"])
    bad = []
    for pt in rng.permutation(int(start["nP"])):
        obs = np.flatnonzero((i == pt) & (j > 1))
        if obs.size and len(bad) < n_bad:
            bad.append(int(rng.choice(obs)))
    bad = np.sort(np.asarray(bad))
    assert bad.size == n_bad
    m = np.array(start["impts"], dtype=np.float64).reshape(-1, 2)
    ang, r = rng.uniform(0.0, 2.0 * np.pi, n_bad), rng.uniform(20.0, 50.0, n_bad)
    m[bad] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    return dict(start, impts=m.reshape(np.shape(start["impts"]))), kc0, poses, bad
