"""Robust losses on the GPU (psba_set_robust_loss, psba_obs_sq_residuals): the error codes and state rules, the
neutral settings against the plain handle, one damping try on every K1 / K3 route against the numpy twin
(tests/robust_twin.py), the gradient against central differences of psba_residual, recovery from outliers, the
solvers, a sharded rank layout and J x.  Needs an MI355X."""
import os

import numpy as np
import pytest

import psba_amd
from psba_amd import capi, synth
from lens_twin import Twin
from robust_twin import KINDS, RobustTwin, robust_pieces
from sba_text import KK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
C = 2.0  # loss scale of the tests (whitened pixels)


def close(got, want, tol, what=""):
    got, want = np.asarray(got), np.asarray(want)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= tol * scale, f"{what}: max|diff|={err:.3e} scale={scale:.3e} rel={err / scale:.3e}"


def _spd(rng, n):
    G = rng.normal(size=(n, 2, 2))
    return G @ np.transpose(G, (0, 2, 1)) + 0.5 * np.eye(2)[None]


def _kc(rng, nC, k1=0.4):
    return np.column_stack([k1 * (1 + 0.1 * rng.normal(size=nC)), -0.3 * (1 + 0.1 * rng.normal(size=nC)),
                            2e-3 * rng.normal(size=nC), 2e-3 * rng.normal(size=nC), 0.2 * rng.normal(size=nC)])


def _prob54():
    return psba_amd.read_problem(os.path.join(DATA, "54cams.txt"), os.path.join(DATA, "54pts.txt"), KK)


def _outliers54(seed=1):
    return synth.add_outliers(_prob54(), 0.05, 20.0, 80.0, seed)


def _lens_outlier_problem(prob, rng, kc_scale=1.0, seed=2):
    """prob's geometry with kc per camera, random SPD covariances, observations re-projected through the lens model
    with ~1 px of noise, then 5 % of them moved by 20-80 px"""
    kc = _kc(rng, prob["nC"]) * kc_scale
    cov = _spd(rng, prob["nO"])
    p = capi.Problem(prob, impts=Twin(prob, kc).project() + rng.normal(size=(prob["nO"], 2)))
    p, idx = synth.add_outliers(p, 0.05, 20.0, 80.0, seed)
    return p, kc, cov


def _handle(prob, kind=None, c=C, kc=None, cov=None, solver=None):
    h = psba_amd.Psba(0)
    if solver is not None:
        h.set_solver(solver, tol=1e-12, max_iter=4000)
    h.upload_problem(prob)
    if kc is not None:
        h.set_distortion(kc)
    if cov is not None:
        h.set_obs_covariance(cov)
    if kind is not None:
        h.set_robust_loss(kind, c)
    return h


def test_errors_and_state_rules():
    prob = _prob54()
    h = psba_amd.Psba(0)
    with pytest.raises(capi.PsbaError) as ei:  # before upload
        h._ck(capi.lib.psba_set_robust_loss(h._h, psba_amd.LOSS_HUBER, 1.0))
    assert ei.value.code == -6
    h.upload_problem(prob)
    assert h.robust_loss() == (psba_amd.LOSS_NONE, 1.0)
    for kind, scale in [(4, 1.0), (-1, 1.0), (psba_amd.LOSS_HUBER, 0.0), (psba_amd.LOSS_CAUCHY, -2.0),
                        (psba_amd.LOSS_SOFT_L1, float("inf")), (psba_amd.LOSS_HUBER, float("nan"))]:
        with pytest.raises(capi.PsbaError) as ei:
            h.set_robust_loss(kind, scale)
        assert ei.value.code == -1, (kind, scale)
    assert h.robust_loss() == (psba_amd.LOSS_NONE, 1.0)  # a refused call changes nothing
    for kind in (psba_amd.LOSS_HUBER, psba_amd.LOSS_CAUCHY, psba_amd.LOSS_SOFT_L1, psba_amd.LOSS_NONE):
        h.set_robust_loss(kind, 3.5)
        assert h.robust_loss() == (kind, 3.5)
    h.set_robust_loss(psba_amd.LOSS_CAUCHY, 2.5)
    assert h.lens_model() == (False, False)  # the loss is not a lens model bit of the C ABI
    with pytest.raises(capi.PsbaError) as ei:
        h.obs_sq_residuals(7)
    assert ei.value.code == -1
    h.upload_problem(prob)  # a new upload resets the loss
    assert h.robust_loss() == (psba_amd.LOSS_NONE, 1.0)
    # a try in flight
    h.set_robust_loss(psba_amd.LOSS_HUBER, 2.0)
    h.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h.schur_reduce()
    h.schur_solve()
    h.backsub_async(mu)
    with pytest.raises(capi.PsbaError) as ei:
        h.set_robust_loss(psba_amd.LOSS_CAUCHY, 2.0)
    assert ei.value.code == -6
    h.backsub_wait()
    h.set_robust_loss(psba_amd.LOSS_CAUCHY, 2.0)
    h.close()
    fk = psba_amd.Psba(0)
    fk.set_camera_model(True)
    fk.upload_problem(psba_amd.read_problem(os.path.join(DATA, "54camsvarK.txt"), os.path.join(DATA, "54pts.txt")))
    with pytest.raises(capi.PsbaError) as ei:
        fk.set_robust_loss(psba_amd.LOSS_HUBER, 2.0)
    assert ei.value.code == -6
    with pytest.raises(capi.PsbaError) as ei:
        fk.obs_sq_residuals()
    assert ei.value.code == -6
    fk.close()


def test_setting_none_equals_plain():
    prob, _ = _outliers54()
    plain = _handle(prob)
    none = _handle(prob, psba_amd.LOSS_NONE, 5.0)
    back = _handle(prob, psba_amd.LOSS_HUBER)
    back.set_robust_loss(psba_amd.LOSS_NONE, 1.0)
    for h in (none, back):
        assert np.array_equal(h.compute_exQT(), plain.compute_exQT())
        for x, y in zip(h.compute_jacobiQT(), plain.compute_jacobiQT()):
            assert np.array_equal(x, y)
        assert np.array_equal(h.obs_sq_residuals(), plain.obs_sq_residuals())
    # the loop runs the same kernels; its sums are deterministic only up to the order of the LDS / global atomics
    # (DESIGN 2), so two handles agree to rounding rather than bit for bit
    for h in (plain, none, back):
        h.reset_params()
    rp, lp = plain.levmar(max_iter=10)
    for h in (none, back):
        r, lg = h.levmar(max_iter=10)
        assert r.iters == rp.iters and lg.shape == lp.shape
        close(lg[:, 1], lp[:, 1], 1e-12, "logged costs")
        assert abs(r.final_err - rp.final_err) <= 1e-12 * rp.final_err
        for x, y in zip(h.get_params(), plain.get_params()):
            close(x, y, 1e-10, "parameters after 10 LM iterations")
    for h in (plain, none, back):
        h.close()


def test_huge_huber_scale_is_plain_levmar():
    prob, _ = _outliers54()
    plain = _handle(prob)
    s = plain.obs_sq_residuals()
    big = _handle(prob, psba_amd.LOSS_HUBER, 1e3 * np.sqrt(s.max()))  # every s <= c2 on the whole path
    assert abs(big.residual(0) - plain.residual(0)) <= 1e-13 * plain.residual(0)
    rp, lp = plain.levmar(max_iter=5)
    rb, lb = big.levmar(max_iter=5)
    assert rp.iters == rb.iters == 5 and rp.flag == rb.flag and lp.shape == lb.shape
    close(lb[:, 1], lp[:, 1], 1e-13, "logged costs")
    close(lb, lp, 1e-9, "levmar log")
    assert abs(rb.final_err - rp.final_err) <= 1e-13 * rp.final_err
    plain.close()
    big.close()


def _one_try_case(case):
    rng = np.random.default_rng(21)
    if case in ("default", "owner", "pcg", "v1", "read_w"):
        base = _prob54()
    elif case == "cam_major":  # >= 230 cameras: K1's camera sums by the camera-major pass
        base = synth.make_problem(240, 1500, 6, seed=7)
    else:  # "long": points seen by more than 256 cameras (the *_long kernels), also camera-major
        base = synth.make_problem(270, 30, 262, seed=8, min_track=258, max_track=270)
        assert np.bincount(base["iidx"]).max() > 256
    return _lens_outlier_problem(base, rng, kc_scale=1.0 if base["nC"] == 54 else 30.0)


ROUTES = {"default": {}, "owner": {"PSBA_SCHUR_OWNER": "1"}, "cam_major": {}, "long": {}, "pcg": {},
          "v1": {"PSBA_LIN_V1": "1"}, "read_w": {"PSBA_BACK_READ_W": "1"}}


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("case", list(ROUTES))
def test_one_damping_try_against_twin(case, kind, monkeypatch):
    for k, v in ROUTES[case].items():
        monkeypatch.setenv(k, v)
    prob, kc, cov = _one_try_case(case)
    t, (e, A, B), lin = robust_pieces(prob, KINDS[kind], C, kc, cov)
    w = t.weights()
    assert w.min() < 0.5 and w.max() > 0.9  # both regions of the loss are exercised
    mu = 1e-3 * lin["maxdiag"]
    ref = robust_pieces(prob, KINDS[kind], C, kc, cov, mu=mu)[2]
    assert ref["ret"] == 0.0
    nA = 6 * prob["nC"]
    h = _handle(prob, KINDS[kind], C, kc, cov, solver=1 if case == "pcg" else None)
    assert abs(h.residual(0) - t.cost()) <= 1e-12 * t.cost()
    close(h.obs_sq_residuals(), t.sq_residuals(), 1e-12, "s")
    h.linearize(1.0, 1.0)
    assert abs(h.max_diag() - lin["maxdiag"]) <= 1e-12 * lin["maxdiag"]
    close(h.get_gradient(), lin["g"], 1e-11, "g")
    h.schur_assemble(mu)
    if case == "pcg":
        jk, val, ea = h.get_sparse_S()
        for (j, k), Bk in zip(jk, val):
            got = Bk if j != k else np.tril(Bk) + np.tril(Bk, -1).T
            assert np.abs(got - ref["S"][6 * j:6 * j + 6, 6 * k:6 * k + 6]).max() <= 1e-11 * np.abs(ref["S"]).max()
    else:
        n32 = (nA + 31) // 32 * 32
        M = h.get_reduce_buffer().reshape(n32 + 1, n32)
        close(M[:nA, :nA], ref["S"], 1e-11, "S")
        ea = M[n32, :nA]
    close(ea, ref["ea"], 1e-10, "ea")
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    dp = ref["dp"]
    got = h.get_dp()
    close(got[:nA], dp[:nA], 1e-8 if case == "pcg" else 1e-9, "dpa")
    if case == "pcg":
        h.close()
        return
    close(got, dp, 1e-9, "dp")
    newp = np.r_[t.cams.reshape(-1), t.pts.reshape(-1)] + dp
    new_cost = t.cost(cams=newp[:nA], pts=newp[nA:])
    for name, g, want in [("dp_l2", sc.dp_l2, dp @ dp), ("gain_den", sc.gain_den, dp @ (mu * dp + lin["g"])),
                          ("new_cost", sc.new_cost, new_cost), ("newp_l2", sc.newp_l2, newp @ newp)]:
        assert abs(g - want) <= 1e-8 * abs(want), (name, g, want)
    close(h.obs_sq_residuals(capi.PARAMS_NEW), t.sq_residuals(newp[:nA], newp[nA:]), 1e-9, "s at the proposal")
    if case in ("default", "v1"):  # the mirror verbs: what the normal equations see
        close(h.compute_exQT(), e.reshape(-1), 1e-11, "w L e")
        JA, JB = h.compute_jacobiQT()
        close(JA, A.reshape(-1), 1e-11, "w L A")
        close(JB, B.reshape(-1), 1e-11, "w L B")
        close(h.compute_U(1.0), lin["U"], 1e-11, "U")
        close(h.compute_V(1.0), lin["V"], 1e-11, "V")
        close(h.compute_Wblks(1.0), lin["W"], 1e-11, "W")
        close(h.compute_g(1.0), lin["g"], 1e-11, "g (mirror)")
    h.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_gradient_against_central_differences(kind):
    """-2 g = dF/dp, with F from psba_residual through psba_set_params: independent of the twin"""
    prob, _ = _outliers54()
    h = _handle(prob, KINDS[kind])
    h.linearize(1.0, 1.0)
    g = h.get_gradient()
    cams, pts = h.get_params()
    p0 = np.r_[cams.reshape(-1), pts.reshape(-1)]
    nA = cams.size
    rng = np.random.default_rng(5)
    ks = np.r_[np.arange(nA), nA + rng.choice(p0.size - nA, 300, replace=False)]
    fd = np.empty(ks.size)
    for n, k in enumerate(ks):
        hk = 1e-6 * max(abs(p0[k]), 1e-2)
        vals = []
        for sgn in (1.0, -1.0):
            p = p0.copy()
            p[k] += sgn * hk
            h.set_params(p[:nA], p[nA:])
            vals.append(h.residual(0))
        fd[n] = (vals[0] - vals[1]) / (2.0 * hk)
    err = np.abs(-2.0 * g[ks] - fd).max() / np.abs(fd).max()
    assert err <= 1e-6, err
    h.close()


# thresholds from the twin's dense LM on the same problem (CPU): reprojection distance to the clean LM
# solution 5.72 px for plain LM on the corrupted data, 1.70 px Huber, 1.51 px Cauchy (c = 2); s > 9 c2 flags 97.8 %
# (Huber) and 100 % (Cauchy) of the corrupted observations and 1 / 0 of the others
def _recovery_problems():
    base = synth.make_problem(30, 300, 6, seed=5, noise_px=1.0)
    prob, idx = synth.add_outliers(base, 0.05, 20.0, 80.0, 5)
    return base, prob, idx


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_recovery_from_outliers(kind):
    base, prob, idx = _recovery_problems()
    clean = _handle(base)
    clean.levmar(max_iter=100)
    tw = Twin(base)
    P0 = tw.project(*clean.get_params())

    def dist(h):
        return np.sqrt(((tw.project(*h.get_params()) - P0) ** 2).sum(1).mean())

    plain = _handle(prob)
    plain.levmar(max_iter=100)
    rob = _handle(prob, KINDS[kind])
    res, _ = rob.levmar(max_iter=100)
    d_plain, d_rob = dist(plain), dist(rob)
    assert d_plain >= 2.5 * d_rob, (d_plain, d_rob)
    assert d_rob < 2.5, d_rob
    s = rob.obs_sq_residuals()
    flag = s > 9.0 * C * C
    assert flag[idx].mean() >= 0.9, flag[idx].mean()
    assert flag.sum() - flag[idx].sum() <= 0.01 * (prob["nO"] - idx.size)
    assert abs(res.final_err - RobustTwin(prob, KINDS[kind], C).cost(*rob.get_params())) <= 1e-10 * res.final_err
    for h in (clean, plain, rob):
        h.close()


def _solver_problem():
    base = synth.make_problem(12, 150, 5, seed=11, noise_px=1.0)
    return synth.add_outliers(base, 0.05, 20.0, 80.0, 11)[0]


@pytest.mark.parametrize("how", ["solve", "pcg"])
def test_solvers_reach_dense_lm_under_huber(how):
    prob = _solver_problem()
    want = RobustTwin(prob, KINDS["huber"], C).solve_lm(200)[2]
    if how == "solve":
        h = _handle(prob, KINDS["huber"])
        got = h.solve(max_iter=200).final_err
    else:
        h = _handle(prob, KINDS["huber"], solver=1)
        got = h.levmar(max_iter=200)[0].final_err
    assert abs(got - want) <= 1e-6 * want, (got, want)
    h.close()


def test_rank_layout_matches_one_handle():
    rng = np.random.default_rng(51)
    prob, kc, cov = _lens_outlier_problem(_prob54(), rng)
    prob = capi.Problem(prob, kc=kc, cov=cov)
    one = _handle(prob, KINDS["cauchy"], C, kc, cov)
    c_one = one.residual(0)
    one.linearize(1.0, 1.0)
    mu = 1e-3 * one.max_diag()
    one.schur_assemble(mu)
    want_buf = one.get_reduce_buffer()
    one.schur_reduce()
    one.schur_solve()
    want = one.backsub(mu)
    hs = []
    for r in range(2):
        s = capi.shard_problem(prob, 2, r)
        h = psba_amd.Psba(0)
        h.set_rank_layout(2, r)
        h.upload_problem(s)
        h.set_distortion(s["kc"])
        h.set_obs_covariance(s["cov"])
        h.set_robust_loss(KINDS["cauchy"], C)
        hs.append(h)
    assert abs(sum(h.residual(0) for h in hs) - c_one) <= 1e-12 * c_one
    for h in hs:
        h.linearize(1.0, 1.0)
        h.schur_assemble(mu)
    total = sum(h.get_reduce_buffer() for h in hs)
    close(total, want_buf, 1e-12, "reduce buffer summed over 2 shards")
    got = np.zeros(4)
    for h in hs:
        h.set_reduce_buffer(total)
        h.schur_solve()
        sc = h.backsub(mu)
        assert sc.status == 0
        got += [sc.dp_l2, sc.gain_den, sc.new_cost, sc.newp_l2]
    for g, w in zip(got, [want.dp_l2, want.gain_den, want.new_cost, want.newp_l2]):
        assert abs(g - w) <= 1e-9 * abs(w), (g, w)
    for h in hs + [one]:
        h.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_jmul_matches_twin(kind):
    rng = np.random.default_rng(41)
    prob, kc, cov = _lens_outlier_problem(_prob54(), rng)
    t = RobustTwin(prob, KINDS[kind], C, kc, cov)
    _, A, B = t.linearize()
    h = _handle(prob, KINDS[kind], C, kc, cov)
    nA = 6 * prob["nC"]
    x1 = rng.normal(size=nA + 3 * prob["nP"])
    x2 = rng.normal(size=x1.size)

    def jx(x):
        xc, xp = x[:nA].reshape(-1, 6), x[nA:].reshape(-1, 3)
        return (np.einsum("nab,nb->na", A, xc[t.j]) + np.einsum("nab,nb->na", B, xp[t.i])).reshape(-1)

    close(h.compute_Jmultiply(x1), jx(x1), 1e-12, "J x")
    d = h.jmul_dots(x1, x2)
    j1, j2 = jx(x1), jx(x2)
    close(d, [j1 @ j1, j1 @ j2, j2 @ j2], 1e-12, "J-norm dots")
    h.close()
