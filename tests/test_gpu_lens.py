"""Lens distortion and per-observation covariances on the GPU (psba_set_distortion, psba_set_obs_covariance):
every route K1 and K3 can take against the numpy twin (tests/lens_twin.py, itself pinned to the oracle), the neutral
settings against the plain handle, Sigma = 4 I as an exact scaling of the oracle-pinned path, recovery of noise-free
distorted data, J x, a sharded rank layout and the error codes.  Needs an MI355X."""
import os

import numpy as np
import pytest

import psba_amd
from psba_amd import capi, synth
from lens_twin import Twin, oracle_pieces
from sba_text import KK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")


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


def _lens_problem(prob, rng, kc_scale=1.0):
    """prob's geometry with synthetic kc per camera and random SPD covariances; observations re-projected through
    the lens model plus ~1 px of noise, so that the residuals are those of a real problem"""
    kc = _kc(rng, prob["nC"]) * kc_scale
    cov = _spd(rng, prob["nO"])
    t = Twin(prob, kc)
    p = capi.Problem(prob, impts=t.project() + rng.normal(size=(prob["nO"], 2)))
    return p, kc, cov


def _handle(prob, kc=None, cov=None, solver=None):
    h = psba_amd.Psba(0)
    if solver is not None:
        h.set_solver(solver, tol=1e-12, max_iter=4000)
    h.upload_problem(prob)
    if kc is not None:
        h.set_distortion(kc)
    if cov is not None:
        h.set_obs_covariance(cov)
    return h


def test_mirror_verbs_match_twin():
    rng = np.random.default_rng(11)
    prob, kc, cov = _lens_problem(_prob54(), rng)
    t = Twin(prob, kc, cov)
    e, A, B = t.linearize()
    lin = oracle_pieces(prob, e, A, B)
    h = _handle(prob, kc, cov)
    assert h.lens_model() == (True, True)
    close(h.compute_exQT(), e.reshape(-1), 1e-11, "whitened e")
    JA, JB = h.compute_jacobiQT()
    close(JA, A.reshape(-1), 1e-11, "whitened A")
    close(JB, B.reshape(-1), 1e-11, "whitened B")
    assert np.abs(JA.reshape(-1, 12)[:, 9]).max() > 0.0  # d10 != 0 under distortion and covariances
    close(h.compute_U(1.0), lin["U"], 1e-11, "U")
    close(h.compute_V(1.0), lin["V"], 1e-11, "V")
    close(h.compute_Wblks(1.0), lin["W"], 1e-11, "W")
    close(h.compute_g(1.0), lin["g"], 1e-11, "g")
    mu = 1e-3 * lin["maxdiag"]
    ref = oracle_pieces(prob, e, A, B, mu=mu)
    h.update_UV(mu)
    close(h.compute_S(), ref["S"], 1e-11, "S")
    close(h.compute_ea(), ref["ea"], 1e-11, "ea")
    # and the twin's own dense Schur complement of the weighted normal equations
    S, ea = t.schur(mu)
    close(ref["S"], S, 1e-9, "oracle sums vs dense twin S")
    close(ref["ea"], ea, 1e-9, "oracle sums vs dense twin ea")
    # the weighted cost
    assert abs(h.residual(0) - t.cost()) <= 1e-12 * t.cost()
    h.close()


@pytest.mark.parametrize("owner", [False, True])
def test_neutral_settings_equal_plain(owner, monkeypatch):
    if owner:
        monkeypatch.setenv("PSBA_SCHUR_OWNER", "1")
    prob = _prob54()
    plain = _handle(prob)
    neutral = _handle(prob, np.zeros((prob["nC"], 5)), np.tile(np.eye(2), (prob["nO"], 1, 1)))
    assert neutral.lens_model() == (True, True) and plain.lens_model() == (False, False)
    assert plain.schur_path() == neutral.schur_path() == (1 if owner else 0)
    for what in ("compute_exQT", "compute_jacobiQT"):
        a, b = getattr(plain, what)(), getattr(neutral, what)()
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            close(y, x, 1e-13, what)
    for what in ("compute_U", "compute_V", "compute_Wblks", "compute_g"):
        close(getattr(neutral, what)(1.0), getattr(plain, what)(1.0), 1e-13, what)
    mu = 1e-3 * plain.maxElmOfUV()
    plain.update_UV(mu)
    neutral.update_UV(mu)
    close(neutral.compute_S(), plain.compute_S(), 1e-13, "S")
    close(neutral.compute_ea(), plain.compute_ea(), 1e-13, "ea")
    for h in (plain, neutral):
        h.restore_UVdiag()
        h.reset_params()
    rp, _ = plain.levmar(max_iter=10)
    rn, _ = neutral.levmar(max_iter=10)
    assert abs(rn.final_err - rp.final_err) <= 1e-10 * rp.final_err
    for x, y in zip(plain.get_params(), neutral.get_params()):
        close(y, x, 1e-10, "parameters after 10 LM iterations")
    plain.close()
    neutral.close()


def test_sigma_4I_is_an_exact_scaling():
    """Sigma = 4 I: L = I / 2 exactly, so every weighted quantity is the plain one times a power of two and the LM
    path (whose plain run is pinned to the oracle by test_gpu_parity) is the same bit for bit."""
    prob = _prob54()
    plain = _handle(prob)
    sc = _handle(prob, cov=np.tile(4.0 * np.eye(2), (prob["nO"], 1, 1)))
    assert sc.lens_model() == (False, True)
    rp, lp = plain.levmar(max_iter=5)
    rs, ls = sc.levmar(max_iter=5)
    assert rp.iters == rs.iters == 5 and rp.flag == rs.flag
    assert lp.shape == ls.shape
    close(4.0 * ls[:, 1], lp[:, 1], 1e-12, "logged costs")
    close(ls[:, 2], lp[:, 2], 1e-12, "rho")
    assert abs(4.0 * rs.final_err - rp.final_err) <= 1e-12 * rp.final_err
    for x, y in zip(plain.get_params(), sc.get_params()):
        close(y, x, 1e-12, "parameters")
    plain.close()
    sc.close()


def _one_try_case(case):
    rng = np.random.default_rng(21)
    if case in ("default", "owner", "pcg"):
        base = _prob54()
    elif case == "cam_major":  # >= 230 cameras: K1's camera sums by the camera-major pass
        base = synth.make_problem(240, 1500, 6, seed=7)
    else:  # "long": points seen by more than 256 cameras (the *_long kernels), also camera-major
        base = synth.make_problem(270, 30, 262, seed=8, min_track=258, max_track=270)
        assert np.bincount(base["iidx"]).max() > 256
    return _lens_problem(base, rng, kc_scale=1.0 if case in ("default", "owner", "pcg") else 30.0)


@pytest.mark.parametrize("case", ["default", "owner", "cam_major", "long", "pcg"])
def test_one_damping_try_against_twin(case, monkeypatch):
    if case == "owner":
        monkeypatch.setenv("PSBA_SCHUR_OWNER", "1")
    prob, kc, cov = _one_try_case(case)
    t = Twin(prob, kc, cov)
    e, A, B = t.linearize()
    lin = oracle_pieces(prob, e, A, B)
    mu = 1e-3 * lin["maxdiag"]
    ref = oracle_pieces(prob, e, A, B, mu=mu)
    assert ref["ret"] == 0.0
    nA = 6 * prob["nC"]
    h = _handle(prob, kc, cov, solver=1 if case == "pcg" else None)
    assert abs(h.residual(0) - t.cost()) <= 1e-12 * t.cost()
    h.linearize(1.0, 1.0)
    assert abs(h.max_diag() - lin["maxdiag"]) <= 1e-12 * lin["maxdiag"]
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
        return
    close(got, dp, 1e-9, "dp")
    newp = np.r_[t.cams.reshape(-1), t.pts.reshape(-1)] + dp
    new_cost = t.cost(cams=newp[:nA], pts=newp[nA:])
    for name, g, w in [("dp_l2", sc.dp_l2, dp @ dp), ("gain_den", sc.gain_den, dp @ (mu * dp + lin["g"])),
                       ("new_cost", sc.new_cost, new_cost), ("newp_l2", sc.newp_l2, newp @ newp)]:
        assert abs(g - w) <= 1e-8 * abs(w), (name, g, w)
    h.close()


def _recovery_problem():
    """noise-free synthetic data with strong distortion (|k1 r^2| ~ 0.1 at the image edge), perturbed start"""
    rng = np.random.default_rng(31)
    base = synth.make_problem(16, 400, 8, seed=9, noise_px=0.0)
    t = Twin(base)
    P = t.project()
    r2max = (((P - base["K"][0, 1:3]) / base["K"][0, 0]) ** 2).sum(1).max()
    k1 = 0.1 / r2max
    kc = np.column_stack([k1 * np.ones(16), np.zeros(16), 1e-3 * rng.normal(size=16), 1e-3 * rng.normal(size=16),
                          np.zeros(16)])
    truth = capi.Problem(base, impts=Twin(base, kc).project())
    start = capi.Problem(truth, cams=truth["cams"] + 1e-4 * rng.normal(size=truth["cams"].shape),
                         pts=truth["pts"] + 1e-3 * rng.normal(size=truth["pts"].shape))
    return truth, start, kc


@pytest.mark.parametrize("how", ["levmar", "solve"])
def test_recovery_of_distorted_data(how):
    truth, start, kc = _recovery_problem()
    h = _handle(start, kc)
    c0 = h.residual(0)
    if how == "levmar":
        res, _ = h.levmar(max_iter=60)
    else:
        res = h.solve(max_iter=60)
    cams, pts = h.get_params()
    rms = np.sqrt(Twin(start, kc).cost(cams=cams, pts=pts) / truth["nO"])
    assert rms < 1e-8, (how, rms, res.final_err, c0)
    plain = _handle(start)
    if how == "levmar":
        rp, _ = plain.levmar(max_iter=60)
    else:
        rp = plain.solve(max_iter=60)
    assert rp.final_err >= 1e3 * max(res.final_err, 1e-30), (rp.final_err, res.final_err)
    assert rp.final_err >= 1e-6  # the plain model stalls far from the data
    h.close()
    plain.close()


def test_jmul_matches_twin():
    rng = np.random.default_rng(41)
    prob, kc, cov = _lens_problem(_prob54(), rng)
    t = Twin(prob, kc, cov)
    _, A, B = t.linearize()
    h = _handle(prob, kc, cov)
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


def test_rank_layout_with_sharded_covariances():
    rng = np.random.default_rng(51)
    prob, kc, cov = _lens_problem(_prob54(), rng)
    prob = capi.Problem(prob, kc=kc, cov=cov)
    one = _handle(prob, kc, cov)
    one.linearize(1.0, 1.0)
    mu = 1e-3 * one.max_diag()
    one.schur_assemble(mu)
    want = one.get_reduce_buffer()
    hs = []
    for r in range(3):
        s = capi.shard_problem(prob, 3, r)
        h = psba_amd.Psba(0)
        h.set_rank_layout(3, r)
        h.upload_problem(s)
        h.set_distortion(s["kc"])
        h.set_obs_covariance(s["cov"])
        h.linearize(1.0, 1.0)
        h.schur_assemble(mu)
        hs.append(h)
    total = sum(h.get_reduce_buffer() for h in hs)
    close(total, want, 1e-12, "reduce buffer summed over 3 shards")
    for h in hs + [one]:
        h.close()


def test_errors():
    prob = _prob54()
    h = psba_amd.Psba(0)
    with pytest.raises(capi.PsbaError) as ei:  # before upload
        h._ck(capi.lib.psba_set_distortion(h._h, None))
    assert ei.value.code == -6
    with pytest.raises(capi.PsbaError) as ei:
        h._ck(capi.lib.psba_set_obs_covariance(h._h, None))
    assert ei.value.code == -6
    h.upload_problem(prob)
    with pytest.raises(capi.PsbaError):  # wrong size (caught by the binding)
        h.set_distortion(np.zeros((prob["nC"] - 1, 5)))
    with pytest.raises(capi.PsbaError):
        h.set_obs_covariance(np.zeros((prob["nO"] + 1, 2, 2)))
    cov = np.tile(np.eye(2), (prob["nO"], 1, 1))
    cov[17] = [[1.0, 2.0], [2.0, 1.0]]  # indefinite
    with pytest.raises(capi.PsbaError) as ei:
        h.set_obs_covariance(cov)
    assert ei.value.code == -1 and "observation 17" in str(ei.value)
    cov[17] = [[1.0, 0.1], [0.1 + 1e-9, 1.0]]  # not symmetric
    with pytest.raises(capi.PsbaError) as ei:
        h.set_obs_covariance(cov)
    assert ei.value.code == -1 and "observation 17" in str(ei.value)
    assert h.lens_model() == (False, False)
    h.set_distortion(np.zeros((prob["nC"], 5)))
    assert h.lens_model() == (True, False)
    h.upload_problem(prob)  # a new upload resets the lens model
    assert h.lens_model() == (False, False)
    h.close()
    fk = psba_amd.Psba(0)
    fk.set_camera_model(True)
    pk = psba_amd.read_problem(os.path.join(DATA, "54camsvarK.txt"), os.path.join(DATA, "54pts.txt"))
    fk.upload_problem(pk)
    with pytest.raises(capi.PsbaError) as ei:
        fk.set_distortion(np.zeros((prob["nC"], 5)))
    assert ei.value.code == -6
    with pytest.raises(capi.PsbaError) as ei:
        fk.set_obs_covariance(np.tile(np.eye(2), (prob["nO"], 1, 1)))
    assert ei.value.code == -6
    fk.close()
