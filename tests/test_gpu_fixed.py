"""Fixed parameter blocks on the GPU (psba_set_fixed): the error codes and state rules, no mask against the plain
handle, one damping try on every K1 / K2 / K3 route against the numpy twin (tests/fixed_twin.py), the gradient against
central differences of psba_residual, the gauge (two cameras fixed, no damping) judged by tests/dense_ref.py, the
loops, a sharded rank layout, J x and the structure-only shortcut.  Needs an MI355X."""
import os

import numpy as np
import pytest

import psba_amd
from psba_amd import capi, synth
import dense_ref as dr
from fixed_twin import ROUTES, FixedTwin, close, fixed_pieces, random_kc as _kc, random_spd as _spd
from lens_twin import Twin
from robust_twin import KINDS
from sba_text import KK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
C = 2.0  # loss scale (whitened pixels)
ETA_MAX = 1e-14  # tests/test_gpu_dense_solve.py


def _golden(n):
    return psba_amd.read_problem(os.path.join(DATA, f"{n}cams.txt"), os.path.join(DATA, f"{n}pts.txt"), KK)


def _mask(prob, cams=(0, 1), frac=0.1, seed=17):
    """flags [nC], [nP]: the named cameras (negative = from the end) and a seeded fraction of the points"""
    fc = np.zeros(prob["nC"], dtype=np.uint8)
    fc[list(cams)] = 1
    fp = np.zeros(prob["nP"], dtype=np.uint8)
    if frac > 0:
        rng = np.random.default_rng(seed)
        fp[rng.choice(prob["nP"], max(1, round(frac * prob["nP"])), replace=False)] = 1
    return fc, fp


def _handle(prob, fc=None, fp=None, kind=None, c=C, kc=None, cov=None, solver=None):
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
    if fc is not None or fp is not None:
        h.set_fixed(fc, fp)
    return h


def _params(h, which=capi.PARAMS_CUR):
    cams, pts = h.get_params(which)
    return np.r_[cams.reshape(-1), pts.reshape(-1)]


# ---- 1. errors and state rules ---------------------------------------------------------------------------------
def test_errors_and_state_rules():
    prob = _golden(54)
    fc, fp = _mask(prob)
    ub = capi.C.POINTER(capi.C.c_ubyte)
    h = psba_amd.Psba(0)
    with pytest.raises(capi.PsbaError) as ei:  # before upload
        h._ck(capi.lib.psba_set_fixed(h._h, fc.ctypes.data_as(ub), fp.ctypes.data_as(ub)))
    assert ei.value.code == -6
    h.upload_problem(prob)
    assert h.fixed_counts() == (0, 0)
    with pytest.raises(capi.PsbaError) as ei:  # a wrong length raises before the C call
        h.set_fixed(fc[:-1], None)
    assert ei.value.code == -1
    h.set_fixed(fc, fp)
    assert h.fixed_counts() == (2, int(fp.sum()))
    with pytest.raises(capi.PsbaError) as ei:  # no free parameter left
        h.set_fixed(np.ones(prob["nC"], dtype=bool), np.ones(prob["nP"], dtype=np.int64))
    assert ei.value.code == -1
    assert h.fixed_counts() == (2, int(fp.sum()))  # a refused call changes nothing
    h.linearize(1.0, 1.0)
    g = h.get_gradient()
    assert np.all(g[:12] == 0.0) and np.all(g[12:18] != 0.0)  # ... the mask on the device included
    h.set_fixed(None, fp)
    assert h.fixed_counts() == (0, int(fp.sum()))
    h.set_fixed(fc, None)
    assert h.fixed_counts() == (2, 0)
    h.set_fixed(None, None)  # two NULLs clear it
    assert h.fixed_counts() == (0, 0)
    h.set_fixed(np.zeros(prob["nC"]), np.zeros(prob["nP"]))  # an all-zero mask is no mask
    assert h.fixed_counts() == (0, 0)
    h.set_fixed(fc, fp)
    h.upload_problem(prob)  # a new upload resets the mask
    assert h.fixed_counts() == (0, 0)
    h.linearize(1.0, 1.0)
    assert np.all(h.get_gradient()[:12] != 0.0)
    # a try in flight
    h.set_fixed(fc, fp)
    h.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h.schur_reduce()
    h.schur_solve()
    h.backsub_async(mu)
    with pytest.raises(capi.PsbaError) as ei:
        h.set_fixed(None, None)
    assert ei.value.code == -6
    assert h.fixed_counts() == (2, int(fp.sum()))
    h.backsub_wait()
    h.set_fixed(None, None)
    # setting the mask discards a linearization queued ahead: the next verb that needs one refuses
    h.linearize(1.0, 1.0)
    h.set_fixed(fc, None)
    with pytest.raises(capi.PsbaError) as ei:
        h.schur_assemble(mu)
    assert ei.value.code == -6
    h.close()
    fk = psba_amd.Psba(0)
    fk.set_camera_model(True)
    fkp = psba_amd.read_problem(os.path.join(DATA, "54camsvarK.txt"), os.path.join(DATA, "54pts.txt"))
    fk.upload_problem(fkp)
    with pytest.raises(capi.PsbaError) as ei:
        fk.set_fixed(fc, fp)
    assert ei.value.code == -6
    assert fk.fixed_counts() == (0, 0)
    fk.close()


# ---- 2. no mask = plain --------------------------------------------------------------------------------------------
def test_no_mask_equals_plain():
    prob = _golden(54)
    fc, fp = _mask(prob)
    plain = _handle(prob)
    zero = _handle(prob, np.zeros(prob["nC"], dtype=np.uint8), np.zeros(prob["nP"], dtype=np.uint8))
    back = _handle(prob, fc, fp)
    back.set_fixed(None, None)
    for h in (zero, back):
        assert h.fixed_counts() == (0, 0)
        assert np.array_equal(h.compute_exQT(), plain.compute_exQT())
        for x, y in zip(h.compute_jacobiQT(), plain.compute_jacobiQT()):
            assert np.array_equal(x, y)
    # the loop runs the same kernels; its sums are deterministic only up to the order of the LDS / global atomics
    # (DESIGN 2), so two handles agree to rounding rather than bit for bit
    for h in (plain, zero, back):
        h.reset_params()
    rp, lp = plain.levmar(max_iter=10)
    for h in (zero, back):
        r, lg = h.levmar(max_iter=10)
        assert r.iters == rp.iters and lg.shape == lp.shape
        close(lg[:, 1], lp[:, 1], 1e-12, "logged costs")
        assert abs(r.final_err - rp.final_err) <= 1e-12 * rp.final_err
    for h in (plain, zero, back):
        h.close()


# ---- 3. one damping try on every route against the twin --------------------------------------------------------------
def _one_try_case(case, model):
    """(problem, kc, cov, kind): the geometry of tests/test_gpu_robust.py's routes; `lens`: distortion + covariances +
    Cauchy on observations re-projected through the lens model with 5 % outliers"""
    rng = np.random.default_rng(21)
    if case in ("default", "owner", "pcg", "v1", "read_w", "atomic", "runs"):
        base = _golden(54)
    elif case == "cam_major":  # >= 230 cameras: K1's camera sums by the camera-major pass
        base = synth.make_problem(240, 1500, 6, seed=7)
    else:  # "long": points seen by more than 256 cameras (the *_long kernels), also camera-major
        base = synth.make_problem(270, 30, 262, seed=8, min_track=258, max_track=270)
        assert np.bincount(base["iidx"]).max() > 256
    if model == "plain":
        return base, None, None, None
    kc = _kc(rng, base["nC"]) * (1.0 if base["nC"] == 54 else 30.0)
    cov = _spd(rng, base["nO"])
    p = capi.Problem(base, impts=Twin(base, kc).project() + rng.normal(size=(base["nO"], 2)))
    p, _ = synth.add_outliers(p, 0.05, 20.0, 80.0, 2)
    return p, kc, cov, KINDS["cauchy"]


def _assert_fixed_block_structure(S, fa, what):
    """rows and columns of fixed cameras: exactly zero off the diagonal block, the block a positive multiple of I"""
    idx = np.flatnonzero(fa)
    for j0 in idx[::6]:
        blk = S[j0:j0 + 6, j0:j0 + 6]
        assert blk[0, 0] > 0 and np.array_equal(blk, blk[0, 0] * np.eye(6)), (what, j0)
        row = S[j0:j0 + 6].copy()
        row[:, j0:j0 + 6] = 0.0
        col = S[:, j0:j0 + 6].copy()
        col[j0:j0 + 6] = 0.0
        assert np.all(row == 0.0) and np.all(col == 0.0), (what, j0)


@pytest.mark.parametrize("model", ["plain", "lens"])
@pytest.mark.parametrize("case", list(ROUTES))
def test_one_damping_try_against_twin(case, model, monkeypatch):
    for k, v in ROUTES[case].items():
        monkeypatch.setenv(k, v)
    prob, kc, cov, kind = _one_try_case(case, model)
    fc, fp = _mask(prob, cams=(0, 1, -1))
    kw = dict(kind=kind if kind is not None else 0, c=C, kc=kc, cov=cov)
    t, (e, A, B), lin = fixed_pieces(prob, fc, fp, **kw)
    fx = t.fixed_entries()
    nA = 6 * prob["nC"]
    fa = fx[:nA]
    free_a = np.flatnonzero(~fa)
    assert fa.sum() == 18 and fx[nA:].sum() == 3 * fp.sum() > 0
    mu = 1e-3 * lin["maxdiag"]
    ref = fixed_pieces(prob, fc, fp, mu=mu, **kw)[2]
    assert ref["ret"] == 0.0 and np.all(ref["dp"][fx] == 0.0)
    h = _handle(prob, fc, fp, kind, C, kc, cov, solver=1 if case == "pcg" else None)
    assert abs(h.residual(0) - t.cost()) <= 1e-12 * t.cost()  # every observation counts
    p_cur = _params(h)
    h.linearize(1.0, 1.0)
    md = h.max_diag()
    print(f"{case}/{model}: max_diag rel {abs(md - lin['maxdiag']) / lin['maxdiag']:.2e}")
    # (the free diagonal entries here are 1e7 and more, far above the placeholder: this holds the maximum to the twin's,
    # not the mask of k_max_diag_fixed -- that is test_gpu_fixed_entrywise.py, on a problem scaled below the placeholder)
    assert abs(md - lin["maxdiag"]) <= 1e-12 * lin["maxdiag"]
    assert abs(h.maxElmOfUV() - lin["maxdiag"]) <= 1e-12 * lin["maxdiag"]
    g = h.get_gradient()
    close(g, lin["g"], 1e-11, "g")
    assert np.all(g[fx] == 0.0)
    h.schur_assemble(mu)
    if case == "pcg":
        jk, val, ea = h.get_sparse_S()
        fcam = fc.astype(bool)
        for (j, k), Bk in zip(jk, val):
            got = Bk if j != k else np.tril(Bk) + np.tril(Bk, -1).T
            if fcam[j] or fcam[k]:
                if j != k:
                    assert np.all(got == 0.0), (j, k)
                else:
                    assert got[0, 0] > 0 and np.array_equal(got, got[0, 0] * np.eye(6)), j
            else:
                assert np.abs(got - ref["S"][6 * j:6 * j + 6, 6 * k:6 * k + 6]).max() <= 1e-11 * np.abs(ref["S"]).max()
    else:
        n32 = (nA + 31) // 32 * 32
        M = h.get_reduce_buffer().reshape(n32 + 1, n32)
        S = M[:nA, :nA]
        close(S[np.ix_(free_a, free_a)], ref["S"][np.ix_(free_a, free_a)], 1e-11, "S (free blocks)")
        _assert_fixed_block_structure(S, fa, "S")
        ea = M[n32, :nA]
    close(ea, ref["ea"], 1e-10, "ea")
    assert np.all(ea[fa] == 0.0)
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    dp = ref["dp"]
    got = h.get_dp()
    print(f"{case}/{model}: dpa rel {np.abs(got[:nA] - dp[:nA]).max() / np.abs(dp[:nA]).max():.2e} "
          f"dp rel {np.abs(got - dp).max() / np.abs(dp).max():.2e}")
    close(got[:nA], dp[:nA], 1e-8 if case == "pcg" else 1e-9, "dpa")  # (the iterative solve: the project's bar for it)
    close(got, dp, 1e-9, "dp")
    assert np.all(got[fx] == 0.0)
    p_new = _params(h, capi.PARAMS_NEW)
    assert np.array_equal(p_new[fx], p_cur[fx]) and not np.array_equal(p_new[~fx], p_cur[~fx])
    newp = np.r_[t.cams.reshape(-1), t.pts.reshape(-1)] + dp
    new_cost = t.cost(cams=newp[:nA], pts=newp[nA:])
    for name, v, want in [("dp_l2", sc.dp_l2, dp @ dp), ("gain_den", sc.gain_den, dp @ (mu * dp + lin["g"])),
                          ("new_cost", sc.new_cost, new_cost), ("newp_l2", sc.newp_l2, newp @ newp)]:
        print(f"{case}/{model}: {name} rel {abs(v - want) / abs(want):.2e}")
        assert abs(v - want) <= 1e-8 * abs(want), (name, v, want)
    if case in ("default", "v1"):  # the mirror verbs: what the normal equations see
        close(h.compute_exQT(), e.reshape(-1), 1e-11, "e")
        JA, JB = h.compute_jacobiQT()
        close(JA, A.reshape(-1), 1e-11, "masked A")
        close(JB, B.reshape(-1), 1e-11, "masked B")
        assert np.all(JA.reshape(-1, 12)[fc[t.j] != 0] == 0.0) and np.all(JB.reshape(-1, 6)[fp[t.i] != 0] == 0.0)
        U = h.compute_U(1.0).reshape(-1, 6, 6)
        V = h.compute_V(1.0).reshape(-1, 3, 3)
        fcb, fpb = fc != 0, fp != 0
        close(U[~fcb], lin["U"].reshape(-1, 6, 6)[~fcb], 1e-11, "U (free)")
        close(V[~fpb], lin["V"].reshape(-1, 3, 3)[~fpb], 1e-11, "V (free)")
        for blk in list(U[fcb]) + list(V[fpb]):
            assert blk[0, 0] > 0 and np.array_equal(blk, blk[0, 0] * np.eye(blk.shape[0]))
        W = h.compute_Wblks(1.0)
        close(W, lin["W"], 1e-11, "W")
        assert np.all(W.reshape(-1, 18)[(fc[t.j] != 0) | (fp[t.i] != 0)] == 0.0)
        gm = h.compute_g(1.0)
        close(gm, lin["g"], 1e-11, "g (mirror)")
        assert np.all(gm[fx] == 0.0)
        h.update_UV(mu)
        Sm = h.compute_S()
        close(Sm[np.ix_(free_a, free_a)], ref["S"][np.ix_(free_a, free_a)], 1e-11, "S (mirror, free blocks)")
        _assert_fixed_block_structure(Sm, fa, "S (mirror)")
        eam = h.compute_ea()
        close(eam, ref["ea"], 1e-10, "ea (mirror)")
        assert np.all(eam[fa] == 0.0)
        h.restore_UVdiag()
    h.close()


# ---- 4. gradient by central differences of psba_residual --------------------------------------------------------------
def test_gradient_against_central_differences():
    """-2 g = dF/dp on the free entries, with F from psba_residual through psba_set_params: independent of the twin"""
    prob, _ = synth.add_outliers(_golden(54), 0.05, 20.0, 80.0, 1)
    fc, fp = _mask(prob)
    h = _handle(prob, fc, fp, KINDS["huber"])
    h.linearize(1.0, 1.0)
    g = h.get_gradient()
    p0 = _params(h)
    nA = 6 * prob["nC"]
    fx = np.r_[np.repeat(fc != 0, 6), np.repeat(fp != 0, 3)]
    assert np.all(g[fx] == 0.0)
    rng = np.random.default_rng(5)
    ks = np.r_[np.arange(nA), nA + rng.choice(p0.size - nA, 300, replace=False)]
    ks = ks[~fx[ks]]
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


# ---- 5. the gauge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 9, 54])
def test_two_fixed_cameras_make_S_positive_definite_without_damping(n):
    prob = _golden(n)
    fc, _ = _mask(prob, frac=0.0)
    h = _handle(prob, fc, None)
    nA = 6 * n
    n32 = dr.n32_of(nA)
    h.linearize(1.0, 1.0)
    h.schur_assemble(0.0)
    M = h.get_reduce_buffer().reshape(n32 + 1, n32)
    S = M[:nA, :nA].copy()
    dr.symmetrize_from_lower(S)  # the factorization reads the lower triangle
    b = M[n32, :nA].copy()
    rc, dpa = h.SPDinv_matVec()
    assert rc == capi.PSBA_OK, f"{n} cameras: rc {rc}"
    assert np.all(np.isfinite(dpa)) and np.all(dpa[:12] == 0.0)
    eta = dr.backward_error(S, dpa, b)
    free = np.arange(12, nA)
    Sf = S[np.ix_(free, free)]
    kappa = dr.cond2(Sf)
    fe = dr.forward_error(dpa[free], dr.refined_solution(Sf, b[free]))
    print(f"{n} cameras, cameras 0 and 1 fixed, mu = 0: eta {eta:.3e}, kappa2 {kappa:.3e}, forward error {fe:.3e} "
          f"(bound {2 * kappa * 1e-14:.3e})")
    assert eta <= ETA_MAX, eta
    assert fe <= 2 * kappa * 1e-14, (fe, kappa)
    if n <= 9:  # the whole undamped step against the reduced Gauss-Newton step (the dense J of 54 cameras is 6 GB)
        sc = h.backsub(0.0)
        assert sc.status == 0
        got = h.get_dp()
        t = FixedTwin(prob, fc, None)
        Jf, fr = t.reduced_jacobian()
        e, _, _ = Twin.linearize(t)
        want = np.zeros(got.size)
        want[fr] = np.linalg.lstsq(Jf, e.reshape(-1), rcond=None)[0]
        cj = np.linalg.cond(Jf)
        err = np.abs(got - want).max() / np.abs(want).max()
        erra = np.abs(got[:nA] - want[:nA]).max() / np.abs(want[:nA]).max()
        print(f"{n} cameras: cond J {cj:.3e}, Gauss-Newton step rel err {err:.3e} (dpa {erra:.3e}), "
              f"bound {2 * cj * cj * 1e-14:.3e}")
        assert err <= 2 * cj * cj * 1e-14 and erra <= 2 * cj * cj * 1e-14
        assert np.all(got[:12] == 0.0)
    h.close()


# ---- 6. loops ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["levmar", "solve", "pcg"])
def test_loops_reach_the_twins_dense_lm(how):
    prob = synth.make_problem(12, 150, 5, seed=11)
    fc, fp = _mask(prob)
    want = FixedTwin(prob, fc, fp).solve_lm(200)[2]
    h = _handle(prob, fc, fp, solver=1 if how == "pcg" else None)
    p0 = _params(h)
    got = h.solve(max_iter=200).final_err if how == "solve" else h.levmar(max_iter=200)[0].final_err
    print(f"{how}: final cost {got:.12e}, twin {want:.12e}, rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-6 * want, (got, want)
    fx = np.r_[np.repeat(fc != 0, 6), np.repeat(fp != 0, 3)]
    p1 = _params(h)
    assert np.array_equal(p1[fx], p0[fx]) and not np.array_equal(p1[~fx], p0[~fx])
    h.close()


def test_trust_region_from_lambda_zero():
    """cameras 0 and 1 fixed: S is positive definite at lambda = 0 (DESIGN 7c records chol_fail next to the unmasked
    run's; try counts are not asserted)"""
    prob = _golden(54)
    fc, _ = _mask(prob, frac=0.0)
    out = {}
    for name, m in (("masked", fc), ("unmasked", None)):
        h = _handle(prob, m, None)
        p0 = _params(h)
        res, _ = h.trust_region(max_iter=30, init_lambda=0.0)
        out[name] = res.chol_fail
        print(f"trust_region, 54 cameras, {name}: iters {res.iters} tries {res.tries} chol_fail {res.chol_fail} "
              f"cost {res.init_err:.6e} -> {res.final_err:.6e}")
        assert np.isfinite(res.final_err) and res.final_err < res.init_err
        if m is not None:
            assert np.array_equal(_params(h)[:12], p0[:12])
        h.close()


# ---- 7. rank layout --------------------------------------------------------------------------------------------------
def test_rank_layout_matches_one_handle():
    base = _golden(54)
    fc, fp = _mask(base)
    prob = capi.Problem(base, fixed_cams=fc, fixed_pts=fp)
    one = _handle(prob, fc, fp)
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
        h.set_fixed(s["fixed_cams"], s["fixed_pts"])
        hs.append(h)
    assert sum(h.fixed_counts()[1] for h in hs) == fp.sum()
    assert abs(sum(h.residual(0) for h in hs) - c_one) <= 1e-12 * c_one
    for h in hs:
        h.linearize(1.0, 1.0)
        h.schur_assemble(mu)
    total = sum(h.get_reduce_buffer() for h in hs)
    close(total, want_buf, 1e-12, "reduce buffer summed over 2 shards")
    nA = 6 * base["nC"]
    n32 = dr.n32_of(nA)
    T, W = total.reshape(n32 + 1, n32), want_buf.reshape(n32 + 1, n32)
    assert np.array_equal(T[:12, :12], W[:12, :12])  # the placeholder is written once, by rank 0
    got = np.zeros(4)
    for h in hs:
        h.set_reduce_buffer(total)
        h.schur_solve()
        sc = h.backsub(mu)
        assert sc.status == 0
        got += [sc.dp_l2, sc.gain_den, sc.new_cost, sc.newp_l2]
        assert np.all(h.get_dp()[:12] == 0.0)
    for v, w in zip(got, [want.dp_l2, want.gain_den, want.new_cost, want.newp_l2]):
        assert abs(v - w) <= 1e-9 * abs(w), (v, w)
    for h in hs + [one]:
        h.close()


# ---- 8. J x ----------------------------------------------------------------------------------------------------------
def test_jmul_uses_the_masked_jacobian():
    prob, kc, cov, kind = _one_try_case("default", "lens")
    fc, fp = _mask(prob)
    t = FixedTwin(prob, fc, fp, kind, C, kc, cov)
    _, A, B = t.linearize()
    h = _handle(prob, fc, fp, kind, C, kc, cov)
    nA = 6 * prob["nC"]
    rng = np.random.default_rng(41)
    x1 = rng.normal(size=nA + 3 * prob["nP"])
    x2 = rng.normal(size=x1.size)

    def jx(x):
        xc, xp = x[:nA].reshape(-1, 6), x[nA:].reshape(-1, 3)
        return (np.einsum("nab,nb->na", A, xc[t.j]) + np.einsum("nab,nb->na", B, xp[t.i])).reshape(-1)

    j1, j2 = jx(x1), jx(x2)
    got = h.compute_Jmultiply(x1)
    close(got, j1, 1e-12, "J x")
    d = h.jmul_dots(x1, x2)
    close(d, [j1 @ j1, j1 @ j2, j2 @ j2], 1e-12, "J-norm dots")
    # fixed entries of x are ignored, whatever they hold
    fx = t.fixed_entries()
    y1, y2 = x1.copy(), x2.copy()
    y1[fx] = 1e6 * rng.normal(size=int(fx.sum()))
    y2[fx] = np.nan
    assert np.array_equal(h.compute_Jmultiply(y1), got)
    assert np.array_equal(h.compute_Jmultiply(y2), h.compute_Jmultiply(x2))
    # (the three dot products are summed over the workgroups with atomics: equal up to the order of those adds,
    # DESIGN 2, not bit for bit -- two calls with the same x differ in the last bits already)
    dy = h.jmul_dots(y1, y2)
    assert np.all(np.isfinite(dy))
    close(dy, d, 1e-12, "J-norm dots with other fixed entries")
    # psba_set_step ignores the fixed entries of dp
    p0 = _params(h)
    step = 1e-3 * rng.normal(size=x1.size)
    h.set_step(step)
    p1 = _params(h, capi.PARAMS_NEW)
    assert np.array_equal(p1[fx], p0[fx]) and np.array_equal(p1[~fx], (p0 + step)[~fx])
    h.close()


# ---- 9. structure-only -----------------------------------------------------------------------------------------------
def _structure_only_problem():
    base = _golden(54)
    rng = np.random.default_rng(9)
    return capi.Problem(base, pts=np.asarray(base["pts"]) + 1e-2 * rng.normal(size=np.asarray(base["pts"]).shape))


@pytest.mark.parametrize("shortcut", [True, False])
def test_structure_only_try(shortcut, monkeypatch):
    if not shortcut:
        monkeypatch.setenv("PSBA_FIXED_NO_SHORTCUT", "1")
    prob = _structure_only_problem()
    fc = np.ones(prob["nC"], dtype=np.uint8)
    t, _, lin = fixed_pieces(prob, fc, None)
    nA = 6 * prob["nC"]
    # the damping an LM loop starts with.  (The golden scene is 0.01 units across, so this perturbation leaves some
    # points next to a camera's principal plane: a few V_i are 1e16 times the median one.  max_diag itself is held
    # to 1e-12 on well-posed scenes in test_one_damping_try_against_twin, not here.)
    mu = 1e-3 * lin["maxdiag"]
    V = lin["V"].reshape(-1, 3, 3) + mu * np.eye(3)[None]
    want = np.linalg.solve(V, lin["g"][nA:].reshape(-1, 3, 1)).reshape(-1)
    h = _handle(prob, fc, None)
    assert h.fixed_counts() == (prob["nC"], 0)
    p0 = _params(h)
    h.linearize(1.0, 1.0)
    h.profile_enable(True)
    h.schur_assemble(mu)
    if shortcut:
        with pytest.raises(capi.PsbaError) as ei:  # nothing was assembled
            h.get_reduce_buffer()
        assert ei.value.code == -6
    else:
        h.get_reduce_buffer()
    h.schur_reduce()
    assert h.schur_solve() == 0
    sc = h.backsub(mu)
    assert sc.status == 0
    n_k2 = [h.profile_get(k)[1] for k in (capi.K_SCHUR, capi.K_SCHUR_REDUCE, capi.K_CHOLESKY)]
    assert (sum(n_k2) == 0) == shortcut, n_k2
    got = h.get_dp()
    assert np.all(got[:nA] == 0.0)
    print(f"structure-only, shortcut {shortcut}: dpb rel {np.abs(got[nA:] - want).max() / np.abs(want).max():.2e}")
    close(got[nA:], want, 1e-9, "dpb")
    p1 = _params(h, capi.PARAMS_NEW)
    assert np.array_equal(p1[:nA], p0[:nA])
    assert abs(sc.dp_l2 - want @ want) <= 1e-8 * (want @ want)
    h.close()


def test_structure_only_levmar_runs_no_schur_and_no_factorization():
    prob = _structure_only_problem()
    h = _handle(prob, np.ones(prob["nC"], dtype=np.uint8), None)
    p0 = _params(h)
    h.profile_enable(True)
    res, log = h.levmar(max_iter=10)
    counts = {capi.KERNEL_NAMES[k]: h.profile_get(k)[1] for k in range(7)}
    print(f"structure-only levmar(10): cost {res.init_err:.6e} -> {res.final_err:.6e}, launches {counts}")
    assert counts["schur"] == 0 and counts["schur_reduce"] == 0 and counts["cholesky"] == 0
    assert counts["linearize"] > 0 and counts["backsub"] > 0
    assert res.final_err < res.init_err
    nA = 6 * prob["nC"]
    p1 = _params(h)
    assert np.array_equal(p1[:nA], p0[:nA]) and not np.array_equal(p1[nA:], p0[nA:])
    # the cost reached is the twin's structure-only optimum
    want = FixedTwin(prob, np.ones(prob["nC"], dtype=bool), None).cost(p1[:nA], p1[nA:])
    assert abs(res.final_err - want) <= 1e-10 * want
    h.close()
