"""Marquardt diagonal damping on the free-intrinsics route (psba_set_damping) on the GPU, against the numpy
twin tests/damping_twin.py, the two camera blocks against each other, and the handle against itself.

Measures and tolerances are those of tests/test_gpu_freekd.py (scaled_errors, scaled_tol; dp 1e-6, new_cost 1e-7, dp_l2
1e-6, gain_den 1e-7; max_diag's 1e-11 for a stored diagonal entry), with d_r = sqrt(N_rr + mu D_r) in the place of
sqrt(N_rr + mu); the grouped case takes shared_ref.shared_tol, the same rule for the length of a group's sum."""
import functools

import numpy as np
import pytest

import shared_ref as sr
from damping_twin import DMAX, DMIN, IDENTITY, MARQUARDT, TwinDamp, damp_diag
from freekd_twin import BAL, CNP, many_obs_problem, ring_problem, start_kc, tiny_problem
from test_freekd_twin import P7, scaled_tol
from test_gpu_freekd import ALL, K_ONLY, handle, scaled_errors, split

pytestmark = pytest.mark.gpu
CLAMPS = {"default": (0.0, 0.0), "1e5": (1e-6, 1e5)}


@functools.lru_cache(maxsize=None)
def problem(name):
    """(problem, starting kc) -- made once, shared, never modified"""
    if name == "ring":
        start, kc0, _, _ = ring_problem()
        return start, kc0
    p = {"tiny": tiny_problem, "P7": P7, "many": many_obs_problem}[name]()
    return p, start_kc(p["nC"])


@functools.lru_cache(maxsize=None)
def twin_diag(name, free):
    p, kc = problem(name)
    d = TwinDamp(p, kc, free).diag_normal()
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def twin_normal(name, free):
    p, kc = problem(name)
    t = TwinDamp(p, kc, free)
    cost, N, g = t.normal()
    for a in (N, g):
        a.setflags(write=False)
    return t, cost, N, g


@functools.lru_cache(maxsize=None)
def twin_levmar(name, damping):
    p, kc = problem(name)
    return TwinDamp(p, kc, BAL).levmar(max_iter=8, damping=damping)


def marquardt(name, free, clamps=(0.0, 0.0)):
    import psba_amd
    p, kc = problem(name)
    h = handle(p, kc, free)
    h.set_damping(psba_amd.DAMPING_MARQUARDT, *clamps)
    return h


def check_diag(D, d, held, dmin, dmax):
    """D of the GPU against clamp(d) of the twin: 1e-11 relative where no clamp is active, the clamp itself -- exactly --
    where the twin's entry lies beyond it by more than that, clamp(1) on held coordinates"""
    want = damp_diag(d, dmin, dmax)
    err = np.abs(D - want) / want
    low, high = d < dmin * (1 - 1e-9), d > dmax * (1 + 1e-9)
    print(f"D: {err.max():.2e} relative; {int(low.sum())} entries at dmin, {int(high.sum())} at dmax")
    assert err.max() <= 1e-11
    assert np.all(D[low] == dmin) and np.all(D[high] == dmax)
    assert np.all(D[held] == min(max(1.0, dmin), dmax))
    return low, high


# ---- 1. D against the twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamps", ["default", "1e5"])
@pytest.mark.parametrize("free", [ALL, BAL], ids=["all", "bal"])
@pytest.mark.parametrize("name", ["tiny", "ring", "P7", "many"])
def test_diag_against_the_twin(name, free, clamps):
    p, _ = problem(name)
    dmin, dmax = CLAMPS[clamps]
    h = marquardt(name, free, (dmin, dmax))
    h.linearize(1.0, 1.0)
    D = h.get_damping_diag()
    h.close()
    d = twin_diag(name, free)
    held = np.flatnonzero(np.tile(np.r_[np.asarray(free) == 0, np.zeros(6, dtype=bool)], p["nC"]))
    low, high = check_diag(D, d, held, dmin or DMIN, dmax or DMAX)
    if name == "tiny" and free == ALL:
        assert low.sum() >= 2          # (test_damping_twin.py: the clamps are not idle on these inputs)
    if name == "ring" and clamps == "1e5":
        assert high.sum() >= 6


# ---- 2. one try against the twin -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", [1e-3, 1e-6])
@pytest.mark.parametrize("name,free,clamps", [("tiny", ALL, "default"), ("tiny", BAL, "default"), ("P7", ALL, "default"),
                                              ("P7", BAL, "default"), ("ring", BAL, "1e5")],
                         ids=["tiny-all", "tiny-bal", "P7-all", "P7-bal", "ring-bal-1e5"])
def test_one_try_against_the_twin(name, free, clamps, mu):
    p, _ = problem(name)
    dmin, dmax = CLAMPS[clamps]
    t, cost, N, g = twin_normal(name, free)
    nA, nT, tol = t.nA, t.nT, scaled_tol(p)
    held = np.flatnonzero(~t.free_a)
    D = damp_diag(N, dmin or DMIN, dmax or DMAX)
    h = marquardt(name, free, (dmin, dmax))
    h.linearize(1.0, 1.0)
    S_want, ea_want = t.schur(N, g, mu, D)
    h.schur_assemble(mu)
    S, ea = split(h, nA)
    d = np.sqrt(np.diag(N)[:nA] + mu * D[:nA])
    eS, ee = scaled_errors(S, ea, S_want, ea_want, d, np.sqrt(cost))
    print(f"{name} mu={mu:g}: S {eS:.2e}, e_a {ee:.2e} (tol {tol:.2e})")
    assert eS <= tol and ee <= tol
    # held coordinates: zero row and column, coeff + mu clamp(coeff) on the diagonal, e_a = 0
    off = S[held].copy()
    off[np.arange(held.size), held] = 0.0
    assert np.all(off == 0.0) and np.all(S[:, held][np.setdiff1d(np.arange(nA), held)] == 0.0)
    assert np.all(S[held, held] == 1.0 + mu * 1.0) and np.all(ea[held] == 0.0)
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    dp_want = np.linalg.solve(N + mu * np.diag(D), g)
    dp = h.get_dp()
    assert np.all(dp[:nA][held] == 0.0)
    for sl in (slice(0, nA), slice(nA, nT)):
        err = np.abs(dp[sl] - dp_want[sl]).max() / np.abs(dp_want[sl]).max()
        print(f"dp block {sl.start}: {err:.2e}")
        assert err <= 1e-6
    new_cost = t.cost(t.cams + dp_want[:nA].reshape(-1, CNP), t.pts + dp_want[nA:].reshape(-1, 3))
    gain = dp_want @ (mu * D * dp_want + g)
    print(f"new_cost {abs(sc.new_cost - new_cost) / new_cost:.2e}, dp_l2 "
          f"{abs(sc.dp_l2 - dp_want @ dp_want) / (dp_want @ dp_want):.2e}, gain_den {abs(sc.gain_den - gain) / abs(gain):.2e}")
    assert abs(sc.new_cost - new_cost) <= 1e-7 * new_cost
    assert abs(sc.dp_l2 - dp_want @ dp_want) <= 1e-6 * (dp_want @ dp_want)
    assert abs(sc.gain_den - gain) <= 1e-7 * abs(gain)
    cams_new, _ = h.get_params(1)
    cams_cur, _ = h.get_params(0)
    cols = np.flatnonzero(~t.free)
    assert np.array_equal(cams_new[:, cols], cams_cur[:, cols])   # the proposal leaves held intrinsics bit-identical
    h.close()


# ---- 3. groups -----------------------------------------------------------------------------------------------------
def test_groups_against_the_twin_of_J_P():
    """ring scene, cameras {0, 2, 4} and {1, 3} grouped, 5 alone, BAL mask: the reduced dense system P^T N P (embedded:
    a folded-away coordinate keeps the placeholder 1 and g = 0), D = clamp of ITS diagonal, mu D added once."""
    import psba_amd
    labels = np.array([0, 1, 0, 1, 0, 2])
    p0, kc0 = problem("ring")
    p, kc = sr.share_problem(p0, kc0, labels)
    rep = sr.representatives(labels)
    t = TwinDamp(p, kc, BAL)
    cost, N, g = t.normal()
    nA, nT = t.nA, t.nT
    phi, away = sr.fold_map(rep, BAL)
    phi_t = np.r_[phi, nA + np.arange(t.nB)]
    rows = np.zeros_like(N)
    np.add.at(rows, phi_t, N)
    Nf = np.zeros_like(N)
    np.add.at(Nf.T, phi_t, rows.T)
    aw = np.flatnonzero(away)
    Nf[aw, aw] = 1.0
    gf = np.bincount(phi_t, weights=g, minlength=nT)
    assert np.all(Nf[aw].sum(1) == 1.0) and np.all(gf[aw] == 0.0)
    held = np.flatnonzero(~t.free_a)
    D = damp_diag(Nf)
    mu = 1e-3
    h = handle(p, kc, BAL)
    h.set_damping(psba_amd.DAMPING_MARQUARDT)      # damping, then groups: they compose in any order
    h.set_intrinsics_groups(labels)
    assert h.damping()[0] == MARQUARDT and h.intrinsics_groups()[1] == 3
    h.linearize(1.0, 1.0)
    check_diag(h.get_damping_diag(), np.diag(Nf), np.r_[held, aw], DMIN, DMAX)
    S_want, ea_want = t.schur(Nf, gf, mu, D)
    h.schur_assemble(mu)
    buf = h.get_reduce_buffer().tobytes()
    S, ea = split(h, nA)
    tol = sr.shared_tol(p, labels)
    d = np.sqrt(np.diag(Nf)[:nA] + mu * D[:nA])
    eS, ee = scaled_errors(S, ea, S_want, ea_want, d, np.sqrt(cost))
    print(f"groups: S {eS:.2e}, e_a {ee:.2e} (tol {tol:.2e})")
    assert eS <= tol and ee <= tol
    sr.check_embedded(S, ea, away, 1.0 + mu * 1.0)
    sr.check_mirror(S)
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    dpe = np.linalg.solve(Nf + mu * np.diag(D), gf)       # embedded; the step of a member is its representative's
    dp_want = dpe[phi_t]
    dp = h.get_dp()
    assert np.all(dp[:nA][held] == 0.0) and np.array_equal(dp[:nA][aw], dp[:nA][phi[aw]])
    for sl in (slice(0, nA), slice(nA, nT)):
        err = np.abs(dp[sl] - dp_want[sl]).max() / np.abs(dp_want[sl]).max()
        print(f"dp block {sl.start}: {err:.2e}")
        assert err <= 1e-6
    gain = dpe @ (mu * D * dpe + gf)                       # a shared parameter counts once
    print(f"gain_den {abs(sc.gain_den - gain) / abs(gain):.2e}, dp_l2 {abs(sc.dp_l2 - dpe @ dpe) / (dpe @ dpe):.2e}")
    assert abs(sc.gain_den - gain) <= 1e-7 * abs(gain)
    assert abs(sc.dp_l2 - dpe @ dpe) <= 1e-6 * (dpe @ dpe)
    # the other order of calls gives the same bits
    h2 = handle(p, kc, BAL)
    h2.set_intrinsics_groups(labels)
    h2.set_damping(psba_amd.DAMPING_MARQUARDT)
    h2.linearize(1.0, 1.0)
    h2.schur_assemble(mu)
    assert h2.get_reduce_buffer().tobytes() == buf
    h2.close()
    # members that start bit-identical stay so
    h.reset_params()
    res, _ = h.levmar(max_iter=3, tr_handoff=False, log_cap=64)
    cams, _ = h.get_params()
    assert res.iters == 3 and res.final_err < res.init_err
    assert np.array_equal(cams[:, :10], cams[rep][:, :10])
    assert not np.array_equal(cams[:, 0], np.asarray(p["K"]).reshape(-1, 5)[:, 0])
    h.close()


# ---- 4. blocks of 11 -----------------------------------------------------------------------------------------------
def test_blocks_of_eleven_against_blocks_of_sixteen():
    """7camsvarK: PSBA_CAMERA_FREE_K against PSBA_CAMERA_FREE_KD with the five intrinsics free and kc = 0 held, both
    under Marquardt (the comparison of test_gpu_freekd.py::test_against_the_eleven_block_route)."""
    import psba_amd
    p = P7()
    t = TwinDamp(p, None, K_ONLY)
    cost, N, g = t.normal()
    h = handle(p, None, K_ONLY)
    h.set_damping(psba_amd.DAMPING_MARQUARDT)
    h11 = psba_amd.Psba(0)
    h11.set_camera_model(psba_amd.CAMERA_FREE_K)
    h11.upload_problem(p)
    h11.set_damping(psba_amd.DAMPING_MARQUARDT)
    assert h11.camera_block() == 11 and h11.damping() == (MARQUARDT, DMIN, DMAX)
    h.linearize(1.0, 1.0)
    h11.linearize(1.0, 1.0)
    mu = 1e-3
    h.schur_assemble(mu)
    h11.schur_assemble(mu)
    nC = p["nC"]
    S, ea = split(h, t.nA)
    S11, ea11 = split(h11, 11 * nC)
    D, D11 = h.get_damping_diag(), h11.get_damping_diag()
    rows = (CNP * np.arange(nC)[:, None] + np.r_[0:5, 10:16][None, :]).reshape(-1)
    tol = 2 * scaled_tol(p)
    d = np.sqrt(np.diag(N)[:t.nA] + mu * damp_diag(N)[:t.nA])[rows]
    eS, ee = scaled_errors(S[np.ix_(rows, rows)], ea[rows], S11, ea11, d, np.sqrt(cost))
    eD = (np.abs(np.r_[D[rows], D[t.nA:]] - D11) / D11).max()
    print(f"16 against 11: S {eS:.2e}, e_a {ee:.2e}, D {eD:.2e} (tol {tol:.2e})")
    assert eS <= tol and ee <= tol and eD <= tol
    h.close()
    h11.close()


# ---- 5. psba_levmar against the twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P7", "ring"])
def test_levmar_against_the_twin(name):
    """psba_levmar as a caller runs it (default options but the length, as test_gpu_freekd.py's test of the same name):
    mu_0 = tau exactly; the first min(len, 6) log rows have the twin's accept flags and its costs at rtol = 1e-6.

    On the noise-free ring scene the loop's absolute stop (cost <= 1e-12) ends both runs after the fifth iteration, at
    3.5e-14 of 3.8e4, so that log has five rows: the stop is there to end such a problem before fp64 is used up.
    Without it (test_ring_headline's run) a sixth row exists, 1.219993e-19 on the MI355X against the twin's
    1.220089e-19, 7.8e-5 apart, where the twin itself gives 1.219777e-19 under another BLAS (2.6e-4): a sum of about
    1150 squared residuals of 1e-11 pixels, each the difference of two numbers of a few hundred pixels known to
    4e-14, is not defined to 1e-6.  That row is held by test_ring_headline's bounds, not by this comparison."""
    want, wlog = twin_levmar(name, MARQUARDT)
    h = marquardt(name, BAL)
    res, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
    h.reset_params()
    res2, _ = h.levmar(max_iter=1, tr_handoff=False, init_mu=0.25)
    h.close()
    assert res.mu0 == 1e-3 == want.mu0
    assert res2.mu0 == 0.25                                   # tau itself, not tau max diag
    assert abs(res.init_err - want.init_err) <= 1e-12 * want.init_err
    assert (res.iters, res.tries, len(log)) == (want.iters, want.tries, len(wlog))
    assert (res.flag == 6) == (want.flag == 3) == (name == "ring")   # PSBA_ITER_ERR_SMALL_ENOUGH / the twin's code for it
    n = min(len(log), len(wlog), 6)
    print(np.c_[log[:n, 1], wlog[:n, 1], np.abs(log[:n, 1] / wlog[:n, 1] - 1), log[:n, 4], wlog[:n, 4]])
    assert n >= 4
    assert np.array_equal(log[:n, 4], wlog[:n, 4])
    np.testing.assert_allclose(log[:n, 1], wlog[:n, 1], rtol=1e-6)


def test_ring_headline():
    """8 iterations without the absolute stop: Marquardt reaches 1e-15 of the initial cost and recovers f, k1, k2
    inside the bounds of test_gpu_freekd.py::test_recovery_of_the_ring_scene (which takes 18 to 30 iterations under
    mu I); the identity run of the same handle and length ends at least 1e6 times higher."""
    import psba_amd
    _, _, K_true, kc_true = ring_problem()
    h = marquardt("ring", BAL)
    res, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256, stop_cost=-1.0)
    cams, _ = h.get_params()
    f = np.abs(cams[:, 0] / K_true[:, 0] - 1).max()
    k1 = np.abs(cams[:, 5] - kc_true[:, 0]).max()
    k2 = np.abs(cams[:, 6] - kc_true[:, 1]).max()
    h.set_damping(psba_amd.DAMPING_IDENTITY)
    h.reset_params()
    ires, ilog = h.levmar(max_iter=8, tr_handoff=False, log_cap=256, stop_cost=-1.0)
    h.close()
    print(f"Marquardt: {res.iters} iterations, {res.tries} tries, cost {res.final_err:.3e} of {res.init_err:.3e}, "
          f"f {f:.2e}, k1 {k1:.2e}, k2 {k2:.2e}; identity: {ires.iters} iterations, {ires.tries} tries, "
          f"cost {ires.final_err:.3e}")
    assert res.final_err <= 1e-15 * res.init_err
    assert f <= 1e-9 and k1 <= 1e-8 and k2 <= 1e-7
    assert ires.final_err >= 1e6 * res.final_err


# ---- 6. determinism and identity -----------------------------------------------------------------------------------
def test_two_marquardt_runs_are_bit_identical():
    h = marquardt("P7", BAL)
    out = []
    for _ in range(2):
        h.reset_params()
        res, log = h.levmar(max_iter=6, tr_handoff=False, log_cap=256)
        cams, pts = h.get_params()
        h.linearize(1.0, 1.0)
        h.schur_assemble(res.mu_final)
        out.append((log.tobytes(), cams.tobytes(), pts.tobytes(), h.get_reduce_buffer().tobytes()))
    h.close()
    assert out[0] == out[1] and len(out[0][0]) > 0


def test_identity_after_marquardt_is_the_handle_that_never_set_a_damping():
    import psba_amd
    p, kc = problem("P7")

    def identity_outputs(h):
        h.reset_params()
        h.linearize(1.0, 1.0)
        h.schur_assemble(1e-3 * h.max_diag())
        buf = h.get_reduce_buffer().tobytes()
        h.reset_params()
        res, log = h.levmar(max_iter=6, tr_handoff=False, log_cap=256)
        return buf, log.tobytes(), res.mu0, h.get_params()[0].tobytes()

    fresh = handle(p, kc, BAL)
    want = identity_outputs(fresh)
    fresh.close()
    h = marquardt("P7", BAL, CLAMPS["1e5"])
    h.levmar(max_iter=4, tr_handoff=False)
    h.set_damping(psba_amd.DAMPING_IDENTITY)
    assert h.damping() == (IDENTITY, DMIN, DMAX)
    got = identity_outputs(h)
    h.close()
    assert got == want and len(want[1]) > 0


# ---- 7. look-ahead -------------------------------------------------------------------------------------------------
def test_the_diagonal_follows_the_look_ahead():
    import psba_amd
    h = marquardt("P7", BAL)
    cost, _ = h.begin()
    h.linearize(1.0, 1.0)
    D0 = h.get_damping_diag()

    def a_try(mu):
        h.schur_assemble(mu)
        h.schur_reduce()
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        return h.backsub_wait()

    # a step the host does not take: the second set was written, the current one is as it was
    sc = a_try(10.0)
    assert sc.status == 0
    assert h.get_damping_diag().tobytes() == D0.tobytes()
    # ... and one it takes
    sc = a_try(1e-3)
    assert sc.status == 0 and sc.new_cost < cost
    assert h.get_damping_diag().tobytes() == D0.tobytes()
    cams, pts = h.get_params(1)
    h.accept()
    D1 = h.get_damping_diag()
    h.linearize(1.0, 1.0)                      # (nothing left to do: the linearization came with the accept)
    assert h.get_damping_diag().tobytes() == D1.tobytes() != D0.tobytes()
    h2 = marquardt("P7", BAL)
    h2.set_params(cams, pts)
    h2.linearize(1.0, 1.0)
    assert h2.get_damping_diag().tobytes() == D1.tobytes()
    # a proposal that was not linearized ahead takes no diagonal with it
    h2.schur_assemble(1e-3)
    h2.schur_solve()
    h2.backsub(1e-3)
    h2.accept()
    with pytest.raises(psba_amd.PsbaError) as ei:
        h2.get_damping_diag()
    assert ei.value.code == -6
    h.close()
    h2.close()


# ---- 8. interface --------------------------------------------------------------------------------------------------
def test_interface():
    import psba_amd
    p, kc = problem("P7")

    def refused(call, code, *texts):
        with pytest.raises(psba_amd.PsbaError) as ei:
            call()
        assert ei.value.code == code, str(ei.value)
        for s in texts:
            assert s in str(ei.value), str(ei.value)

    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    refused(lambda: h.set_damping(psba_amd.DAMPING_MARQUARDT), -6, "psba_set_damping", "no problem uploaded")
    refused(lambda: h.damping(), -6)
    refused(lambda: h.get_damping_diag(), -6)
    h.upload_problem(p)
    h.set_distortion(kc)
    assert (psba_amd.DAMPING_IDENTITY, psba_amd.DAMPING_MARQUARDT) == (0, 1) == (IDENTITY, MARQUARDT)
    assert h.damping() == (IDENTITY, 1e-6, 1e32)
    # the getter round-trips, zero clamps report the defaults
    h.set_damping(MARQUARDT, 1e-3, 1e7)
    assert h.damping() == (MARQUARDT, 1e-3, 1e7)
    h.set_damping(MARQUARDT, 0.0, 1e7)
    assert h.damping() == (MARQUARDT, 1e-6, 1e7)
    h.set_damping(MARQUARDT, 2.5, 2.5)
    assert h.damping() == (MARQUARDT, 2.5, 2.5)
    h.set_damping(MARQUARDT)
    assert h.damping() == (MARQUARDT, 1e-6, 1e32)
    # refused arguments change nothing
    h.set_damping(MARQUARDT, 1e-3, 1e7)
    for bad in ((2, 0.0, 0.0), (-1, 0.0, 0.0), (MARQUARDT, 1e3, 1e2), (MARQUARDT, -1e-6, 1.0), (MARQUARDT, 1e-6, -1.0),
                (MARQUARDT, np.nan, 1.0), (MARQUARDT, 1e-6, np.inf), (MARQUARDT, np.inf, np.inf), (IDENTITY, 2.0, 1.0)):
        refused(lambda: h.set_damping(*bad), -1, "psba_set_damping")
    assert h.damping() == (MARQUARDT, 1e-3, 1e7)
    # the diagonal: after a linearization under Marquardt, until the parameters or the model change
    refused(lambda: h.get_damping_diag(), -6, "psba_linearize")
    h.linearize(1.0, 1.0)
    D = h.get_damping_diag()
    assert D.shape == (h.nT,) and D.min() >= 1e-3 and D.max() <= 1e7
    cams, pts = h.get_params()
    for change in (lambda: h.set_params(cams, pts), lambda: h.reset_params(), lambda: h.set_intrinsics_mask(BAL),
                   lambda: h.set_distortion(kc), lambda: h.set_intrinsics_groups(None),
                   lambda: h.set_damping(MARQUARDT, 1e-3, 1e7)):
        h.linearize(1.0, 1.0)
        h.get_damping_diag()
        change()
        refused(lambda: h.get_damping_diag(), -6)
    h.set_damping(IDENTITY)
    h.linearize(1.0, 1.0)
    refused(lambda: h.get_damping_diag(), -6, "PSBA_DAMPING_MARQUARDT")
    # setting it discards what was linearized
    refused(lambda: (h.set_damping(MARQUARDT), h.schur_assemble(1e-3)), -6, "psba_linearize")
    # refused while a try is in flight, and then nothing changes
    h.linearize(1.0, 1.0)
    h.schur_assemble(1e-3)
    h.schur_solve()
    h.backsub_async(1e-3)
    refused(lambda: h.set_damping(IDENTITY), -6, "psba_set_damping", "in flight")
    h.backsub_wait()
    assert h.damping() == (MARQUARDT, 1e-6, 1e32)
    # a new upload resets to identity with the default clamps
    h.set_damping(MARQUARDT, 1e-3, 1e7)
    h.upload_problem(p)
    assert h.damping() == (IDENTITY, 1e-6, 1e32)
    h.linearize(1.0, 1.0)
    refused(lambda: h.get_damping_diag(), -6)
    h.close()
    # six-parameter blocks keep mu I and say so
    h6 = psba_amd.Psba(0)
    h6.upload_problem(p)
    refused(lambda: h6.set_damping(MARQUARDT), -6, "psba_set_damping", "free-intrinsics models only")
    refused(lambda: h6.damping(), -6)
    refused(lambda: h6.get_damping_diag(), -6)
    h6.close()
