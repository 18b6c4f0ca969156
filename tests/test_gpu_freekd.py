"""PSBA_CAMERA_FREE_KD on the GPU: camera blocks of 16 (intrinsics, distortion, pose) with a mask over the ten
intrinsics, against the numpy twin tests/freekd_twin.py, the 11-block route, the fixed-K route and itself.

S and e_a are compared entry by entry in the scale of their own row and column: |dS_rc| <= tol d_r d_c and
|de_a,r| <= tol d_r ||e|| with d_r = sqrt(N_rr + mu) (the entries span 1e0 ... 1e12: a comparison relative to max |S|
would not see the intrinsic blocks) and tol = 64 eps (largest observation count of one camera + 16), the bound of a
sum of that length with a safety of 64.  The twin's own rounding in this measure is below 1e-15
(test_freekd_twin.py::test_twin_sums_against_extended_precision)."""
import functools

import numpy as np
import pytest

import freekd_twin
from freekd_twin import BAL, CNP, TwinKD, ring_problem, start_kc, tiny_problem
from test_freekd_twin import P7, P54, scaled_tol

pytestmark = pytest.mark.gpu
ALL = (1,) * 10
K_ONLY = (1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
NONE = (0,) * 10
PROBLEMS = {"tiny": tiny_problem, "P7": P7, "P54": P54}


@functools.lru_cache(maxsize=None)
def prob(name):
    return PROBLEMS[name]()


@functools.lru_cache(maxsize=None)
def twin_normal(name, free, zero_kc=False):
    """(twin, cost, N, g) at the start: computed once, shared, never modified"""
    p = prob(name)
    t = TwinKD(p, None if zero_kc else start_kc(p["nC"]), free)
    cost, N, g = t.normal()
    for a in (N, g):
        a.setflags(write=False)
    return t, cost, N, g


@functools.lru_cache(maxsize=None)
def twin_levmar(name, free, max_iter):
    p = prob(name)
    return TwinKD(p, start_kc(p["nC"]), free).levmar(max_iter=max_iter)


def handle(p, kc, free, env=None):
    import psba_amd
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(p)
    if kc is not None:
        h.set_distortion(kc)
    h.set_intrinsics_mask(free)
    return h


def split(h, nA):
    n32 = (nA + 31) // 32 * 32
    M = h.get_reduce_buffer().reshape(n32 + 1, n32)
    return M[:nA, :nA], M[n32, :nA]


def scaled_errors(S, ea, S_want, ea_want, d, enorm):
    return (np.abs(S - S_want) / np.outer(d, d)).max(), (np.abs(ea - ea_want) / (d * enorm)).max()


def one_try(h, name, free, which_mu):
    """One damping try of handle h against the twin; returns (S, e_a, mu) of the GPU."""
    t, cost, N, g = twin_normal(name, free)
    p, nA, nT = prob(name), t.nA, t.nT
    tol = scaled_tol(p)
    held = np.flatnonzero(~t.free_a)
    assert abs(h.residual() - cost) <= 1e-12 * cost
    h.linearize(1.0, 1.0)
    maxdiag = h.max_diag()
    assert abs(maxdiag - t.max_diag(N)) <= 1e-11 * maxdiag      # over the free entries only
    mu = 1e-3 * t.max_diag(N) if which_mu == "big" else 1e-6 * float(np.median(np.diag(N)))
    gg = h.get_gradient()
    assert np.all(gg[:nA][held] == 0.0)
    d_all = np.sqrt(np.diag(N))
    print(f"g: {(np.abs(gg - g) / (d_all * np.sqrt(cost))).max():.2e}")
    assert np.all(np.abs(gg - g) <= tol * d_all * np.sqrt(cost))
    S_want, ea_want = t.schur(N, g, mu)
    h.schur_assemble(mu)
    S, ea = split(h, nA)
    d = np.sqrt(np.diag(N)[:nA] + mu)
    eS, ee = scaled_errors(S, ea, S_want, ea_want, d, np.sqrt(cost))
    print(f"{name} free={free} mu={mu:.3e}: S {eS:.2e}, e_a {ee:.2e} (tol {tol:.2e})")
    assert eS <= tol and ee <= tol
    # masked coordinates: zero row and column, the placeholder coeff + mu on the diagonal, e_a = 0
    off = S[held].copy()
    off[np.arange(held.size), held] = 0.0
    assert np.all(off == 0.0) and np.all(S[:, held][np.setdiff1d(np.arange(nA), held)] == 0.0)
    assert np.all(S[held, held] == 1.0 + mu) and np.all(ea[held] == 0.0)
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    dp_want = np.linalg.solve(N + mu * np.eye(nT), g)
    dp = h.get_dp()
    assert np.all(dp[:nA][held] == 0.0)
    for sl in (slice(0, nA), slice(nA, nT)):
        err = np.abs(dp[sl] - dp_want[sl]).max() / np.abs(dp_want[sl]).max()
        print(f"dp block {sl.start}: {err:.2e}")
        assert err <= 1e-6
    new_cost = t.cost(t.cams + dp_want[:nA].reshape(-1, CNP), t.pts + dp_want[nA:].reshape(-1, 3))
    assert abs(sc.new_cost - new_cost) <= 1e-7 * new_cost
    assert abs(sc.dp_l2 - dp_want @ dp_want) <= 1e-6 * (dp_want @ dp_want)
    assert abs(sc.gain_den - dp_want @ (mu * dp_want + g)) <= 1e-7 * abs(dp_want @ (mu * dp_want + g))
    cams_new, _ = h.get_params(1)
    cams_cur, _ = h.get_params(0)
    cols = np.flatnonzero(~t.free)
    assert np.array_equal(cams_new[:, cols], cams_cur[:, cols])   # the proposal leaves held intrinsics bit-identical
    return S, ea, mu


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("free", [ALL, BAL], ids=["all", "bal"])
@pytest.mark.parametrize("name", ["tiny", "P7", "P54"])
def test_one_damping_try_against_the_twin(name, free, which_mu):
    p = prob(name)
    h = handle(p, start_kc(p["nC"]), free)
    assert h.schur_path() == 5
    one_try(h, name, free, which_mu)
    h.close()


def test_segmented_blocks(monkeypatch):
    """PSBA_FKD_SEG=3 cuts almost every block of P7 into many segments (partial tiles, summed in segment order)."""
    p = prob("P7")
    kc = start_kc(p["nC"])
    h = handle(p, kc, BAL)
    monkeypatch.setenv("PSBA_FKD_SEG", "3")
    h3 = handle(p, kc, BAL)
    monkeypatch.delenv("PSBA_FKD_SEG")
    S, ea, mu = one_try(h, "P7", BAL, "small")
    S3, ea3, _ = one_try(h3, "P7", BAL, "small")
    t, cost, N, g = twin_normal("P7", BAL)
    eS, ee = scaled_errors(S3, ea3, S, ea, np.sqrt(np.diag(N)[:t.nA] + mu), np.sqrt(cost))
    print(f"L = 3 against the default: S {eS:.2e}, e_a {ee:.2e}")
    assert eS <= scaled_tol(p) and ee <= scaled_tol(p)
    h.close()
    h3.close()


def test_two_runs_are_bit_identical():
    p = prob("P54")
    kc = start_kc(p["nC"])
    bufs, logs = [], []
    for _ in range(2):
        h = handle(p, kc, BAL)
        h.linearize(1.0, 1.0)
        h.schur_assemble(1e-3 * h.max_diag())
        bufs.append(h.get_reduce_buffer().tobytes())
        h.reset_params()
        res, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
        logs.append(log.tobytes())
        h.close()
    assert bufs[0] == bufs[1]
    assert logs[0] == logs[1] and len(logs[0]) > 0


def test_four_handles_of_three_camera_blocks_share_no_state():
    """Handles of blocks 16, 11, 6 and 11 alive at once on 7camsvarK, the verbs of one damping try interleaved over
    them: the two instantiations of kernels_free.hip and the six-parameter kernels keep no state outside their
    handle.  The two 11-block handles agree bit for bit; the 16-block handle meets this module's tolerances against
    the twin, the six-parameter one test_gpu_parity.py's against the oracle."""
    import psba_amd
    from oracle_lib import Oracle
    p = prob("P7")
    t, cost, N, g = twin_normal("P7", ALL)
    o = Oracle(p)
    lin = o.linearize()
    hs = [handle(p, start_kc(p["nC"]), ALL)]
    for model in (psba_amd.CAMERA_FREE_K, psba_amd.CAMERA_FIXED_K, psba_amd.CAMERA_FREE_K):
        h = psba_amd.Psba(0)
        h.set_camera_model(model)
        h.upload_problem(p)
        hs.append(h)
    assert [h.camera_block() for h in hs] == [16, 11, 6, 11]
    begun = [h.begin() for h in hs]
    mus = [1e-3 * t.max_diag(N), 1e-3 * begun[1][1], 1e-3 * lin["maxdiag"], 1e-3 * begun[3][1]]
    for h, mu in zip(hs, mus):
        h.schur_assemble(mu)
    reds = [h.get_reduce_buffer() for h in (hs[0], hs[1], hs[3])]
    for h in hs:
        h.schur_reduce()
    for h in hs:
        h.schur_solve()
    scs = [h.backsub(mu) for h, mu in zip(hs, mus)]
    dps = [h.get_dp() for h in hs]
    for h in hs:
        h.close()
    assert all(sc.status == 0 for sc in scs)
    # blocks of 11, twice
    assert begun[1] == begun[3] and reds[1].tobytes() == reds[2].tobytes() and dps[1].tobytes() == dps[3].tobytes()
    assert all(getattr(scs[1], f) == getattr(scs[3], f) for f, _ in scs[1]._fields_)
    # blocks of 16 against the twin (one_try's measures)
    nA, nT, mu = t.nA, t.nT, mus[0]
    assert abs(begun[0][0] - cost) <= 1e-12 * cost and abs(begun[0][1] - t.max_diag(N)) <= 1e-11 * begun[0][1]
    n32 = (nA + 31) // 32 * 32
    M = reds[0].reshape(n32 + 1, n32)
    S_want, ea_want = t.schur(N, g, mu)
    eS, ee = scaled_errors(M[:nA, :nA], M[n32, :nA], S_want, ea_want, np.sqrt(np.diag(N)[:nA] + mu), np.sqrt(cost))
    assert eS <= scaled_tol(p) and ee <= scaled_tol(p)
    dp_want = np.linalg.solve(N + mu * np.eye(nT), g)
    for sl in (slice(0, nA), slice(nA, nT)):
        assert np.abs(dps[0][sl] - dp_want[sl]).max() <= 1e-6 * np.abs(dp_want[sl]).max()
    new_cost = t.cost(t.cams + dp_want[:nA].reshape(-1, CNP), t.pts + dp_want[nA:].reshape(-1, 3))
    assert abs(scs[0].new_cost - new_cost) <= 1e-7 * new_cost
    assert abs(scs[0].dp_l2 - dp_want @ dp_want) <= 1e-6 * (dp_want @ dp_want)
    assert abs(scs[0].gain_den - dp_want @ (mu * dp_want + g)) <= 1e-7 * abs(dp_want @ (mu * dp_want + g))
    # blocks of 6 against the oracle (test_gpu_parity.py: dp 1e-9 of the largest entry, the try's scalars 1e-8)
    mu = mus[2]
    assert abs(begun[2][0] - lin["ex"] @ lin["ex"]) <= 1e-12 * begun[2][0]
    assert abs(begun[2][1] - lin["maxdiag"]) <= 1e-12 * lin["maxdiag"]
    _, dp6, _ = o.solve(lin, o.schur(lin, mu))
    assert np.abs(dps[2] - dp6).max() <= 1e-9 * np.abs(dp6).max()
    newp = np.r_[o.cams, o.pts] + dp6
    ex_new = o.exQT(cams=newp[: o.nA], pts=newp[o.nA:])
    for got, want in [(scs[2].dp_l2, dp6 @ dp6), (scs[2].gain_den, dp6 @ (mu * dp6 + lin["g"])),
                      (scs[2].new_cost, ex_new @ ex_new), (scs[2].newp_l2, newp @ newp)]:
        assert abs(got - want) <= 1e-8 * abs(want), (got, want)


def test_against_the_eleven_block_route():
    """kc = 0 held, the five intrinsics free: the 11 x 11 sub-blocks are the FREE_K route's (twice the tolerance: the
    same again for that route's atomics)."""
    import psba_amd
    p = prob("P7")
    t, cost, N, g = twin_normal("P7", K_ONLY, True)
    h = handle(p, None, K_ONLY)
    h11 = psba_amd.Psba(0)
    h11.set_camera_model(True)
    h11.upload_problem(p)
    h.linearize(1.0, 1.0)
    h11.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h11.schur_assemble(mu)
    S, ea = split(h, t.nA)
    S11, ea11 = split(h11, 11 * p["nC"])
    rows = (CNP * np.arange(p["nC"])[:, None] + np.r_[0:5, 10:16][None, :]).reshape(-1)
    d = np.sqrt(np.diag(N)[:t.nA] + mu)[rows]
    eS, ee = scaled_errors(S[np.ix_(rows, rows)], ea[rows], S11, ea11, d, np.sqrt(cost))
    print(f"against FREE_K: S {eS:.2e}, e_a {ee:.2e} (tol {2 * scaled_tol(p):.2e})")
    assert eS <= 2 * scaled_tol(p) and ee <= 2 * scaled_tol(p)
    h.reset_params()
    h11.reset_params()
    _, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
    _, log11 = h11.levmar(max_iter=8, tr_handoff=False, log_cap=256)
    assert len(log) >= 6 and len(log11) >= 6
    assert np.array_equal(log[:6, 4], log11[:6, 4])
    np.testing.assert_allclose(log[:6, 1], log11[:6, 1], rtol=1e-6)
    h.close()
    h11.close()


@functools.lru_cache(maxsize=None)
def all_masked_run(name):
    """8 LM iterations with all ten intrinsics held: (final cost, start cameras, final cameras)"""
    p = prob(name)
    h = handle(p, start_kc(p["nC"]), NONE)
    c0, _ = h.get_params()
    res, _ = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
    c1, _ = h.get_params()
    h.close()
    return res.final_err, c0, c1


def test_against_the_fixed_k_route():
    """All ten intrinsics held at a non-zero kc: the 6 x 6 extrinsic sub-blocks are the fixed-K route's with
    set_distortion(kc); the LM ends at the same cost and never touches columns 0..9."""
    import psba_amd
    p = prob("P7")
    kc = start_kc(p["nC"])
    t, cost, N, g = twin_normal("P7", NONE)
    h = handle(p, kc, NONE)
    h6 = psba_amd.Psba(0)
    h6.upload_problem(p)
    h6.set_distortion(kc)
    h.linearize(1.0, 1.0)
    h6.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h6.schur_assemble(mu)
    S, ea = split(h, t.nA)
    S6, ea6 = split(h6, 6 * p["nC"])
    rows = (CNP * np.arange(p["nC"])[:, None] + np.arange(10, 16)[None, :]).reshape(-1)
    d = np.sqrt(np.diag(N)[:t.nA] + mu)[rows]
    eS, ee = scaled_errors(S[np.ix_(rows, rows)], ea[rows], S6, ea6, d, np.sqrt(cost))
    print(f"against fixed K: S {eS:.2e}, e_a {ee:.2e} (tol {2 * scaled_tol(p):.2e})")
    assert eS <= 2 * scaled_tol(p) and ee <= 2 * scaled_tol(p)
    h6.reset_params()
    res6, _ = h6.levmar(max_iter=8, tr_handoff=False)
    final, c0, c1 = all_masked_run("P7")
    assert abs(final - res6.final_err) <= 1e-6 * res6.final_err
    assert np.array_equal(c0[:, :10], c1[:, :10]) and not np.array_equal(c0[:, 10:], c1[:, 10:])
    assert np.array_equal(c0[:, 5:10], kc)
    h.close()
    h6.close()


@pytest.mark.parametrize("name", ["P7", "P54"])
def test_levmar_against_the_twin(name):
    p = prob(name)
    want, wlog = twin_levmar(name, BAL, 8)
    h = handle(p, start_kc(p["nC"]), BAL)
    res, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
    assert abs(res.init_err - want.init_err) <= 1e-12 * want.init_err
    n = min(len(log), len(wlog), 6)
    assert n >= 4
    np.testing.assert_allclose(log[:n, 1], wlog[:n, 1], rtol=1e-6)
    assert np.array_equal(log[:n, 4], wlog[:n, 4])
    assert abs(res.final_err - want.final_err) <= 1e-5 * want.final_err
    assert res.final_err <= all_masked_run(name)[0] * (1 + 1e-9)   # more freedom must not end above less
    cams, _ = h.get_params()
    held = [k for k in range(10) if not BAL[k]]
    assert np.array_equal(cams[:, held], np.hstack([np.asarray(p["K"]).reshape(-1, 5), start_kc(p["nC"])])[:, held])
    assert np.abs(cams[:, 0] - np.asarray(p["K"]).reshape(-1, 5)[:, 0]).max() > 0
    h.close()


def test_recovery_of_the_ring_scene():
    """Exact projections, BAL mask, 30 iterations; the bounds on the cost, f, k1 and k2 are the ones set for this test,
    which assume an LM that runs until fp64 is used up (the numpy twin without the absolute stop reaches f 9e-15,
    k1 1e-13, k2 2e-12 at iteration 21).  psba_levmar's default absolute stop (cost <= 1e-12, in squared pixels) ends
    this noise-free scene at iteration 18 with cost 2.2e-13 of 3.8e4, f 4.4e-9, k1 6.0e-8, k2 7.5e-7 -- as the twin
    with the same rule does -- so the run asks for no absolute stop (psba_lm_options.stop_cost < 0).  The second run
    pins the default: it ends on that test, above the first run's cost."""
    start, kc0, K_true, kc_true = ring_problem()
    h = handle(start, kc0, BAL)
    res, log = h.levmar(max_iter=30, tr_handoff=False, log_cap=256, stop_cost=-1.0)
    cams, _ = h.get_params()
    f = np.abs(cams[:, 0] / K_true[:, 0] - 1).max()
    k1 = np.abs(cams[:, 5] - kc_true[:, 0]).max()
    k2 = np.abs(cams[:, 6] - kc_true[:, 1]).max()
    print(f"iterations {res.iters} flag {res.flag}: cost {res.final_err:.3e} of {res.init_err:.3e}, f {f:.2e}, "
          f"k1 {k1:.2e}, k2 {k2:.2e}")
    h.reset_params()
    dres, _ = h.levmar(max_iter=30, tr_handoff=False, log_cap=256)
    print(f"default stop: iterations {dres.iters} flag {dres.flag}: cost {dres.final_err:.3e}")
    h.close()
    assert res.final_err <= 1e-15 * res.init_err
    assert f <= 1e-9 and k1 <= 1e-8 and k2 <= 1e-7
    assert dres.flag == 6 and res.final_err < dres.final_err <= 1e-12 and dres.iters <= res.iters


def test_interface():
    import psba_amd
    p = prob("P7")
    kc = start_kc(p["nC"])
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(p)
    assert h.camera_block() == 16 and h.nA == 16 * p["nC"] and h.schur_path() == 5
    assert h.lens_model() == (True, False)
    cams, pts = h.get_params()
    assert cams.shape == (p["nC"], 16) and np.all(cams[:, 5:10] == 0.0)
    assert np.array_equal(cams[:, :5], np.asarray(p["K"]).reshape(-1, 5))
    assert np.array_equal(cams[:, 10:], np.asarray(p["cams"]).reshape(-1, 6))
    h.set_distortion(kc)
    moved = cams + 1e-3
    h.set_params(moved, pts)
    assert np.array_equal(h.get_params()[0], moved)
    h.reset_params()
    assert np.array_equal(h.get_params()[0][:, 5:10], kc)          # the starting kc survives reset_params
    h.set_distortion(None)
    assert np.all(h.get_params()[0][:, 5:10] == 0.0)
    # the mask round-trips, NULL means all free, a new upload resets it
    assert h.intrinsics_mask() == ALL
    h.set_intrinsics_mask(psba_amd.INTRINSICS_BAL)
    assert h.intrinsics_mask() == BAL == psba_amd.INTRINSICS_BAL
    h.set_intrinsics_mask(NONE)
    assert h.intrinsics_mask() == NONE
    h.set_intrinsics_mask(None)
    assert h.intrinsics_mask() == ALL
    h.set_intrinsics_mask(BAL)
    h.upload_problem(p)
    assert h.intrinsics_mask() == ALL
    # refused while a try is in flight, and then nothing changes
    h.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h.schur_solve()
    h.backsub_async(mu)
    for call in (lambda: h.set_intrinsics_mask(BAL), lambda: h.set_distortion(kc)):
        with pytest.raises(psba_amd.PsbaError) as ei:
            call()
        assert ei.value.code == -6 and "in flight" in str(ei.value)
    h.backsub_wait()
    assert h.intrinsics_mask() == ALL and np.all(h.get_params()[0][:, 5:10] == 0.0)
    # what this route does not offer says so, naming the model
    refused = [lambda: h.set_obs_covariance(np.tile(np.eye(2), (p["nO"], 1, 1))), lambda: h.set_robust_loss(1, 1.0),
               lambda: h.set_fixed(np.r_[1, np.zeros(p["nC"] - 1)], None), lambda: h.compute_S(),
               lambda: h.compute_exQT(), lambda: h.jmul_dots(np.zeros(h.nT)), lambda: h.compute_Jmultiply(np.zeros(h.nT)),
               lambda: h.trust_region(max_iter=2), lambda: h.solve(max_iter=2), lambda: h.obs_sq_residuals(),
               lambda: h.set_rank_layout(2, 0)]
    for call in refused:
        with pytest.raises(psba_amd.PsbaError) as ei:
            call()
        assert "PSBA_CAMERA_FREE_KD" in str(ei.value)
    h.close()
    hp = psba_amd.Psba(0)
    hp.set_camera_model(psba_amd.CAMERA_FREE_KD)
    hp.set_solver(1)
    with pytest.raises(psba_amd.PsbaError) as ei:
        hp.upload_problem(p)
    assert "PSBA_CAMERA_FREE_KD" in str(ei.value)
    hp.close()
    # the mask belongs to this model only; True still means the 11-block model
    for model, cnp in ((True, 11), (False, 6), (psba_amd.CAMERA_FREE_K, 11), (psba_amd.CAMERA_FIXED_K, 6)):
        ho = psba_amd.Psba(0)
        ho.set_camera_model(model)
        ho.upload_problem(p)
        assert ho.camera_block() == cnp
        with pytest.raises(psba_amd.PsbaError):
            ho.set_intrinsics_mask(BAL)
        with pytest.raises(psba_amd.PsbaError):
            ho.intrinsics_mask()
        ho.close()
