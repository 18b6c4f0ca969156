"""Intrinsics shared between cameras under the block-sparse solver (psba_set_sparse_intrinsics_groups) on
the GPU, against the host reference tests/sparse_shared_ref.py (which derives every bound; nothing here is fitted).
Needs an MI355X.

Inputs: those of test_gpu_shared_intrinsics.py opened with SOLVER_SPARSE -- tiny_problem (both cameras one group),
wide_problem(64 / 65) with shared_ref.wide_labels, wide_problem(65) as one group, P7 with labels one and two; masks all
free and BAL; both damping rules -- plus band scenes whose labels put the new kernels either side of their launch
boundaries: 4 / 5 members (k_fgrp_partial, four waves a workgroup), 25 / 26 groups (k_fbsr_fold_ea, 256
threads of ten per group), 64 / 65 cameras (k_fbsr_diag_inverse, eight cameras a workgroup), 512 / 513 cameras with
labels j % 3 (the block product's second trip; three interleaved groups of 171, more members than a workgroup has lanes)
and 2048 / 2049 cameras with labels j % 3 (the second trip of k_fpcg_fold, k_fpcg_start and k_fpcg_direction).
  T1  e_a is the dense grouped route's, bit for bit.      T2  the stored blocks are the ungrouped handle's minus mu D.
  T3  psba_sparse_S_times entry by entry.                   T4  psba_get_sparse_precond block by block.
  T5  the true residual of psba_schur_solve.                T6  the stop at the burst edges on constructed systems.
  T7  the expanded step, dp_b and the four try scalars.     T8  no grouping is bit-identical to never asking; runs repeat.
  T9  psba_levmar against the shared twin.                  T10 recovery of the shared ring scene with two poses held.
  T11 the settings compose on 54camsvarK.                   T12 the interface.
The module prints the worst found / allowed per input and quantity."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import freepcg_ref as fp
import shared_ref as sr
import sparse_shared_ref as ss
import test_gpu_shared_intrinsics as gs
from freekd_twin import BAL, CNP, start_kc
from test_freekd_twin import P54

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

PSBA_OK, PSBA_E_INVALID, PSBA_E_STATE = 0, -1, -6
TOL, MAXIT = 1e-10, 2000     # (wide, all ten free, small mu needs 470 iterations at 1e-10: test_sparse_shared_ref.py)
MQ_RULE, MQ_MUS = gs.MQ_RULE, gs.MQ_MUS
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nsparse groups, worst found / allowed per input and quantity:")
        for key in sorted({k[0] for k in WORST}):
            print(f"  {key}: " + ", ".join(f"{q} {v:.2e}" for (kk, q), v in WORST.items() if kk == key))


def note(case, what, ratio):
    WORST[(case, what)] = max(WORST.get((case, what), 0.0), float(ratio))
    print(f"{case} {what}: {float(ratio):.3e}")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def handle(p, kc, free, labels="never", sparse=True, rule=fr.NO_RULE, tol=TOL, max_iter=MAXIT):
    """a FREE_KD handle on (p, kc) under the mask; labels 'never': the groups' verb is not called"""
    import psba_amd
    h = psba_amd.Psba(0)
    if sparse:
        h.set_solver(psba_amd.SOLVER_SPARSE, tol=tol, max_iter=max_iter)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(p)
    h.set_distortion(kc)
    h.set_intrinsics_mask(free)
    if rule.marquardt:
        h.set_damping(rule.kind, rule.dmin, rule.dmax)
    if not isinstance(labels, str):
        (h.set_sparse_intrinsics_groups if sparse else h.set_intrinsics_groups)(labels)
    assert h.schur_path() == (6 if sparse else 5)
    return h


def dense_ea(h, nA):
    n32 = (nA + 31) // 32 * 32
    return h.get_reduce_buffer().reshape(n32 + 1, n32)[n32, :nA].copy()


def fused(v, mu, d):
    """round(v + mu d) with one rounding (what a contracted multiply-add stores)"""
    return float(Fraction(float(v)) + Fraction(float(mu)) * Fraction(float(d)))


# ---- T3, T4, T5 on whatever a handle holds ------------------------------------------------------------------------

def judge_product(case, h, fo, n_cams):
    for what, x in fp.product_vectors(n_cams, CNP):
        y = h.sparse_S_times(x)
        ratio, at = ar.excess(y, fo.times(x), fo.product_bound(x))
        note(case, "product / bound", ratio)
        assert ratio <= 1.0, f"{case}, x = {what}: y[{at}] (camera {at // CNP}, row {at % CNP}) is {ratio:.3e} of its bound"
        assert bits_equal(y[fo.away], fo.placeholder_product(x)), f"{case}, x = {what}: a folded-away entry of y"


def judge_precond(case, h, fo, cams=None):
    M = h.get_sparse_precond()
    B, E = ss.folded_blocks(fo)
    worst = 0.0
    for j in range(fo.n_cams) if cams is None else cams:
        kappa, allowed = ss.precond_bound(B[j], E[j])
        found = ss.precond_residual(M[j], B[j])
        worst = max(worst, found / allowed)
        assert found <= allowed, f"{case}: camera {j}: || M B - I || = {found:.3e} > {allowed:.3e} (kappa {kappa:.2e})"
    note(case, "|| M B - I || / allowed", worst)
    aw = fo.away.reshape(-1, CNP)
    j, a = np.nonzero(aw)
    off = M.copy()
    off[j, a, a] = 0.0
    assert np.all(off[j, a, :] == 0.0) and np.all(off[j, :, a] == 0.0), f"{case}: a folded-away row or column of M"


def judge_solve(case, h, fo, ea, tol=TOL):
    """-> (dp, iterations): relres <= tol and the true residual against the folded operator"""
    rc = h.schur_solve()
    iters, relres, _, _ = h.pcg_info()
    dp = h.get_dp()
    tr, gap = ss.relres_and_gap(fo, dp[:fo.n], ea, iters)
    note(case, "relres / tol", relres / tol)
    note(case, "true relres / allowed", tr / (tol + fp.C_GAP * gap))
    assert rc == PSBA_OK and relres <= tol, f"{case}: rc {rc}, relres {relres:.3e} after {iters} iterations"
    assert tr <= tol + fp.C_GAP * gap, f"{case}: true relres {tr:.6e}, tol {tol:.1e}, gap unit {gap:.3e}"
    return dp, iters


# ---- T1 .. T5, T7: one damping try ---------------------------------------------------------------------------------

def one_try(name, mask, which_mu, rule=fr.NO_RULE):
    rt, sm, mus, _ = gs.ref(name, mask)
    nA, nC = rt.nA, rt.nC
    mu = (MQ_MUS if rule.marquardt else mus)[which_mu]
    case = f"{name} {mask} {which_mu}" + (" marquardt" if rule.marquardt else "")
    hd = handle(rt.p, rt.kc, rt.free, rt.labels, sparse=False, rule=rule)
    hu = handle(rt.p, rt.kc, rt.free, "never", rule=rule)
    h = handle(rt.p, rt.kc, rt.free, rt.labels, rule=rule)
    try:
        rep, ngroups = h.intrinsics_groups()
        assert np.array_equal(rep, rt.rep) and ngroups == np.unique(rt.rep).size
        for x in (hd, hu, h):
            x.linearize(1.0, 1.0)
            x.schur_assemble(mu)
        D = h.get_damping_diag() if rule.marquardt else None
        Du = hu.get_damping_diag() if rule.marquardt else None
        jk, val, ea = h.get_sparse_S()
        # ---- T1
        assert bits_equal(ea, dense_ea(hd, nA)), f"{case}: e_a differs from the dense grouped route's"
        assert np.all(ea[rt.away] == 0.0)
        # ---- T2
        jku, valu, _ = hu.get_sparse_S()
        assert np.array_equal(jk, jku)
        dg = np.flatnonzero(jk[:, 0] == jk[:, 1])
        k = np.arange(CNP)
        offd = np.ones(val.shape, dtype=bool)
        offd[dg[:, None], k[None, :], k[None, :]] = False
        assert bits_equal(val[offd], valu[offd]), f"{case}: an off-diagonal entry differs from the ungrouped handle's"
        g, u = val[dg][:, k, k], valu[dg][:, k, k]                                    # [nC, 16] by camera: jk ascending
        assert np.array_equal(jk[dg, 0], np.arange(nC))
        if not rule.marquardt:
            assert bits_equal(g + mu, u), f"{case}: fl(grouped + mu) is not the ungrouped diagonal"
        else:
            same = (D[:nA] == Du[:nA]).reshape(nC, CNP)
            assert same[:, 10:].all() and same[np.bincount(rt.rep, minlength=nC)[rt.rep] == 1].all()
            two = g + mu * Du[:nA].reshape(nC, CNP)
            one = np.array([fused(a, mu, d) for a, d in zip(g.reshape(-1), Du[:nA])]).reshape(nC, CNP)
            ok = (two.view(np.int64) == u.view(np.int64)) | (one.view(np.int64) == u.view(np.int64))
            assert ok[same].all(), f"{case}: grouped + mu D is not the ungrouped diagonal where D involves no group"
        # ---- T3
        fo = ss.FoldedOp(nC, jk, val, rt.rep, rt.free, mu, D=D)
        judge_product(case, h, fo, nC)
        # ---- T5, T4
        dp, iters = judge_solve(case, h, fo, ea)
        judge_precond(case, h, fo)
        # ---- T7
        sc = h.backsub(mu)
        assert sc.status == 0
        dp = h.get_dp()
        newcams, newpts = h.get_params(1)
        dpa = dp[:nA].reshape(-1, CNP)
        assert bits_equal(dpa[:, :10], dpa[rt.rep][:, :10]) and bits_equal(newcams[:, :10], newcams[rt.rep][:, :10])
        assert np.all(dp[:nA][rt.held] == 0.0)
        r, bound = fr.dpb_residual(rt, sm, dp, mu, rule) if rule.marquardt else fr.dpb_residual(rt, sm, dp, mu)
        ratio, at = ar.excess(r, np.zeros(r.shape, ar.LD), bound)
        note(case, "dp_b", ratio)
        assert ratio <= 1.0, f"{case}: point {at // 3} entry {at % 3}: residual {float(r[at]):.3e} > {bound[at]:.3e}"
        got = dict(dp_l2=sc.dp_l2, gain_den=sc.gain_den, newp_l2=sc.newp_l2, new_cost=sc.new_cost)
        bad = []
        for what, (x, b) in sr.scalars(rt, sm, dp, newcams, newpts, mu, D=D).items():
            ratio = float(abs(ar.LD(got[what]) - x) / b)
            note(case, what, ratio)
            if not ratio <= 1.0:
                bad.append(f"{what} = {got[what]!r}, exact {float(x)!r}, bound {b:.3e}")
        assert not bad, f"{case}: " + "; ".join(bad)
    finally:
        for x in (hd, hu, h):
            x.close()


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name,mask", gs.CASES + [("P7-one", "bal"), ("P7-two", "bal")])
def test_one_damping_try_entrywise(name, mask, which_mu):
    one_try(name, mask, which_mu)


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name", ["wide-above", "one-group"])
def test_one_damping_try_entrywise_marquardt(name, which_mu):
    one_try(name, "bal", which_mu, MQ_RULE)


# ---- launch boundaries and the interleaved labels -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def band(n_cams, kind):
    """(problem, kc, labels) of band_scene(n_cams): 'mod3' = labels j % 3; ('first', m) = the first m cameras one group;
    ('pairs', g) = g groups of two neighbours, the rest alone"""
    lab = np.arange(n_cams) + 10
    if kind == "mod3":
        lab = np.arange(n_cams) % 3
    elif kind[0] == "first":
        lab[:kind[1]] = 0
    else:
        lab[:2 * kind[1]] = np.arange(2 * kind[1]) // 2
    lab = lab.astype(np.int32)
    p, kc = sr.share_problem(fp.band_scene(n_cams), start_kc(n_cams), lab)
    return p, kc, lab


def band_try(n_cams, kind, mask, dense):
    """T1 (where a dense handle is affordable), T3, T4, T5 and a second, bit-identical run on a band scene"""
    p, kc, lab = band(n_cams, kind)
    rep = sr.representatives(lab)
    nA = CNP * n_cams
    case = f"band{n_cams} {kind if isinstance(kind, str) else kind[0] + str(kind[1])} {mask}"
    h = handle(p, kc, gs.MASKS[mask], lab)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        h.schur_assemble(mu)
        jk, val, ea = h.get_sparse_S()
        if dense:
            hd = handle(p, kc, gs.MASKS[mask], lab, sparse=False)
            try:
                hd.linearize(1.0, 1.0)
                assert hd.max_diag() == h.max_diag()
                hd.schur_assemble(mu)
                assert bits_equal(ea, dense_ea(hd, nA)), f"{case}: e_a differs from the dense grouped route's"
            finally:
                hd.close()
        fo = ss.FoldedOp(n_cams, jk, val, rep, gs.MASKS[mask], mu)
        assert np.all(ea[fo.away] == 0.0)
        judge_product(case, h, fo, n_cams)
        dp, iters = judge_solve(case, h, fo, ea)
        multi = np.flatnonzero(np.bincount(rep, minlength=n_cams) > 1)
        judge_precond(case, h, fo, None if n_cams <= 128 else np.r_[multi, rep.size - 3:rep.size, [n_cams // 2]])
        sc = h.backsub(mu)
        dp = h.get_dp()
        assert sc.status == 0 and bits_equal(dp[:nA].reshape(-1, CNP)[:, :10], dp[:nA].reshape(-1, CNP)[rep][:, :10])
        # a second run of the same handle: the same bits (T8)
        h.schur_assemble(mu)
        assert all(bits_equal(a, b) for a, b in zip(h.get_sparse_S()[1:], (val, ea)))
        assert h.schur_solve() == PSBA_OK and h.pcg_info()[0] == iters
        sc2 = h.backsub(mu)
        assert bits_equal(h.get_dp(), dp) and (sc2.dp_l2, sc2.gain_den, sc2.new_cost) == (sc.dp_l2, sc.gain_den, sc.new_cost)
    finally:
        h.close()


@pytest.mark.parametrize("n_cams,kind,mask,dense", [
    (16, ("first", 4), "all", True), (16, ("first", 5), "all", True),       # k_fgrp_partial: one / two workgroups
    (64, ("pairs", 25), "bal", True), (65, ("pairs", 26), "bal", True),     # k_fbsr_fold_ea: 250 / 260 threads; k_fbsr_diag_inverse
    (512, "mod3", "bal", False), (513, "mod3", "bal", False),              # k_fpcg_spmv's second trip, groups of 171
    (2048, "mod3", "bal", False), (2049, "mod3", "bal", False)])           # k_fpcg_fold / start / direction's second trip
def test_launch_boundaries_and_interleaved_labels(n_cams, kind, mask, dense):
    assert (n_cams > 512) == ((n_cams + 3) // 4 > 128) and (n_cams > 2048) == ((CNP * n_cams + 255) // 256 > 128)
    band_try(n_cams, kind, mask, dense)


# ---- T6: constructed systems ------------------------------------------------------------------------------------------

MU_C = 1e-3


@functools.lru_cache(maxsize=None)
def constructed():
    """a grouped handle on the pattern problem of band43 (labels j % 3), every intrinsic free"""
    n_cams, blocks = fp.fpattern("band43")
    lab = (np.arange(n_cams) % 3).astype(np.int32)
    p, kc = sr.share_problem(fp.pattern_problem(n_cams, blocks), start_kc(n_cams), lab)
    h = handle(p, kc, fr.ALL, lab)
    h.linearize(1.0, 1.0)
    return h, lab


@pytest.fixture(scope="module", autouse=True)
def _close_constructed():
    yield
    if constructed.cache_info().currsize:
        constructed()[0].close()
        constructed.cache_clear()


def solve_constructed(h, case, tol, max_iter):
    h.set_solver(2, tol=tol, max_iter=max_iter)
    h.schur_assemble(MU_C)
    assert np.array_equal(h.get_sparse_S()[0], case["jk"])
    h.set_sparse_S(case["val"], case["b"])
    back = h.get_sparse_S()[2]                                              # e_a at folded-away coordinates is taken as 0
    assert np.all(back[case["fo"].away] == 0.0) and bits_equal(back[case["fo"].kept], case["b"][case["fo"].kept])
    rc = h.schur_solve()
    iters, relres, _, _ = h.pcg_info()
    x = h.get_dp()[:case["fo"].n].copy()
    h.backsub(MU_C)
    return rc, iters, relres, x


@pytest.mark.parametrize("k", fp.BURST_EDGES)
def test_stop_at_chosen_iteration(k):
    h, lab = constructed()
    case = ss.burst_case("band43", k, lab, MU_C)
    assert case is not None
    tol, fo = case["tol"], case["fo"]
    rc, iters, relres, x = solve_constructed(h, case, tol, fp.MAXIT)
    print(f"\nk = {k}: delta {case['delta']:.4g}, tol {tol:.3e}, twin {case['hist'][k - 1]:.3e} -> {case['hist'][k]:.3e}; "
          f"iters {iters}, relres {relres:.3e}")
    assert rc == PSBA_OK and iters == k and relres <= tol, f"stopped after {iters} iterations, the long-double twin after {k}"
    tr, gap = ss.relres_and_gap(fo, x, case["b"], iters)                    # T5 on a constructed system
    note("constructed band43", "true relres / allowed", tr / (tol + fp.C_GAP * gap))
    assert tr <= tol + fp.C_GAP * gap
    rc2, iters2, relres2, _ = solve_constructed(h, case, tol, k)
    assert rc2 == PSBA_OK and iters2 == k and relres2 <= tol
    rc3, iters3, relres3, _ = solve_constructed(h, case, tol, k - 1)
    assert rc3 == 4 and iters3 == k - 1 and relres3 > tol                    # PSBA_PCG_MAXIT
    assert abs(relres3 - case["hist"][k - 1]) <= 1e-3 * case["hist"][k - 1] + 1e-15


# ---- T8 ------------------------------------------------------------------------------------------------------------------

def lm_run(rt, labels):
    h = handle(rt.p, rt.kc, rt.free, labels)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        h.schur_assemble(mu)
        _, val, ea = h.get_sparse_S()
        assert h.schur_solve() == PSBA_OK
        assert h.backsub(mu).status == 0
        dp = h.get_dp()
        h.reset_params()
        res, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
        return val.tobytes(), ea.tobytes(), dp.tobytes(), log.tobytes(), h.get_params()[0]
    finally:
        h.close()


def test_no_grouping_is_bit_identical_and_grouped_runs_repeat():
    rt = gs.ref("wide-above", "bal")[0]
    never = lm_run(rt, "never")
    for labels in (None, np.arange(rt.nC)[::-1].copy()):
        got = lm_run(rt, labels)
        assert got[:4] == never[:4] and len(got[3]) > 0
    a, b = lm_run(rt, rt.labels), lm_run(rt, rt.labels)
    assert a[:4] == b[:4] and len(a[3]) > 0 and np.array_equal(a[4], b[4])
    assert a[0] != never[0] and np.array_equal(a[4][:, :10], a[4][rt.rep][:, :10])


# ---- T9, T10 -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(gs.P7_LABELS))
def test_levmar_against_the_shared_twin(which):
    rt = gs.ref("P7-" + which, "bal")[0]
    want, wlog = gs.twin_levmar(which)
    h = handle(rt.p, rt.kc, rt.free, rt.labels, tol=1e-10, max_iter=500)
    try:
        res, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
        assert res.pcg_unconverged == 0
        assert abs(res.init_err - want.init_err) <= 1e-12 * want.init_err
        n = min(len(log), len(wlog), 6)
        assert n >= 4
        np.testing.assert_allclose(log[:n, 1], wlog[:n, 1], rtol=1e-6)
        assert np.array_equal(log[:n, 4], wlog[:n, 4])
        assert abs(res.final_err - want.final_err) <= 1e-5 * want.final_err
        assert res.iters == want.iters and res.flag == gs.TWIN_FLAG[want.flag]
        cams, _ = h.get_params()
        assert bits_equal(cams[:, :10], cams[rt.rep][:, :10])
        held = [k for k in range(10) if not BAL[k]]
        assert np.array_equal(cams[:, held], np.hstack([np.asarray(rt.p["K"]).reshape(-1, 5), rt.kc])[:, held])
        assert np.abs(cams[:, 0] - np.asarray(rt.p["K"]).reshape(-1, 5)[:, 0]).max() > 0
    finally:
        h.close()


def test_recovery_of_the_shared_ring_scene_with_two_poses_held():
    lab = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    start, kc0, K_true, kc_true = sr.shared_ring(lab)
    rep = sr.representatives(lab)
    from freekd_twin import _ring_cameras
    cams0 = np.array(start["cams"], dtype=np.float64)             # the true poses of cameras 0 and 1 into the start, as
    cams0[:2, :3] = 0.0                                           # held_ref.held_ring does: they are held there
    cams0[:2, 3:] = _ring_cameras(6)[1][:2]
    start = dict(start, cams=cams0)
    poses = np.zeros(6, dtype=np.uint8)
    poses[:2] = 1
    for sparse in (False, True):                                  # the dense grouped handle: the input's sanity reference
        h = handle(start, kc0, BAL, lab, sparse=sparse, tol=1e-10, max_iter=500)
        try:
            h.set_held(poses, None)
            res, log = h.levmar(max_iter=30, tr_handoff=False, log_cap=256, stop_cost=-1.0)
            cams, _ = h.get_params()
        finally:
            h.close()
        f = np.abs(cams[:, 0] / K_true[:, 0] - 1).max()
        k1 = np.abs(cams[:, 5] - kc_true[:, 0]).max()
        k2 = np.abs(cams[:, 6] - kc_true[:, 1]).max()
        print(f"{'sparse' if sparse else 'dense'}: iterations {res.iters} flag {res.flag}: cost {res.final_err:.3e} of "
              f"{res.init_err:.3e}, f {f:.2e}, k1 {k1:.2e}, k2 {k2:.2e}")
        assert res.final_err <= 1e-15 * res.init_err and res.pcg_unconverged == 0
        assert f <= 1e-9 and k1 <= 1e-8 and k2 <= 1e-7
        assert bits_equal(cams[:, :10], cams[rep][:, :10])
        assert np.array_equal(cams[:2, 10:], np.asarray(start["cams"])[:2])


# ---- T11 -----------------------------------------------------------------------------------------------------------------

def test_settings_compose():
    """54camsvarK (450 points), four groups j % 4 with a per-camera mask row per group, held poses and a held point,
    priors on cameras and points, a Huber loss with sigmas, Marquardt's rule: T1, T3, T5."""
    import psba_amd
    nC = 54
    lab = (np.arange(nC) % 4).astype(np.int32)
    rep = sr.representatives(lab)
    p, kc = sr.share_problem(P54(), start_kc(nC), lab)
    nP, nA = p["nP"], CNP * nC
    rows = np.array([BAL, fr.ALL, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0], [1, 1, 1, 0, 0, 1, 1, 1, 0, 0]], dtype=np.uint8)[lab]
    rng = np.random.default_rng(3)
    poses, pts = np.zeros(nC, dtype=np.uint8), np.zeros(nP, dtype=np.uint8)
    poses[[0, 7]] = 1
    pts[5] = 1
    sigma = rng.uniform(0.5, 2.0, p["nO"])
    mu = 1e-3
    out = []
    for sparse in (True, False):
        h = handle(p, kc, fr.ALL, "never", sparse=sparse, rule=MQ_RULE)
        try:
            cams, pts0 = h.get_params(0)
            h.set_camera_masks(rows)
            (h.set_sparse_intrinsics_groups if sparse else h.set_intrinsics_groups)(lab)
            h.set_held(poses, pts)
            h.set_priors(cams * (1.0 + 1e-3), np.full((nC, CNP), 1e-2), pts0 + 1e-3, np.full((nP, 3), 1e-1))
            h.set_obs_weighting(psba_amd.LOSS_HUBER, 2.0, sigma)
            h.linearize(1.0, 1.0)
            h.schur_assemble(mu)
            if not sparse:
                out.append(dense_ea(h, nA))
                continue
            jk, val, ea = h.get_sparse_S()
            out.append(ea)
            fo = ss.FoldedOp(nC, jk, val, rep, rows, mu, D=h.get_damping_diag())
            judge_product("P54 composed", h, fo, nC)
            dp, _ = judge_solve("P54 composed", h, fo, ea)
            judge_precond("P54 composed", h, fo)
            assert h.backsub(mu).status == 0
            dpa = h.get_dp()[:nA].reshape(nC, CNP)
            assert np.all(dpa[[0, 7], 10:] == 0.0) and np.all(dpa[:, :10][rows == 0] == 0.0)
            sh = np.hstack([rows != 0, np.zeros((nC, 6), dtype=bool)])
            assert bits_equal(dpa[sh], dpa[rep][sh])
        finally:
            h.close()
    assert bits_equal(out[0], out[1]), "e_a differs from the dense grouped route's"


# ---- T12 -----------------------------------------------------------------------------------------------------------------

def test_interface():
    import psba_amd
    rt = gs.ref("P7-two", "bal")[0]
    p, lab, nC = rt.p, rt.labels, rt.nC

    def refused(call, code, *words):
        with pytest.raises(psba_amd.PsbaError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), str(ei.value)

    # only a SOLVER_SPARSE handle on blocks of 16 takes the verb; the text names the dense route's
    for model, sparse in ((psba_amd.CAMERA_FIXED_K, False), (psba_amd.CAMERA_FREE_K, False), (psba_amd.CAMERA_FREE_K, True),
                          (psba_amd.CAMERA_FREE_KD, False)):
        ho = psba_amd.Psba(0)
        if sparse:
            ho.set_solver(psba_amd.SOLVER_SPARSE)
        ho.set_camera_model(model)
        ho.upload_problem(p)
        refused(lambda: ho.set_sparse_intrinsics_groups(lab), PSBA_E_STATE, "psba_set_intrinsics_groups")
        if model == psba_amd.CAMERA_FREE_KD:
            assert ho.intrinsics_groups()[1] == nC
            refused(ho.get_sparse_precond, PSBA_E_STATE, "PSBA_SOLVER_SPARSE")
        ho.close()
    h = psba_amd.Psba(0)
    h.set_solver(psba_amd.SOLVER_SPARSE, tol=1e-10, max_iter=500)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    refused(lambda: h.set_sparse_intrinsics_groups(None), PSBA_E_STATE, "no problem uploaded")
    refused(h.get_sparse_precond, PSBA_E_STATE)
    h.upload_problem(p)
    h.set_distortion(rt.kc)
    h.set_intrinsics_mask(BAL)
    # the dense verb stays refused and changes nothing; the getter round-trips; NULL and all-alone are no grouping
    refused(lambda: h.set_intrinsics_groups(lab), PSBA_E_STATE, "PSBA_SOLVER_SPARSE")
    assert np.array_equal(h.intrinsics_groups()[0], np.arange(nC)) and h.intrinsics_groups()[1] == nC
    h.set_sparse_intrinsics_groups(lab * -1000 + 7)
    rep, n = h.intrinsics_groups()
    assert np.array_equal(rep, rt.rep) and n == 2
    h.set_sparse_intrinsics_groups(None)
    assert h.intrinsics_groups()[1] == nC
    h.set_sparse_intrinsics_groups(lab)
    h.set_sparse_intrinsics_groups(np.arange(nC) + 5)
    assert h.intrinsics_groups()[1] == nC
    h.set_sparse_intrinsics_groups(lab)
    # the preconditioner hook: only while the last solve stands; the covariance verbs refuse under groups
    h.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    refused(h.get_sparse_precond, PSBA_E_STATE, "psba_schur_solve")
    h.schur_assemble(mu)
    refused(h.get_sparse_precond, PSBA_E_STATE, "psba_schur_solve")
    refused(lambda: h.sparse_S_times_many(np.zeros((1, CNP * nC, 16))), PSBA_E_STATE, "psba_set_sparse_intrinsics_groups")
    refused(lambda: h.sparse_camera_covariance([0], mu=mu), PSBA_E_STATE, "psba_set_sparse_intrinsics_groups")
    refused(lambda: h.sparse_point_covariance([0], mu=mu), PSBA_E_STATE, "psba_set_sparse_intrinsics_groups")
    jk, val, ea = h.get_sparse_S()                                        # the refusals changed nothing
    assert h.schur_solve() == PSBA_OK
    M = h.get_sparse_precond()
    assert M.shape == (nC, CNP, CNP) and np.all(np.isfinite(M))
    assert h.backsub(mu).status == 0
    assert bits_equal(h.get_sparse_precond(), M)                          # the back-substitution leaves it standing
    dp = h.get_dp()
    h.schur_assemble(mu)
    refused(h.get_sparse_precond, PSBA_E_STATE, "psba_schur_solve")
    assert all(bits_equal(a, b) for a, b in zip(h.get_sparse_S()[1:], (val, ea)))
    poisoned = ea.copy()
    poisoned[rt.away] = 1e300                                             # entries at folded-away coordinates are taken as 0
    h.set_sparse_S(val, poisoned)
    assert bits_equal(h.get_sparse_S()[2], ea)
    assert h.schur_solve() == PSBA_OK and h.backsub(mu).status == 0 and bits_equal(h.get_dp(), dp)
    h.set_intrinsics_mask(BAL)                                            # a setter of the model ends the solve's standing
    refused(h.get_sparse_precond, PSBA_E_STATE, "psba_schur_solve")
    # members that differ: the message names the camera and the column; nothing changes
    h.set_sparse_intrinsics_groups(None)
    cams, pts = h.get_params()
    split = cams.copy()
    split[4, 6] += 1e-9
    h.set_params(split, pts)
    refused(lambda: h.set_sparse_intrinsics_groups(lab), PSBA_E_INVALID, "camera 4", "column 6")
    assert h.intrinsics_groups()[1] == nC
    h.set_params(cams, pts)
    h.set_sparse_intrinsics_groups(lab)
    # ... also a difference in the copy psba_reset_params restores
    hk = psba_amd.Psba(0)
    hk.set_solver(psba_amd.SOLVER_SPARSE)
    hk.set_camera_model(psba_amd.CAMERA_FREE_KD)
    Ks = np.asarray(p["K"], dtype=np.float64).reshape(-1, 5).copy()
    Ks[2, 0] *= 1.01
    hk.upload_problem(dict(p, K=Ks))
    refused(lambda: hk.set_sparse_intrinsics_groups(lab), PSBA_E_INVALID, "camera 2", "column 0")
    c7, p7 = hk.get_params()
    c7[:, :10] = c7[rt.rep][:, :10]
    hk.set_params(c7, p7)
    refused(lambda: hk.set_sparse_intrinsics_groups(lab), PSBA_E_INVALID, "psba_reset_params", "camera 2")
    assert hk.intrinsics_groups()[1] == nC
    hk.close()
    # set_params / set_distortion / set_camera_masks that would split a group: refused before the device is touched
    refused(lambda: h.set_params(split, pts), PSBA_E_INVALID, "psba_set_params", "camera 4", "column 6")
    assert np.array_equal(h.get_params()[0], cams)
    kc_split = rt.kc.copy()
    kc_split[5, 2] = 1e-3
    refused(lambda: h.set_distortion(kc_split), PSBA_E_INVALID, "psba_set_distortion", "camera 5", "column 7")
    rows = np.ones((nC, 10), dtype=np.uint8)
    rows[2, 5] = 0
    refused(lambda: h.set_camera_masks(rows), PSBA_E_INVALID, "camera 2", "k1")
    assert np.array_equal(h.get_params()[0], cams) and h.intrinsics_groups()[1] == 2 and np.all(h.camera_masks() == 1)
    rows[rt.rep == 0, 5] = 0
    h.set_camera_masks(rows)                                              # equal rows inside the groups pass
    h.set_sparse_intrinsics_groups(None)
    rows[4, 0] = 0
    h.set_camera_masks(rows)
    refused(lambda: h.set_sparse_intrinsics_groups(lab), PSBA_E_INVALID, "camera 4", "fu")
    h.set_camera_masks(None)
    h.set_sparse_intrinsics_groups(lab)
    h.set_distortion(rt.kc)
    h.set_params(cams, pts)
    # refused while a try is in flight, and then nothing changes
    h.linearize(1.0, 1.0)
    h.schur_assemble(mu)
    h.schur_solve()
    h.backsub_async(mu)
    refused(lambda: h.set_sparse_intrinsics_groups(None), PSBA_E_STATE, "in flight")
    h.backsub_wait()
    assert np.array_equal(h.intrinsics_groups()[0], rt.rep)
    # a new upload resets the groups
    h.upload_problem(p)
    assert h.intrinsics_groups()[1] == nC and np.array_equal(h.intrinsics_groups()[0], np.arange(nC))
    h.close()
