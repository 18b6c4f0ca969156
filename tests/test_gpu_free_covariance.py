"""Covariance of the refined cameras and points with free intrinsics on the GPU (psba_free_covariance_compute and its
getters; blocks of 11 and 16).  The reference and its judges are tests/freecov_ref.py; no constant is fitted
to a GPU result.  Needs an MI355X.

  1  the state and error rules
  2  the inverse on the device's own S (psba_get_reduce_buffer) by freecov_ref.inverse_judge, and the exact parts with ==
  3  the points per entry on the device's own inputs (V and Y from psba_get_free_point_blocks, C_aa from the device)
  4  end to end against freecov_ref.reduced_dense
  5  psba_get_free_sigmas
  6  bit-identity and non-interference
The module prints the worst found / allowed per case; DESIGN 7l keeps the table."""
import numpy as np
import pytest

import psba_amd
from psba_amd import capi
import assembly_ref as ar
import free_ref as fr
import freecov_ref as fc
import held_ref as hr
import prior_ref as pr
import weight_ref as wr
from freekd_twin import BAL, _scene, start_kc, wide_problem
from test_freecov_ref import MQ, ROUTES, p7, plain_route, ring
from test_freekd_twin import P7
from test_gpu_priors import plain_handle, read_system, shared_handle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

LD = ar.LD
RULES = {"identity": fr.NO_RULE, "marquardt": MQ}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nfree covariance: worst found / allowed per case:\n" + "\n".join(f"  {k}: {v:.3e}" for k, v in WORST.items()))


def note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))
    print(f"{what}: {float(ratio):.3e}")


def handle(rt, rule=fr.NO_RULE):
    """the device's handle of a route: mask, damping, groups, holds, priors, weighting"""
    if hasattr(rt, "labels"):
        h = shared_handle(rt, rule, ("mask", "groups", "damping", "holds", "priors"))
    else:
        h = plain_handle(rt.p, rt.cnp, rt.free, rule)
        if rt.held_poses.any() or rt.held_pts.any():
            h.set_held(rt.held_poses, rt.held_pts)
        if sum(rt.pri.counts()):
            h.set_priors(**rt.pri.args())
    if rt.weighted:
        h.set_obs_weighting(rt.kind, rt.c, rt.sigma if rt.has_sigma else None)
    return h


def mu_of(h, rule, rel=1e-6):
    """1e-6 of the largest diagonal entry; Marquardt's mu is relative already"""
    if rule.marquardt:
        return rel
    h.linearize(1.0, 1.0)
    return rel * h.max_diag()


def refused(fn, code, *words):
    with pytest.raises(capi.PsbaError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def getters_refuse(h):
    for fn in (h.free_camera_covariance, h.free_covariance_matrix, h.free_point_covariance, h.free_sigmas, h.free_covariance_times):
        refused(fn, -6)


def check_exact_parts(rt, C):
    """zeros, bit-symmetry, member rows equal to the representative's"""
    src = fc.coord_map(rt)
    dead = src < 0
    assert np.array_equal(C, C.T)
    assert np.all(C[dead] == 0.0) and np.all(C[:, dead] == 0.0)
    away = np.flatnonzero((src >= 0) & (src != np.arange(rt.nA)))
    assert np.array_equal(C[away], C[src[away]]) and np.array_equal(C[:, away], C[:, src[away]])
    live = np.flatnonzero(src == np.arange(rt.nA))
    assert np.all(np.diag(C)[live] > 0.0)
    return live, away


# ---- 1. state and error rules ------------------------------------------------------------------------------------------
def test_state_and_error_rules():
    rt = p7("kd-bal")
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    refused(lambda: h.free_covariance(), -6, "no problem uploaded")
    for name in ("psba_get_free_covariance_matrix", "psba_get_free_point_covariance", "psba_get_free_sigmas"):
        assert getattr(capi.lib, name)(h._h, None) == -6
    h.close()
    h = handle(rt)
    getters_refuse(h)  # nothing computed yet
    for mu, scale in ((-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.0, 0.0), (0.0, -2.0),
                      (0.0, float("nan")), (0.0, float("inf"))):
        refused(lambda: h.free_covariance(mu, scale), -1)
    getters_refuse(h)
    refused(lambda: h.free_covariance(reassemble=False), -6, "psba_schur_assemble")  # nothing in the reduce buffer
    refused(h.free_point_blocks, -6, "assembled")
    refused(lambda: h.covariance(1.0), -6, "PSBA_CAMERA_FREE_KD")  # the fixed-K verb still refuses the model
    assert h.free_covariance() == capi.PSBA_OK
    refused(h.covariance_matrix, -6)  # ... and its getters a free handle
    C, D, P, sg = h.free_covariance_matrix(), h.free_camera_covariance(), h.free_point_covariance(), h.free_sigmas()
    assert C.shape == (rt.nA, rt.nA) and D.shape == (7, 16, 16) and P.shape == (rt.nP, 3, 3) and sg.shape == (rt.nT,)
    assert h.free_covariance_times().shape == (3,) and capi.lib.psba_free_covariance_times(h._h, None) == -1
    V, Y = h.free_point_blocks()
    assert V.shape == (rt.nP, 3, 3) and Y.shape == (rt.nO, 16, 3)
    # a refused call changes nothing
    refused(lambda: h.free_covariance(-1.0), -1)
    refused(lambda: h.free_camera_covariance([(0, 7)]), -1, "out of range")
    refused(lambda: h.free_camera_covariance([(-1, 2)]), -1, "out of range")
    out = np.empty(256 * 3)
    assert capi.lib.psba_get_free_camera_covariance(h._h, 3, None, capi._d(out)) == -1  # no list: n_pairs must be nCams
    assert capi.lib.psba_get_free_camera_covariance(h._h, 7, None, None) == -1
    assert np.array_equal(h.free_covariance_matrix(), C) and np.array_equal(h.free_point_covariance(), P)
    # pairs in both orders are the blocks of the matrix and their transposes, bit for bit
    pairs = np.random.default_rng(3).integers(0, 7, size=(20, 2))
    pairs[0] = (6, 0)
    B, Bt = h.free_camera_covariance(pairs), h.free_camera_covariance(pairs[:, ::-1])
    for (j, k), b, bt in zip(pairs, B, Bt):
        assert np.array_equal(b, C[16 * j:16 * j + 16, 16 * k:16 * k + 16]) and np.array_equal(bt, b.T)
    assert all(np.array_equal(D[j], C[16 * j:16 * j + 16, 16 * j:16 * j + 16]) for j in range(7))
    # the handle is as after psba_schur_reduce: a solve may follow, and a try does not touch the result
    h.schur_solve()
    assert h.backsub(0.0).status == 0
    assert np.array_equal(h.free_covariance_matrix(), C)
    h.accept()  # ... but accepting its step moves the parameters
    getters_refuse(h)
    # the point part does not exist after reassemble = 0
    h.linearize(1.0, 1.0)
    h.schur_assemble(0.0)
    assert h.free_covariance(reassemble=False) == capi.PSBA_OK
    h.free_covariance_matrix()
    refused(h.free_point_covariance, -6, "reassemble = 0")
    refused(h.free_sigmas, -6, "reassemble = 0")
    # every setter of the route, and whatever moves the parameters, invalidates the result
    cams, pts = h.get_params()
    pri = pr.Priors(7, 16, rt.nP)
    pri.cam_info[2], pri.pt_info[5] = np.eye(16), np.eye(3)
    movers = [lambda: h.set_params(cams, pts), h.reset_params, lambda: h.set_distortion(start_kc(7)),
              lambda: h.set_intrinsics_mask(BAL), lambda: h.set_intrinsics_groups(None),
              lambda: h.set_damping(fr.MARQUARDT), lambda: h.set_damping(fr.IDENTITY),
              lambda: h.set_held(rt.held_poses, None), lambda: h.set_held(rt.held_poses, rt.held_pts),
              lambda: h.set_priors(**pri.args()), lambda: h.set_priors(),
              lambda: h.set_obs_weighting(wr.CAUCHY, 2.0), lambda: h.set_obs_weighting(wr.NONE, 1.0)]
    for move in movers:
        assert h.free_covariance() == capi.PSBA_OK
        h.free_covariance_matrix()
        move()
        getters_refuse(h)
    # a try in flight
    h.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h.schur_reduce()
    h.schur_solve()
    h.backsub_async(mu)
    refused(lambda: h.free_covariance(), -6, "in flight")
    h.backsub_wait()
    assert h.free_covariance() == capi.PSBA_OK
    h.close()
    # blocks of 11 refuse the fixed-K verb too; the six-block handle refuses the new one and names the other
    fk = handle(p7("fk"))
    refused(lambda: fk.covariance(1.0), -6, "PSBA_CAMERA_FREE_K")
    fk.close()
    six = psba_amd.Psba(0)
    six.upload_problem(P7())
    refused(lambda: six.free_covariance(1.0), -6, "psba_covariance_compute")
    getters_refuse(six)
    six.close()


# ---- 2. the inverse, on the device's own S -------------------------------------------------------------------------------
def judge_inverse(rt, rule, mu, what, kappa_max=None):
    h = handle(rt, rule)
    try:
        mu = mu_of(h, rule) if mu is None else mu
        assert h.free_covariance(mu) == capi.PSBA_OK
        S, _, _ = read_system(h, rt.nA)  # the S that was inverted
        C = h.free_covariance_matrix()
    finally:
        h.close()
    live, _ = check_exact_parts(rt, C)
    # the diagonal blocks of the route's S are symmetric only to rounding (kernels_free.hip): their lower triangle is
    # the matrix, and the lower triangle is what the factorization reads
    S = np.tril(S) + np.tril(S, -1).T
    dev, yard, allowed, kappa = fc.inverse_judge(S[np.ix_(live, live)], C[np.ix_(live, live)])
    print(f"{what}: n = {live.size}, kappa of the scaled S {kappa:.2e}, yardstick {yard:.2e}, device {dev:.2e}, "
          f"device / yardstick {dev / yard:.2f}")
    if kappa_max is not None:
        assert kappa <= kappa_max, kappa
    note(f"inverse {what}", dev / allowed)
    assert dev <= allowed, (what, dev, allowed)


def test_inverse_the_true_covariance_of_7camsvarK():
    """kd-bal, mu = 0 with poses 0 and 1 held: the scaled S is well conditioned (test_held_ref.py asserts the same)"""
    judge_inverse(p7("kd-bal", False), fr.NO_RULE, 0.0, "7camsvarK kd-bal mu = 0", kappa_max=1e6)


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("which", list(ROUTES))
def test_inverse_7camsvarK_at_a_small_mu(which, rule):
    """kd-all and fk are singular at mu = 0 with holds alone, so every route gets mu = 1e-6 max diag"""
    judge_inverse(p7(which), RULES[rule], None, f"7camsvarK {which} {rule}")


@pytest.mark.parametrize("which, nC", [("kd-all", 20), ("fk", 30)])
def test_inverse_wide_problems(which, nC):
    """cameras with 1 and 0 observations and a point with none; n = 320 and 330"""
    judge_inverse(plain_route(wide_problem(nC), which), fr.NO_RULE, None, f"wide_problem({nC}) {which}")


def test_inverse_shared_ring():
    """two groups of three, mu = 0, poses 0 and 1 held (priors and a weighting as well)"""
    rt = ring()
    judge_inverse(rt, fr.NO_RULE, 0.0, "shared ring mu = 0")


# ---- 3. points, on the device's own inputs -------------------------------------------------------------------------------
def judge_points(rt, rule, what, scale=2.5, points=None):
    h = handle(rt, rule)
    try:
        mu = mu_of(h, rule)
        assert h.free_covariance(mu, scale) == capi.PSBA_OK
        Caa, P = h.free_covariance_matrix(), h.free_point_covariance()
        V, Y = h.free_point_blocks()
    finally:
        h.close()
    assert np.all(P[rt.held_pts] == 0.0)  # held points are exactly 0
    assert np.array_equal(P, np.transpose(P, (0, 2, 1)))  # symmetry is bit-exact
    cnt = np.bincount(rt.i, minlength=rt.nP)
    free_pts = np.flatnonzero(~rt.held_pts)
    if points is not None:
        free_pts = np.intersect1d(free_pts, points)
    J = fc.point_judges(rt.i, rt.j, V, Y, Caa, mu, rule, scale, free_pts, rt.cnp)
    worst = 0.0
    for q, (want, bound, want_ld) in J.items():
        err = np.abs(P[q].astype(LD) - want_ld).astype(np.float64)
        worst = max(worst, ar.excess(P[q], want_ld, bound)[0])  # (an entry that is exactly 0 has a zero bound)
        assert np.all(err <= bound), (what, q, int(cnt[q]), err, bound)
    print(f"{what}: {len(J)} points (tracks {cnt[free_pts].min()} .. {cnt[free_pts].max()})")
    note(f"points {what}", worst)
    return P, V, cnt, mu, scale


def weighted_p7(which):
    """7camsvarK with poses 0 and 1 and a point held, drawn priors and Cauchy + sigmas"""
    cnp, free = ROUTES[which]
    p = P7()
    poses, pts = hr.flags(7, [0, 1]), hr.flags(int(p["nP"]), [hr.point_with_views(p)])
    rt0 = hr.HeldRoute(p, cnp, free, poses, pts)
    sigma, c = wr.draw_weighting(rt0, wr.CAUCHY)
    return wr.WeightRoute(p, cnp, pr.draw_priors(rt0), (wr.CAUCHY, c), sigma, free, poses, pts)


@pytest.mark.parametrize("which", list(ROUTES))
def test_points_7camsvarK_with_holds_priors_and_weighting(which):
    rt = weighted_p7(which)
    assert rt.held_pts.sum() == 1 and sum(rt.pri.counts()) > 0 and rt.weighted
    judge_points(rt, MQ, f"7camsvarK {which} held, priors, Cauchy + sigmas")


@pytest.mark.parametrize("which, nC", [("kd-all", 65), ("fk", 94)])
def test_points_wide_problems(which, nC):
    """points seen once, a point without observations (scale V*^-1 exactly as the kernel forms it), cameras without"""
    rt = plain_route(wide_problem(nC), which, pts=[3])
    P, V, cnt, mu, scale = judge_points(rt, fr.NO_RULE, f"wide_problem({nC}) {which}")
    assert np.any(cnt == 1) and cnt[-1] == 0 and np.all(np.einsum("ikk->ik", P[[0, rt.nP - 1]]) > 0.0)


def test_points_with_tracks_longer_than_a_staging_chunk():
    """the rows Z_j of 32 cameras are staged at a time: tracks of 33 .. 55 cameras take two chunks (the second one
    partial), 64 exactly two, 70 three, with the sum carried from chunk to chunk"""
    rng = np.random.default_rng(41)
    nC, nP = 70, 40
    lens = np.r_[[33, 40, 47, 55, 64, 70], rng.integers(33, 56, nP - 6)]
    keep = np.zeros((nP, nC), dtype=bool)
    for i, n in enumerate(lens):
        keep[i, rng.choice(nC, size=n, replace=False)] = True
    p = _scene(rng, nC, rng.uniform(-1.0, 1.0, (nP, 3)), keep)
    for which in ("kd-all", "fk"):
        rt = plain_route(p, which, [0, 1], [7])
        _, _, cnt, _, _ = judge_points(rt, fr.NO_RULE, f"70 cameras, long tracks {which}", points=np.arange(12))
        assert np.array_equal(cnt, lens)


# ---- 4. end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["7camsvarK kd-bal", "shared ring"])
def test_end_to_end_against_the_reduced_dense_inverse(name):
    """mu = 0; the scaled error may be at most kappa 1e-11 with kappa of the scaled reduced system <= 1e7 (7h's rule)"""
    rt = p7("kd-bal") if name.startswith("7") else ring()
    h = handle(rt)
    try:
        assert h.free_covariance(0.0, 1.0) == capi.PSBA_OK
        Caa, P = h.free_covariance_matrix(), h.free_point_covariance()
    finally:
        h.close()
    C, kappa = fc.reduced_dense(rt, 0.0)
    assert kappa <= 1e7, kappa
    want_a, want_b = fc.split(C, rt)
    ea, eb = fc.scaled_error(Caa, want_a), fc.scaled_error(P, want_b)
    print(f"{name}: kappa {kappa:.2e}, cameras {ea:.2e}, points {eb:.2e} (allowed {kappa * 1e-11:.2e})")
    note(f"end to end {name} cameras", ea / (kappa * 1e-11))
    note(f"end to end {name} points", eb / (kappa * 1e-11))
    assert ea <= kappa * 1e-11 and eb <= kappa * 1e-11
    check_exact_parts(rt, Caa)


# ---- 5. the standard deviations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kd-bal", "fk"])
def test_sigmas_are_the_square_roots_of_the_diagonals(which):
    rt = p7(which)
    h = handle(rt)
    try:
        assert h.free_covariance(mu_of(h, fr.NO_RULE), 1.5) == capi.PSBA_OK
        C, P, sg = h.free_covariance_matrix(), h.free_point_covariance(), h.free_sigmas()
    finally:
        h.close()
    want = np.sqrt(np.r_[np.diag(C), np.einsum("ikk->ik", P).reshape(-1)])
    assert np.array_equal(sg, want)
    assert np.all(sg[rt.held_all] == 0.0) and np.all(sg[rt.free_all] > 0.0)


# ---- 6. bit-identity and non-interference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["7camsvarK kd-all", "7camsvarK fk", "shared ring"])
def test_two_computes_and_a_fresh_handle_are_bit_identical(name):
    """the route has no atomics: no condition is needed"""
    rt = ring() if name == "shared ring" else weighted_p7(name.split()[1])
    got = []
    for computes in (2, 1):
        h = handle(rt, MQ)
        for _ in range(computes):
            assert h.free_covariance(1e-6, 1.0) == capi.PSBA_OK
            got.append((read_system(h, rt.nA)[0], h.free_covariance_matrix(), h.free_point_covariance()))
        h.close()
    assert len(got) == 3
    for S, C, P in got[1:]:
        assert np.array_equal(S, got[0][0]) and np.array_equal(C, got[0][1]) and np.array_equal(P, got[0][2])


@pytest.mark.parametrize("which", ["kd-bal", "fk"])
def test_levmar_after_a_compute_is_the_run_of_a_handle_that_never_computed(which):
    rt = weighted_p7(which)
    runs = []
    for compute in (True, False):
        h = handle(rt)
        if compute:
            assert h.free_covariance(mu_of(h, fr.NO_RULE)) == capi.PSBA_OK
            assert h.free_covariance(0.0 if which == "kd-bal" else 1.0, 2.0) == capi.PSBA_OK
        res, log = h.levmar(max_iter=5, log_cap=64)
        if compute:
            getters_refuse(h)  # the loop accepted steps
        runs.append((log, *h.get_params()))
        h.close()
    assert runs[0][0].shape[0] >= 2
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
