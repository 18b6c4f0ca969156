"""Gaussian priors on the free-intrinsics routes (psba_set_priors) on the host: the reference of
tests/prior_ref.py against itself (central differences of F, the augmented dense normal matrix, the reduced solve
against the embedded Schur system), its judges against a plain fp64 evaluation and against injected faults, the dense
LM with priors on the ring scene, and the existence of the entry points.  No GPU."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import held_ref as hr
import prior_ref as pr
import shared_ref as sr
from freekd_twin import BAL, tiny_problem
from test_freekd_twin import P7, scaled_tol
from test_gpu_dense_solve import ETA_MAX

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

ROUTES = {"kd-all": (16, fr.ALL), "kd-bal": (16, BAL), "fk": (11, None)}
RULES = {"identity": fr.NO_RULE, "marquardt": fr.Rule(fr.MARQUARDT)}


@functools.lru_cache(maxsize=None)
def prob(name):
    return {"tiny": tiny_problem, "P7": P7}[name]()


@functools.lru_cache(maxsize=None)
def route(name, which):
    """the holds of test_held_ref.py (tiny: pose 1 and point 1; P7: poses 0 and 1, the camera with the largest pose
    diagonal, one point with three views) with prior_ref.draw_priors on top"""
    cnp, free = ROUTES[which]
    p = prob(name)
    if name == "tiny":
        poses, pts = [1], [1]
    else:
        big, _ = hr.largest_pose_camera(p, cnp, free)
        poses, pts = sorted({0, 1, big}), [hr.point_with_views(p)]
    rt0 = hr.HeldRoute(p, cnp, free, hr.flags(p["nC"], poses), hr.flags(p["nP"], pts))
    rt = pr.PriorRoute(p, cnp, pr.draw_priors(rt0), free, rt0.held_poses, rt0.held_pts)
    return rt, pr.sums(rt)


def mu_of(rt, sm, rule):
    return 1e-3 if rule.marquardt else 1e-3 * float(np.concatenate([sm["diagU"], sm["diagV"]])[rt.free_all].max())


def test_the_drawn_priors_are_what_the_tests_need():
    rt, sm = route("P7", "kd-bal")
    pri = rt.pri
    has = np.any(pri.cam_info != 0.0, axis=(1, 2))
    assert has.any() and not has.all() and pri.counts()[1] == 3
    ranks = [np.linalg.matrix_rank(pri.cam_info[j]) for j in np.flatnonzero(has)]
    assert 2 in ranks and 16 in ranks
    diag_only = [j for j in np.flatnonzero(has) if np.array_equal(pri.cam_info[j], np.diag(np.diag(pri.cam_info[j])))]
    assert diag_only
    for info in (pri.cam_info, pri.pt_info):
        assert np.array_equal(info, info.transpose(0, 2, 1)) and np.all(np.linalg.eigvalsh(info) >= -1e-9 * np.abs(info).max())
    # a held pose and a held point carry a prior: the off-diagonal entries between held and free coordinates are there
    j = int(np.flatnonzero(rt.held_poses & has)[0])
    assert np.any(pri.cam_info[j][:10, 10:] != 0.0) and np.all(rt.info_eff()[0][j][:, 10:] == 0.0)
    assert np.any(pri.pt_info[rt.held_pts] != 0.0) and sm["cost"] > sm["cost_obs"]


@pytest.mark.parametrize("which", list(ROUTES))
def test_central_differences_of_F(which):
    """-2 g is the derivative of F on every free coordinate that a prior or an observation reaches, the mask and the
    holds included (a held coordinate's deviation stays in the gradient of the free ones); g of a held one is 0"""
    rt, sm = route("P7", which)
    cams, pts = rt.current()
    x0 = hr.flat(cams, pts)
    g = sm["g"].astype(np.float64)
    diag = np.concatenate([sm["diagU"], sm["diagV"]])
    F = sm["cost"]
    assert np.all(g[rt.held_all] == 0.0)
    rng = np.random.default_rng(0)
    free = np.flatnonzero(rt.free_all)
    with_prior = np.r_[np.flatnonzero(np.repeat(np.any(rt.pri.cam_info != 0.0, axis=(1, 2)), rt.cnp)),
                       rt.nA + np.flatnonzero(np.repeat(np.any(rt.pri.pt_info != 0.0, axis=(1, 2)), 3))]
    pick = np.union1d(rng.choice(free, 12, replace=False), rng.choice(np.intersect1d(free, with_prior), 24, replace=False))
    for k in pick:
        h = 1e-5 * np.sqrt(F / diag[k])
        vals = []
        for s in (1.0, -1.0):
            x = x0.copy()
            x[k] += s * h
            vals.append(pr.total_cost(rt, x[:rt.nA].reshape(rt.nC, rt.cnp), x[rt.nA:].reshape(rt.nP, 3)))
        cd = (vals[0] - vals[1]) / (2.0 * h)
        assert abs(cd + 2.0 * g[k]) <= 1e-6 * (np.sqrt(diag[k] * F) + abs(2.0 * g[k])), (k, cd, -2.0 * g[k])


@pytest.mark.parametrize("which", ["kd-bal", "fk"])
def test_the_augmented_normal_matrix(which):
    """J with the prior rows appended: J^T J = N + Lambda and J^T r = g + Lambda d; the reduced solve of that system
    (held columns deleted) agrees with the solve of the embedded Schur system the judges use"""
    rt, sm = route("P7", which)
    J, r = pr.augmented_jacobian(rt)
    N, g = pr.dense_system(rt)
    d = np.sqrt(np.where(np.diag(N) > 0.0, np.diag(N), 1.0))   # (a masked coordinate without a prior: an empty column)
    big = np.zeros(rt.nT)                                      # (R comes from an eigendecomposition: its error is relative to
    big[:rt.nA] = np.repeat(np.abs(rt.pri.cam_info).max(axis=(1, 2)), rt.cnp)   # the largest entry of the block)
    big[rt.nA:] = np.repeat(np.abs(rt.pri.pt_info).max(axis=(1, 2)), 3)
    assert np.all(np.abs(J.T @ J - N) <= 1e-12 * (np.outer(d, d) + np.sqrt(np.outer(big, big))))
    dC, _, dP, _ = pr.deviations(rt)
    d1 = np.r_[np.repeat(np.abs(dC.astype(np.float64)).sum(axis=1), rt.cnp), np.repeat(np.abs(dP.astype(np.float64)).sum(axis=1), 3)]
    assert np.all(np.abs(J.T @ r - g) <= 1e-12 * (np.abs(g).max() + big * d1))
    assert abs(float(r @ r) - sm["cost"]) <= 1e-12 * (sm["cost"] + float((big * d1 * d1).sum()))
    f = rt.free_all
    assert np.abs(g[f] - sm["g"].astype(np.float64)[f]).max() <= 1e-10 * np.abs(g).max()
    mu = mu_of(rt, sm, fr.NO_RULE)
    want = pr.reduced_solve(rt, mu, scaled=True)
    S, ea = pr.schur_ref(rt, sm, mu)
    ds = 1.0 / np.sqrt(np.diag(S))
    dpa = ds * np.linalg.solve(ds[:, None] * S * ds[None, :], ds * ea)
    assert np.all(want[rt.held_all] == 0.0)
    assert np.linalg.norm((dpa - want[:rt.nA]) / ds) <= 1e-8 * np.linalg.norm(want[:rt.nA] / ds)


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("name,which", [("tiny", "kd-all"), ("tiny", "fk"), ("P7", "kd-all"), ("P7", "kd-bal"), ("P7", "fk")])
def test_judges_pass_a_plain_evaluation(name, which, rule):
    rt, sm = route(name, which)
    rule = RULES[rule]
    mu = mu_of(rt, sm, rule)
    out = pr.judge(rt, sm, mu, rule, pr.plain_try(rt, mu, rule), scaled_tol(rt.p), ETA_MAX)
    assert {"S", "e_a", "g", "max_diag", "dp_b", "new_cost", "residual cost", "prior_cur cams", "prior_new pts"} <= set(out)
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("fault", pr.FAULTS)
def test_injected_faults_fail_the_judges(fault, rule):
    rt, sm = route("P7", "kd-bal")
    rule = RULES[rule]
    mu = mu_of(rt, sm, rule)
    got = pr.plain_try(rt, mu, rule, fault)
    try:
        out = pr.judge(rt, sm, mu, rule, got, scaled_tol(rt.p), ETA_MAX)
    except AssertionError as e:                              # an exact part
        assert fault == "held-row" and "held" in str(e)
        return
    bad = {k for k, v in out.items() if not v <= 1.0}
    want = {"g-dropped": {"g", "e_a"}, "sign": {"g", "e_a"}, "no-new-cost": {"new_cost"}}[fault]
    assert want <= bad, (fault, out)
    if fault == "no-new-cost":
        assert bad == {"new_cost"}


@functools.lru_cache(maxsize=None)
def shared_route():
    """shared_ref.shared_ring, two groups of three cameras, {f, k1, k2}, poses 0 and 1 held, drawn priors: the members
    of a group carry different priors on the shared intrinsics"""
    labels = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    start, kc0, _, _ = sr.shared_ring(labels)
    poses = hr.flags(6, [0, 1])
    rt0 = hr.HeldSharedRoute(start, labels, BAL, kc0, poses)
    rt = pr.PriorSharedRoute(start, labels, pr.draw_priors(rt0), BAL, kc0, poses)
    return rt, pr.sums(rt)


def test_a_shared_intrinsic_gets_the_sum_of_its_members_priors():
    rt, sm = shared_route()
    has = np.any(rt.pri.cam_info != 0.0, axis=(1, 2))
    assert has[0] and has[1] and rt.rep[1] == 0 and rt.pri.cam_info[1][0, 0] != rt.pri.cam_info[0][0, 0]
    mu = 1e-3 * float(rt.folded_diag(sm)[0][rt.folded_diag(sm)[1]].max())
    S_want, ea_want = pr.schur_ref(rt, sm, mu)
    d = pr.scale_diag(rt, sm, mu)
    eS, ee = sr.scaled_errors(*pr.plain_shared_system(rt, mu), S_want, ea_want, d, sm["cost"])
    assert eS <= rt.tol and ee <= rt.tol
    eS, ee = sr.scaled_errors(*pr.plain_shared_system(rt, mu, "shared-once"), S_want, ea_want, d, sm["cost"])
    assert eS > rt.tol and ee > rt.tol
    # the folded diagonal of a shared coordinate is the sum over the members, priors included
    fd = rt.folded_diag(sm)[0]
    assert abs(fd[0] - sm["diagU"].reshape(6, 16)[:3, 0].sum()) <= 1e-12 * fd[0]


LM_ITERS = 15


@functools.lru_cache(maxsize=None)
def ring_lm(w_scale=1.0):
    start, kc0, pri = pr.ring_priors()
    pri.cam_info[:, 0, 0] *= w_scale
    t = pr.PriorTwin(start, pri, kc0, BAL)
    res, log = t.levmar(max_iter=LM_ITERS)
    return res, log, t.cams.copy(), pri


def test_prior_twin_on_the_ring_scene():
    """the weights of tests/test_gpu_priors.py's LM case: below 1e-6 of the starting cost within 15 iterations without
    ending on a stop test; a million-fold weight on fu ends closer to its mean"""
    res, log, cams, pri = ring_lm()
    assert res.flag == 0 and res.iters == LM_ITERS and res.final_err <= 1e-6 * res.init_err
    _, _, cams2, pri2 = ring_lm(1e6)
    assert np.all(np.abs(cams2[:, 0] - pri2.cam_mean[:, 0]) < np.abs(cams[:, 0] - pri.cam_mean[:, 0]))


def test_entry_points_exist():
    """the library exports the verbs (a null handle is refused before anything is touched) and capi.py binds them"""
    from psba_amd import capi
    assert capi.lib.psba_set_priors(None, None, None, None, None) == -1
    assert capi.lib.psba_prior_counts(None, None, None) == -1
    assert capi.lib.psba_prior_cost(None, 0, None, None) == -1
    assert all(hasattr(capi.Psba, k) for k in ("set_priors", "prior_counts", "prior_cost"))
