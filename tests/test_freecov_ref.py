"""Covariance with free intrinsics (psba_free_covariance_compute) on the host: the two statements of the
model in tests/freecov_ref.py against each other, its judges against a plain fp64 evaluation and against injected
faults, and the existence of the entry points.  No GPU."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import freecov_ref as fc
import held_ref as hr
import prior_ref as pr
import shared_ref as sr
import weight_ref as wr
from freekd_twin import BAL, tiny_problem
from test_freekd_twin import P7

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

ROUTES = {"kd-all": (16, fr.ALL), "kd-bal": (16, BAL), "fk": (11, None)}
MQ = fr.Rule(fr.MARQUARDT)
AGREE = 1e-11  # times kappa of the scaled reduced system: 7h's rule for two fp64 statements of one inverse


def plain_route(p, which, poses=None, pts=None):
    """a route without priors and without a weighting"""
    cnp, free = ROUTES[which]
    nC, nP = int(p["nC"]), int(p["nP"])
    return wr.WeightRoute(p, cnp, pr.Priors(nC, cnp, nP), free=free, poses=None if poses is None else hr.flags(nC, poses),
                          pts=None if pts is None else hr.flags(nP, pts))


@functools.lru_cache(maxsize=None)
def p7(which, held_pt=True):
    p = P7()
    return plain_route(p, which, [0, 1], [hr.point_with_views(p)] if held_pt else None)


@functools.lru_cache(maxsize=None)
def ring(weighted=True):
    """shared_ref.shared_ring, two groups of three, {f, k1, k2}, poses 0 and 1 held, drawn priors, Cauchy + sigmas"""
    labels = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    start, kc0, _, _ = sr.shared_ring(labels)
    poses = hr.flags(6, [0, 1])
    rt0 = hr.HeldSharedRoute(start, labels, BAL, kc0, poses)
    sigma, c = wr.draw_weighting(rt0, wr.CAUCHY)
    loss = (wr.CAUCHY, c) if weighted else (wr.NONE, 1.0)
    return wr.WeightSharedRoute(start, labels, pr.draw_priors(rt0), loss, sigma if weighted else None, BAL, kc0, poses)


def mu_small(rt):
    N, _ = pr.dense_system(rt)
    return 1e-6 * float(np.diag(N)[rt.free_all].max())


def agree(rt, mu, rule=fr.NO_RULE, scale=1.0, fault=None):
    """(scaled error of the camera part, of the point blocks, the allowed kappa AGREE) of the Schur statement against
    the reduced dense inverse"""
    C, kappa = fc.reduced_dense(rt, mu, rule, scale)
    want_a, want_b = fc.split(C, rt)
    Caa, Cbb = fc.schur_statement(rt, mu, rule, scale, fault)
    return fc.scaled_error(Caa, want_a), fc.scaled_error(Cbb, want_b), kappa * AGREE


def test_the_two_statements_agree_on_tiny_problem():
    """mu > 0 only: the problem is singular at 0"""
    for which in ROUTES:
        rt = plain_route(tiny_problem(), which, [1], [1])
        for rule, mu in ((fr.NO_RULE, 1e-3 * mu_small(rt) / 1e-6), (MQ, 1e-3)):
            ea, eb, tol = agree(rt, mu, rule, 2.5)
            assert ea <= tol and eb <= tol, (which, str(rule), ea, eb, tol)


@pytest.mark.parametrize("which", list(ROUTES))
def test_the_two_statements_agree_on_7camsvarK(which):
    rt = p7(which)
    cases = [(fr.NO_RULE, mu_small(rt)), (MQ, 1e-6)] + ([(fr.NO_RULE, 0.0)] if which == "kd-bal" else [])
    for rule, mu in cases:
        C, kappa = fc.reduced_dense(rt, mu, rule)
        assert kappa <= 1e7, (which, mu, kappa)
        ea, eb, tol = agree(rt, mu, rule)
        print(f"{which} {rule} mu = {mu:.3g}: kappa {kappa:.2e}, cameras {ea:.2e}, points {eb:.2e} (allowed {tol:.2e})")
        assert ea <= tol and eb <= tol
        # the exact parts of the definition
        Caa, Cbb = fc.split(C, rt)
        assert np.all(Caa[rt.held] == 0.0) and np.all(Caa[:, rt.held] == 0.0) and np.all(Cbb[rt.held_pts] == 0.0)
        live = np.flatnonzero(fc.coord_map(rt) >= 0)
        assert np.all(np.diag(Caa)[live] > 0.0)


def test_the_two_statements_agree_on_the_shared_ring_with_priors_and_cauchy():
    rt = ring()
    src = fc.coord_map(rt)
    away = np.flatnonzero((src >= 0) & (src != np.arange(rt.nA)))
    assert away.size == 4 * 3 and np.all(src[rt.held] == -1)
    for rule, mu in ((fr.NO_RULE, 0.0), (MQ, 1e-6)):
        C, kappa = fc.reduced_dense(rt, mu, rule)
        assert kappa <= 1e7, kappa
        ea, eb, tol = agree(rt, mu, rule)
        assert ea <= tol and eb <= tol, (str(rule), ea, eb, tol)
        Caa = C[:rt.nA, :rt.nA]
        # shared intrinsics are perfectly correlated: a member's row and column are its representative's
        assert np.array_equal(Caa[away], Caa[src[away]]) and np.array_equal(Caa[:, away], Caa[:, src[away]])


def _live_S(rt, mu):
    """the live part of the folded S of the Schur statement (fp64) and the Schur statement's own inputs"""
    N, _ = pr.dense_system(rt)
    nA = rt.nA
    src = fc.coord_map(rt)
    live = np.flatnonzero(src == np.arange(nA))
    E = fc.expansion(src, live)
    fb = rt.free_all[nA:]
    Nab = N[:nA, nA:][:, fb]
    Nbb = N[nA:, nA:][np.ix_(fb, fb)] + mu * np.eye(int(fb.sum()))
    S = E.T @ (N[:nA, :nA] - Nab @ np.linalg.solve(Nbb, Nab.T)) @ E + mu * np.eye(live.size)
    return 0.5 * (S + S.T)


def test_a_plain_fp64_inverse_passes_the_inverse_judge_and_a_perturbed_one_does_not():
    """a plain fp64 Cholesky inverse of the unscaled S in the device's place"""
    for rt, mu in ((p7("kd-bal", False), 0.0), (ring(False), 0.0)):
        S = _live_S(rt, mu)
        L = np.linalg.cholesky(S)
        Li = np.zeros_like(L)
        for r in range(S.shape[0]):  # forward substitution, row by row (a pivoted solve would not be scale-invariant)
            Li[r] = ((np.arange(S.shape[0]) == r) - L[r, :r] @ Li[:r]) / L[r, r]
        X = Li.T @ Li
        dev, yard, allowed, kappa = fc.inverse_judge(S, X)
        print(f"n = {S.shape[0]}: kappa of D S D {kappa:.2e}, plain Cholesky {dev:.2e}, yardstick {yard:.2e}, allowed {allowed:.2e}")
        assert kappa <= 1e6 and dev <= allowed
        assert fc.inverse_judge(S, X * (1.0 + 1e-9))[0] > allowed
        assert fc.inverse_judge(S, np.linalg.inv(S + 1e-6 * np.diag(np.diag(S))))[0] > allowed


def _plain_points(rt, mu, rule, scale):
    """(i, j, V, Y, Caa, C_bb) of a plain fp64 evaluation of the point formula in the observations' point-major order"""
    N, _ = pr.dense_system(rt)
    nA, cnp = rt.nA, rt.cnp
    dead = fc.full_map(rt)[0] < 0
    N[dead, :] = 0.0
    N[:, dead] = 0.0
    order = np.argsort(rt.i, kind="stable")
    i, j = rt.i[order], rt.j[order]
    V = np.stack([N[nA + 3 * q:nA + 3 * q + 3, nA + 3 * q:nA + 3 * q + 3] for q in range(rt.nP)])
    V[rt.held_pts] = np.eye(3)
    Vs = fc.damped_V(V, mu, rule)
    Y = np.stack([N[cnp * jj:cnp * jj + cnp, nA + 3 * ii:nA + 3 * ii + 3] @ np.linalg.inv(Vs[ii]) for ii, jj in zip(i, j)])
    Caa, _ = fc.schur_statement(rt, mu, rule, scale)
    Cbb = scale * np.linalg.inv(Vs)
    for a in range(i.size):
        for b in np.flatnonzero(i == i[a]):
            Cbb[i[a]] += Y[a].T @ Caa[cnp * j[a]:cnp * j[a] + cnp, cnp * j[b]:cnp * j[b] + cnp] @ Y[b]
    Cbb[rt.held_pts] = 0.0
    return i, j, V, Y, Caa, Cbb


@pytest.mark.parametrize("which", ["kd-bal", "fk"])
def test_a_plain_fp64_point_sum_passes_the_point_judge_and_faults_do_not(which):
    rt = p7(which)
    rule, mu, scale = MQ, 1e-6, 2.5
    i, j, V, Y, Caa, Cbb = _plain_points(rt, mu, rule, scale)
    pts = np.flatnonzero(~rt.held_pts)[:40]
    J = fc.point_judges(i, j, V, Y, Caa, mu, rule, scale, pts, rt.cnp)
    worst = max(float((np.abs(ar.ld(Cbb[q]) - J[q][2]).astype(np.float64) / J[q][1]).max()) for q in J)
    print(f"{which}: plain fp64 point sums, worst found / allowed {worst:.3f}")
    assert worst <= 1.0
    # mu I where Marquardt's D belongs, the j != k terms missing, scale applied twice
    for bad in (fc.point_judges(i, j, V, Y, Caa, mu, fr.NO_RULE, scale, pts, rt.cnp),
                fc.point_judges(i, j, V, Y, Caa, mu, rule, scale * scale, pts, rt.cnp)):
        assert max(float((np.abs(ar.ld(Cbb[q]) - bad[q][2]).astype(np.float64) / bad[q][1]).max()) for q in bad) > 1.0
    _, Cno = fc.schur_statement(rt, mu, rule, scale, "no-cross")
    assert max(float((np.abs(ar.ld(Cno[q]) - J[q][2]).astype(np.float64) / J[q][1]).max()) for q in J) > 1.0


@pytest.mark.parametrize("fault", fc.FAULTS)
def test_each_injected_fault_fails_the_agreement(fault):
    rt = ring()
    rule, mu, scale = MQ, 1e-3, 2.5
    ea, eb, tol = agree(rt, mu, rule, scale)
    assert ea <= tol and eb <= tol
    ea, eb, tol = agree(rt, mu, rule, scale, fault)
    print(f"{fault}: cameras {ea:.2e}, points {eb:.2e} (allowed {tol:.2e})")
    assert max(ea, eb) > tol
    if fault != "no-cross":
        assert ea > tol


def test_the_entry_points_exist():
    """the library exports the verbs (a null handle is refused before anything is touched) and capi.py binds them"""
    from psba_amd import capi
    assert capi.lib.psba_free_covariance_compute(None, 0.0, 1.0, 1) == -1
    assert capi.lib.psba_get_free_camera_covariance(None, 0, None, None) == -1
    for name in ("psba_get_free_covariance_matrix", "psba_get_free_point_covariance", "psba_get_free_sigmas",
                 "psba_free_covariance_times"):
        assert getattr(capi.lib, name)(None, None) == -1
    assert capi.lib.psba_get_free_point_blocks(None, None, None) == -1
    assert all(hasattr(capi.Psba, k) for k in ("free_covariance", "free_camera_covariance", "free_covariance_matrix",
                                               "free_point_covariance", "free_sigmas", "free_point_blocks",
                                               "free_covariance_times"))
