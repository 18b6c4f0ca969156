"""Observation weighting on the free-intrinsics routes (psba_set_obs_weighting) on the host: the reference
of tests/weight_ref.py against itself (central differences of F), its judges against a plain fp64 evaluation and
against injected faults, the contaminated ring scene on the dense twins, and the existence of the entry points.  No GPU."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import held_ref as hr
import prior_ref as pr
import weight_ref as wr
from freekd_twin import BAL, ring_problem, tiny_problem, wide_problem
from test_freekd_twin import P7, scaled_tol
from test_gpu_dense_solve import ETA_MAX

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

ROUTES = {"kd-all": (16, fr.ALL), "kd-bal": (16, BAL), "fk": (11, None)}
WIDE = {16: 65, 11: 94}
RULES = {"identity": fr.NO_RULE, "marquardt": fr.Rule(fr.MARQUARDT)}
KINDS = {"none": wr.NONE, "huber": wr.HUBER, "cauchy": wr.CAUCHY, "soft-l1": wr.SOFT_L1}


@functools.lru_cache(maxsize=None)
def prob(name, cnp=16):
    if name == "wide":
        return wide_problem(WIDE[cnp])
    return {"tiny": tiny_problem, "P7": P7}[name]()


@functools.lru_cache(maxsize=None)
def route(name, which, kind):
    """the holds and priors of test_prior_ref.py / test_gpu_priors.py with weight_ref.draw_weighting on top"""
    cnp, free = ROUTES[which]
    p = prob(name, cnp)
    nC, nP = int(p["nC"]), int(p["nP"])
    if name == "tiny":
        poses, pts = [1], [1]
    elif name == "P7":
        big, _ = hr.largest_pose_camera(p, cnp, free)
        poses, pts = sorted({0, 1, big}), [hr.point_with_views(p)]
    else:
        poses, pts = [0, 1, 3, 4, nC - 1], [0, nP - 1, hr.point_with_views(p)]
    rt0 = hr.HeldRoute(p, cnp, free, hr.flags(nC, poses), hr.flags(nP, pts))
    sigma, c = wr.draw_weighting(rt0, KINDS[kind])
    rt = wr.WeightRoute(p, cnp, pr.draw_priors(rt0), (KINDS[kind], c), sigma, free, rt0.held_poses, rt0.held_pts)
    return rt, wr.sums(rt)


def mu_of(rt, sm, rule):
    return 1e-3 if rule.marquardt else 1e-3 * float(np.concatenate([sm["diagU"], sm["diagV"]])[rt.free_all].max())


def test_the_drawn_weighting_is_what_the_tests_need():
    """sigma spans [0.5, 2]; both branches of Huber occur on every input, tiny included; the weighted cost is below
    the whitened sum of squares"""
    for name, which in (("tiny", "kd-all"), ("P7", "kd-bal"), ("wide", "fk")):
        rt, sm = route(name, which, "huber")
        s = sm["s"].astype(np.float64)
        assert rt.sigma.min() >= 0.5 and rt.sigma.max() <= 2.0 and rt.has_sigma and rt.weighted
        assert 4 * (s < rt.c ** 2).sum() >= rt.nO and 4 * (s > rt.c ** 2).sum() >= rt.nO
        om = (sm["w"] / ar.ld(rt.isig)).astype(np.float64)
        assert np.all(om[s <= rt.c ** 2] == 1.0) and np.all(om[s > rt.c ** 2] < 1.0)
        assert sm["cost_obs"] < float(s.sum()) and sm["cost"] > sm["cost_obs"]
    assert route("tiny", "kd-all", "huber")[0].nO == 4


@pytest.mark.parametrize("kind", ["huber", "cauchy", "soft-l1"])
def test_central_differences_of_F(kind):
    """-2 g of the weighted blocks is the derivative of F = sum rho(s) + priors on every free coordinate (IRLS drops
    only rho'' from the Hessian, nothing from the gradient); g of a held one is 0.  The route's own dense system gives
    the same g."""
    rt, sm = route("P7", "kd-bal", kind)
    cams, pts = rt.current()
    x0 = hr.flat(cams, pts)
    g = sm["g"].astype(np.float64)
    diag = np.concatenate([sm["diagU"], sm["diagV"]])
    F = sm["cost"]
    assert abs(wr.total_cost(rt, cams, pts) - F) <= 1e-12 * F
    assert np.all(g[rt.held_all] == 0.0)
    _, gd = pr.dense_system(rt)
    f = rt.free_all
    assert np.abs(gd[f] - g[f]).max() <= 1e-10 * np.abs(g).max()
    rng = np.random.default_rng(0)
    for k in rng.choice(np.flatnonzero(f), 36, replace=False):
        h = 1e-5 * np.sqrt(F / diag[k])
        vals = []
        for sgn in (1.0, -1.0):
            x = x0.copy()
            x[k] += sgn * h
            vals.append(wr.total_cost(rt, x[:rt.nA].reshape(rt.nC, rt.cnp), x[rt.nA:].reshape(rt.nP, 3)))
        cd = (vals[0] - vals[1]) / (2.0 * h)
        assert abs(cd + 2.0 * g[k]) <= 1e-6 * (np.sqrt(diag[k] * F) + abs(2.0 * g[k])), (k, cd, -2.0 * g[k])


WANTED = {"S", "e_a", "g", "max_diag", "dp_b", "new_cost", "residual cost", "residual cost_new", "prior_cur cams",
          "prior_new pts", "w_cur s", "w_cur w", "w_new s", "w_new w", "g ahead"}


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("name,which,kind", [
    ("tiny", "kd-all", "huber"), ("tiny", "fk", "cauchy"), ("P7", "kd-all", "soft-l1"), ("P7", "kd-bal", "huber"),
    ("P7", "kd-bal", "cauchy"), ("P7", "kd-bal", "none"), ("P7", "fk", "huber"), ("wide", "kd-bal", "cauchy"),
    ("wide", "fk", "soft-l1")])
def test_judges_pass_a_plain_evaluation(name, which, kind, rule):
    rt, sm = route(name, which, kind)
    rule = RULES[rule]
    mu = mu_of(rt, sm, rule)
    out = wr.judge(rt, sm, mu, rule, wr.plain_try(rt, mu, rule), scaled_tol(rt.p), ETA_MAX)
    assert WANTED <= set(out)
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, bad


def test_the_judges_pass_the_weighted_blocks_themselves():
    """psba_get_free_obs_blocks' judge on the plain fp64 products of the weighted blocks"""
    rt, sm = route("P7", "kd-bal", "cauchy")
    e, A, B, _ = rt.blocks()
    out = wr.blocks_judge(rt, sm, np.einsum("ark,arc->akc", A, B), B, e)
    assert max(out.values()) <= 1.0, out
    _, _, B0, _ = rt.blocks("B-unweighted")
    assert wr.blocks_judge(rt, sm, np.einsum("ark,arc->akc", A, B0), B0, e)["B"] > 1.0


EXPECT = {"B-unweighted": {"S", "g"}, "omega-unwhitened": {"S", "g"}, "rho-prime": {"S", "g"}, "sigma-twice": {"S", "g"},
          "cost-s": {"new_cost", "residual cost", "residual cost_new"},
          "prior-weighted": {"new_cost", "residual cost", "residual cost_new"}, "ahead-current": {"g ahead"}}


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("fault", wr.FAULTS)
def test_injected_faults_fail_the_judges(fault, rule):
    rt, sm = route("P7", "kd-bal", "cauchy")
    rule = RULES[rule]
    mu = mu_of(rt, sm, rule)
    out = wr.judge(rt, sm, mu, rule, wr.plain_try(rt, mu, rule, fault), scaled_tol(rt.p), ETA_MAX)
    bad = {k for k, v in out.items() if not v <= 1.0}
    assert EXPECT[fault] <= bad, (fault, out)
    if fault in ("cost-s", "prior-weighted", "ahead-current"):
        assert bad == EXPECT[fault], (fault, out)


LM_ITERS = 30


@functools.lru_cache(maxsize=None)
def ring_lm(kind, c=2.0):
    prob_, kc0, poses, bad = wr.contaminated_ring()
    t = wr.WeightTwin(prob_, (kind, c), None, kc0, BAL, poses)
    res, log = t.levmar(max_iter=LM_ITERS)
    return res, log, t.cams.copy(), t.s(), bad


def test_the_contaminated_ring_scene():
    """held_ring(7), 571 observations, {f, k1, k2}, poses 0 and 1 held, 45 observations (8 %) moved by 20 to 50 px, each
    on a different point and none on camera 0 or 1: the dense Cauchy twin (c = 2) ends at most 1/20 as far from the
    true focal lengths as the plain one, and s > 9 c^2 at its end flags exactly the moved observations."""
    _, _, K, _ = ring_problem()
    _, _, cams0, _, bad = ring_lm(wr.NONE)
    res, _, cams, s, _ = ring_lm(wr.CAUCHY)
    assert bad.size == 45 and res.final_err < res.init_err
    far0, far = np.abs(cams0[:, 0] - K[:, 0]).max(), np.abs(cams[:, 0] - K[:, 0]).max()
    assert 20.0 * far <= far0, (far, far0)
    assert np.array_equal(np.flatnonzero(s > 9.0 * 2.0 ** 2), bad)


def test_entry_points_exist():
    """the library exports the verbs (a null handle is refused before anything is touched) and capi.py binds them"""
    from psba_amd import capi
    assert capi.lib.psba_set_obs_weighting(None, 0, 1.0, None) == -1
    assert capi.lib.psba_obs_weighting(None, None, None, None) == -1
    assert capi.lib.psba_get_obs_weights(None, 0, None, None) == -1
    assert all(hasattr(capi.Psba, k) for k in ("set_obs_weighting", "obs_weighting", "get_obs_weights"))
