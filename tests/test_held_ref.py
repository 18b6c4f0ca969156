"""Held poses and points on the free-intrinsics routes (psba_set_held) on the host: the reference of
tests/held_ref.py against itself (the reduced statement against the embedded one), its judges against a plain fp64
evaluation and against injected faults, the two conditioning facts the GPU tests stand on, the dense LM with holds on
the ring scene, and the existence of the entry points.  No GPU."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import held_ref as hr
from freekd_twin import BAL, tiny_problem
from test_freekd_twin import P7, scaled_tol

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

ROUTES = {"kd-all": (16, fr.ALL), "kd-bal": (16, BAL), "fk": (11, None)}


@functools.lru_cache(maxsize=None)
def prob(name):
    return {"tiny": tiny_problem, "P7": P7}[name]()


@functools.lru_cache(maxsize=None)
def route(name, which):
    """tiny: pose 1 and point 1 (seen once) held; P7: poses 0 and 1, the camera with the largest pose diagonal, and
    one point with at least three views"""
    cnp, free = ROUTES[which]
    p = prob(name)
    if name == "tiny":
        poses, pts = [1], [1]
    else:
        big, _ = hr.largest_pose_camera(p, cnp, free)
        poses, pts = sorted({0, 1, big}), [hr.point_with_views(p)]
    rt = hr.HeldRoute(p, cnp, free, hr.flags(p["nC"], poses), hr.flags(p["nP"], pts))
    return rt, hr.sums(rt)


def test_the_route_holds_what_it_says():
    rt, sm = route("P7", "kd-bal")
    assert rt.held_poses.sum() >= 2 and rt.held_pts.sum() == 1
    assert rt.held.size == 7 * rt.nC + 6 * int(rt.held_poses.sum()) and rt.held_b.size == 3
    e, A, B, _ = rt.blocks()
    assert np.all(A[rt.held_poses[rt.j]][:, :, 10:] == 0.0) and np.any(A[~rt.held_poses[rt.j]][:, :, 10:] != 0.0)
    assert np.all(A[:, :, [0, 5, 6]] != 0.0)                # the intrinsics of a held pose stay free
    assert np.all(B[rt.held_pts[rt.i]] == 0.0) and np.all(np.abs(B[~rt.held_pts[rt.i]]).sum(axis=(1, 2)) > 0)
    assert np.all(sm["diagU"][rt.held] == 1.0) and np.all(sm["diagV"][rt.held_b] == 1.0)
    mine = np.r_[rt.held_pose, rt.nA + rt.held_b]           # (a masked intrinsic keeps free_ref's group slack)
    assert np.all(sm["g"][rt.held_all] == 0) and np.all(sm["envg"][mine] == 0.0)
    assert np.all(sm["W"].reshape(rt.nO, -1)[rt.held_pts[rt.i]] == 0)
    # the largest entry of the unheld diagonal belongs to a held pose: a max_diag that forgets the mask reports it
    assert hr.largest_pose_camera(rt.p, 16, BAL)[1]
    assert hr.plain_try(rt, 1.0, fault="max-diag-all")["max_diag"] > 1.001 * hr.dampings(rt, sm)[0]["big"] * 1e3


@pytest.mark.parametrize("which", list(ROUTES))
@pytest.mark.parametrize("name", ["tiny", "P7"])
def test_reduced_against_embedded(name, which):
    """The dense solve with the held columns deleted, scattered back with zeros, equals the embedded solve with
    placeholders to 1e-10 relative at mu = 1e-3 max diag, for blocks of 11 and of 16."""
    rt, sm = route(name, which)
    mu = hr.dampings(rt, sm)[0]["big"]
    red = hr.reduced_solve(rt, mu)
    emb, N, g = hr.embedded_solve(rt, mu)
    assert np.all(red[rt.held_all] == 0.0) and np.all(g[rt.held_all] == 0.0)
    off = N[rt.held_all].copy()
    off[np.arange(rt.held_all.size), rt.held_all] = 0.0
    assert np.all(off == 0.0) and np.all(N[rt.held_all, rt.held_all] == 1.0)
    err = np.abs(red - emb).max() / np.abs(red).max()
    print(f"{name} {which}: reduced against embedded {err:.3e}")
    assert err <= 1e-10
    assert np.abs(emb[rt.held_all]).max() <= 1e-10 * np.abs(red).max()


def judge(rt, sm, mu, rule, tr):
    """every judge the GPU test applies to a try, on the dict of held_ref.plain_try"""
    hr.check_max_diag(rt, sm, tr["max_diag"])
    hr.check_held_system(rt, tr["S"], tr["ea"], mu, rule)
    hr.check_held_step(rt, tr["g"], tr["dp"], hr.flat(tr["cams"], rt.twin.pts), hr.flat(tr["newcams"], tr["newpts"]))
    S_want, ea_want = hr.schur_ref(rt, sm, mu, rule)
    d = fr.scale_diag(rt, sm, mu, rule)
    tol = scaled_tol(rt.p)
    eS = (np.abs(tr["S"] - S_want) / np.outer(d, d)).max()
    ee = (np.abs(tr["ea"] - ea_want) / (d * np.sqrt(sm["cost"]))).max()
    assert eS <= tol and ee <= tol, f"scaled S {eS:.3e}, e_a {ee:.3e}, tol {tol:.3e}"
    r, bound = fr.dpb_residual(rt, sm, tr["dp"], mu, rule)
    ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), bound)
    assert ratio <= 1.0, f"dp_b of point {k // 3}: {ratio:.3e}"
    D = tr["D"] if rule.marquardt else None
    for what, (x, b) in fr.scalars(rt, sm, tr["dp"], tr["newcams"], tr["newpts"], mu, D=D).items():
        assert abs(ar.LD(tr["sc"][what]) - x) <= b, what


RULES = {"identity": fr.NO_RULE, "marquardt": fr.Rule(fr.MARQUARDT)}


def mu_of(rt, sm, rule):
    return 1e-3 if rule.marquardt else hr.dampings(rt, sm)[0]["big"]


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("which", list(ROUTES))
@pytest.mark.parametrize("name", ["tiny", "P7"])
def test_judges_pass_a_plain_evaluation(name, which, rule):
    rt, sm = route(name, which)
    rule = RULES[rule]
    mu = mu_of(rt, sm, rule)
    judge(rt, sm, mu, rule, hr.plain_try(rt, mu, rule))


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("fault", ["pose-column", "no-placeholder", "point-g", "max-diag-all"])
def test_injected_faults_fail_the_judges(fault, rule):
    """a held pose column left non-zero, a missing placeholder, a held point with g_b != 0, a max_diag that ignores
    the mask: each must be rejected (7camsvarK, {f, k1, k2})"""
    rt, sm = route("P7", "kd-bal")
    rule = RULES[rule]
    mu = mu_of(rt, sm, rule)
    tr = hr.plain_try(rt, mu, rule, fault)
    with pytest.raises(AssertionError):
        judge(rt, sm, mu, rule, tr)
    # ... and by the judge that is there for it
    own = {"pose-column": lambda: hr.check_held_system(rt, tr["S"], tr["ea"], mu, rule),
           "no-placeholder": lambda: hr.check_held_system(rt, tr["S"], tr["ea"], mu, rule),
           "point-g": lambda: hr.check_held_step(rt, tr["g"], tr["dp"], hr.flat(tr["cams"], rt.twin.pts),
                                                 hr.flat(tr["newcams"], tr["newpts"])),
           "max-diag-all": lambda: hr.check_max_diag(rt, sm, tr["max_diag"])}[fault]
    with pytest.raises(AssertionError):
        own()


def test_conditioning_facts():
    """What the GPU tests stand on (7camsvarK, {f, k1, k2}): without holds the diagonally scaled S is singular at
    mu = 0; with poses 0 and 1 held the scaled reduced S has a condition number of at most 1e6."""
    p = prob("P7")
    free_rt = hr.HeldRoute(p, 16, BAL)
    lam = np.linalg.eigvalsh(hr.reduced_scaled_S(free_rt))
    print(f"no holds: smallest eigenvalue of the scaled S {lam[0]:.3e}")
    assert lam[0] <= 1e-12
    rt = hr.HeldRoute(p, 16, BAL, hr.flags(p["nC"], [0, 1]))
    lam = np.linalg.eigvalsh(hr.reduced_scaled_S(rt))
    print(f"poses 0 and 1 held: condition of the scaled reduced S {lam[-1] / lam[0]:.3e}")
    assert lam[0] > 0 and lam[-1] / lam[0] <= 1e6


@functools.lru_cache(maxsize=None)
def ring_lm():
    start, kc0, poses = hr.held_ring()
    t = hr.HeldTwin(start, kc0, BAL, poses)
    cams0 = t.cams.copy()
    res, log = t.levmar(max_iter=30)
    return res, log, cams0, t


def test_held_twin_recovers_the_ring_scene():
    """the dense LM with the true poses of cameras 0 and 1 held, {f, k1, k2} free: the cost falls by more than six
    orders of magnitude and the held poses do not move"""
    res, log, cams0, t = ring_lm()
    print(f"ring scene, poses 0 and 1 held: {res.init_err:.6e} -> {res.final_err:.6e} in {res.iters} iterations")
    assert res.final_err <= 1e-6 * res.init_err
    assert t.cams[:2, 10:].tobytes() == cams0[:2, 10:].tobytes()
    assert np.any(t.cams[2:, 10:] != cams0[2:, 10:]) and np.any(t.cams[:2, 0] != cams0[:2, 0])


def test_entry_points_exist():
    """fails on a library without the verbs: a NULL handle is PSBA_E_INVALID (-1), not a missing symbol"""
    from psba_amd import capi
    assert capi.lib.psba_set_held(None, None, None) == -1
    assert capi.lib.psba_held_counts(None, None, None) == -1
    assert hasattr(capi.Psba, "set_held") and hasattr(capi.Psba, "held_counts")
