"""The host reference of shared intrinsics (tests/shared_ref.py; no GPU): J P against central differences with all
members perturbed together, the folded 80-bit blocks against the dense Schur complement of P^T N P, the judges applied
to a plain fp64 evaluation and to four injected faults, and the shared twin's LM on the ring scene."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import shared_ref as sr
from freekd_twin import BAL, CNP, ring_problem, start_kc, tiny_problem, wide_problem
from test_freekd_twin import P7
from test_gpu_dense_solve import ETA_MAX

needs_ld = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")
MASKS = {"all": fr.ALL, "bal": BAL}
P7_LABELS = {"one": [0] * 7, "two": [0, 1, 0, 1, 0, 1, 0]}


@functools.lru_cache(maxsize=None)
def problem(name):
    return {"tiny": tiny_problem, "P7": P7, "64": lambda: wide_problem(64), "65": lambda: wide_problem(65)}[name]()


def labels_of(name, which="groups"):
    p = problem(name)
    if which == "one":
        return np.zeros(p["nC"], dtype=int)
    return np.zeros(2, dtype=int) if name == "tiny" else sr.wide_labels(p["nC"])


def test_labels_are_what_the_tests_claim():
    p = problem("65")
    lab = sr.wide_labels(65)
    rep = sr.representatives(lab)
    per_cam = np.bincount(p["jidx"], minlength=65)
    assert list(rep[:6]) == [0, 0, 0, 3, 4, 5] and rep[20] == 4 and rep[40] == 4
    assert per_cam[4] == 0 and per_cam[3] == 1                 # a representative without observations, a lone camera with one
    assert (rep == 3).sum() == 1 and (rep == 5).sum() == 1 and (rep == 0).sum() == 3 and (rep == 4).sum() == 3
    assert sr.group_obs_max(p, lab) >= 64 + 65 + 63
    assert np.array_equal(sr.representatives([7, 7, 3, 7, 3]), [0, 0, 2, 0, 2])
    phi, away = sr.fold_map([0, 0, 2], BAL)
    assert list(np.flatnonzero(away)) == [16 + 0, 16 + 5, 16 + 6] and phi[16 + 5] == 5 and phi[16 + 1] == 16 + 1


@pytest.mark.parametrize("which", list(P7_LABELS))
def test_shared_columns_against_central_differences(which):
    """All members of a group perturbed together; the accuracy of test_twin_jacobian_against_central_differences."""
    p = problem("P7")
    t = sr.SharedTwin(p, P7_LABELS[which], start_kc(p["nC"]))
    _, JP = t.jacobian_shared()
    assert JP.shape[1] == t.nT - 10 * (p["nC"] - len(set(P7_LABELS[which])))
    for g in np.unique(t.rep):
        members = np.flatnonzero(t.rep == g)
        for k in range(10):
            h = 1e-6 * max(1.0, np.abs(t.cams[:, k]).max())
            cp, cm = t.cams.copy(), t.cams.copy()
            cp[members, k] += h
            cm[members, k] -= h
            num = -(t.residual(cams=cp) - t.residual(cams=cm)).reshape(-1) / (2 * h)
            t._set(None, None)
            err = np.abs(JP[:, t.col[CNP * g + k]] - num).max() / np.abs(num).max()
            assert err <= 1e-6, f"group {g} column {k}: {err:.2e}"


@needs_ld
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("name,which", [("tiny", "groups"), ("64", "groups"), ("65", "groups"), ("65", "one")])
def test_folded_blocks_against_the_dense_schur_complement(name, which, mask):
    """fold(schur_blocks) (80-bit, block by block, then folded) against S of the dense P^T N P (fp64, formed from J P
    in the reduced numbering, embedded): inside a quarter of the tolerance, as the unshared twin's own test asks."""
    p, lab = problem(name), labels_of(name, which)
    rt = sr.SharedRoute(p, lab, MASKS[mask])
    t = sr.SharedTwin(p, lab, start_kc(p["nC"]), MASKS[mask])
    cost, Nr, gr = t.normal_shared()
    N, g = t.embed(Nr, gr)
    sm = fr.sums(rt)
    mus, fdiag = sr.dampings(rt, sm)
    assert abs(t.max_diag_shared(Nr) - 1e3 * mus["big"]) <= 1e-11 * 1e3 * mus["big"]
    for mu in mus.values():
        S, ea = t.schur(N, g, mu)
        Sx, eax = sr.fold(*rt.twin.schur_blocks(mu), rt.rep, rt.free, mu)
        d = np.sqrt(fdiag[:rt.nA] + mu)
        eS, ee = sr.scaled_errors(S, ea, Sx.astype(np.float64), eax.astype(np.float64), d, cost)
        print(f"{name} {which} {mask} mu {mu:.3e}: S {eS:.2e}, e_a {ee:.2e} (tol {rt.tol:.2e})")
        assert max(eS, ee) <= 0.25 * rt.tol
        sr.check_embedded(Sx.astype(np.float64), eax.astype(np.float64), rt.away, 1.0 + mu)


@functools.lru_cache(maxsize=None)
def plain(name, which, mask, which_mu):
    p, lab = problem(name), labels_of(name, which)
    rt = sr.SharedRoute(p, lab, MASKS[mask])
    sm = fr.sums(rt)
    mus, fdiag = sr.dampings(rt, sm)
    mu = mus[which_mu]
    Sx, eax = sr.fold(*rt.twin.schur_blocks(mu), rt.rep, rt.free, mu)
    return rt, sm, mu, fdiag, Sx.astype(np.float64), eax.astype(np.float64), sr.plain_try(rt, mu)


def judge_system(rt, sm, mu, fdiag, Sx, eax, S, ea):
    """what the GPU test asks of [S | e_a]: the scaled measure, the mirror, the embedded structure"""
    d = np.sqrt(fdiag[:rt.nA] + mu)
    eS, ee = sr.scaled_errors(S, ea, Sx, eax, d, sm["cost"])
    assert eS <= rt.tol and ee <= rt.tol, f"scaled S {eS:.3e}, e_a {ee:.3e}, tol {rt.tol:.3e}"
    sr.check_mirror(S)
    sr.check_embedded(S, ea, rt.away, 1.0 + mu)
    return eS, ee


@needs_ld
@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name,which,mask", [("tiny", "groups", "all"), ("tiny", "groups", "bal"), ("65", "groups", "all"),
                                             ("65", "groups", "bal"), ("65", "one", "bal")])
def test_judges_pass_a_plain_evaluation(name, which, mask, which_mu):
    rt, sm, mu, fdiag, Sx, eax, tr = plain(name, which, mask, which_mu)
    eS, ee = judge_system(rt, sm, mu, fdiag, Sx, eax, tr["S"], tr["ea"])
    print(f"{name} {which} {mask} {which_mu}: S {eS / rt.tol:.2e}, e_a {ee / rt.tol:.2e} of tol")
    assert max(eS, ee) <= 0.5 * rt.tol
    # the fold alone, against the unfolded plain buffer
    S1, ea1, _ = fr.plain_schur(rt, mu)
    n32 = (rt.nA + 31) // 32 * 32
    M = np.zeros((n32 + 1, n32))
    M[:rt.nA, :rt.nA], M[n32, :rt.nA] = S1, ea1
    Fx, Fb, ex, eb, _ = sr.fold_bound(M, rt.rep, rt.free, mu)
    low = np.tril(np.ones((rt.nA, rt.nA), dtype=bool))
    rS, _ = ar.excess(tr["S"][low], Fx[low], Fb[low])
    re, _ = ar.excess(tr["ea"], ex, eb)
    print(f"  the fold alone: S {rS:.2e}, e_a {re:.2e} of the bound")
    assert rS <= 1.0 and re <= 1.0
    # dp
    eta, fe, kappa = fr.solve_judge(tr["S"], tr["ea"], tr["dp_embedded"])
    assert eta <= 0.5 * ETA_MAX and fe <= 0.5 * 2 * kappa * 1e-14
    r, b = fr.dpb_residual(rt, sm, tr["dp"], mu)
    assert ar.excess(r, np.zeros(r.shape, ar.LD), b)[0] <= 0.5
    for what, (x, bound) in sr.scalars(rt, sm, tr["dp"], tr["newcams"], tr["newpts"], mu).items():
        ratio = float(abs(ar.LD(tr["sc"][what]) - x) / bound)
        print(f"  {what} {ratio:.2e}")
        assert ratio <= 0.5, what
    # the expanded step: members carry their representative's entries
    dpa = tr["dp"][:rt.nA].reshape(-1, CNP)
    free = np.flatnonzero(np.asarray(rt.free))
    assert np.array_equal(dpa[:, free], dpa[rt.rep][:, free])
    assert np.array_equal(tr["newcams"][:, :10], tr["newcams"][rt.rep][:, :10])


@needs_ld
@pytest.mark.parametrize("which_mu", ["big", "small"])
def test_injected_faults_fail_the_judges(which_mu):
    rt, sm, mu, fdiag, Sx, eax, tr = plain("65", "groups", "bal", which_mu)
    S1, ea1, _ = fr.plain_schur(rt, mu)
    judge_system(rt, sm, mu, fdiag, Sx, eax, *sr.plain_fold(S1, ea1, rt.rep, rt.free, mu))
    faults = {"mu counted n_g times": dict(mu_per_member=True), "one member left out of a sum": dict(skip=(2, 0)),
              "upper triangle not mirrored": dict(mirror=False), "a non-representative row left uncleared": dict(clear=False)}
    for what, kw in faults.items():
        S, ea = sr.plain_fold(S1, ea1, rt.rep, rt.free, mu, **kw)
        with pytest.raises(AssertionError):
            judge_system(rt, sm, mu, fdiag, Sx, eax, S, ea)
        print(f"{what}: caught")
    # each fault is caught by the check that is meant for it
    S, ea = sr.plain_fold(S1, ea1, rt.rep, rt.free, mu, mu_per_member=True)
    d = np.sqrt(fdiag[:rt.nA] + mu)
    assert sr.scaled_errors(S, ea, Sx, eax, d, sm["cost"])[0] > rt.tol
    S, ea = sr.plain_fold(S1, ea1, rt.rep, rt.free, mu, skip=(2, 0))
    assert min(sr.scaled_errors(S, ea, Sx, eax, d, sm["cost"])) > rt.tol
    S, ea = sr.plain_fold(S1, ea1, rt.rep, rt.free, mu, mirror=False)
    with pytest.raises(AssertionError, match="upper triangle"):
        sr.check_mirror(S)
    S, ea = sr.plain_fold(S1, ea1, rt.rep, rt.free, mu, clear=False)
    with pytest.raises(AssertionError, match="folded-away"):
        sr.check_embedded(S, ea, rt.away, 1.0 + mu)
    # dp_l2 that counts the members' copies misses its envelope
    want = sr.scalars(rt, sm, tr["dp"], tr["newcams"], tr["newpts"], mu)["dp_l2"]
    assert abs(ar.LD(float(tr["dp"] @ tr["dp"])) - want[0]) > want[1]


def test_shared_ring_is_the_ring_scene():
    a, b = sr.shared_ring(np.arange(6)), ring_problem()
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    for key in ("K", "initrot", "cams", "pts", "impts", "iidx", "jidx"):
        assert np.array_equal(a[0][key], b[0][key]), key


RING_LABELS = {"two": [0, 1, 0, 1, 0, 1], "one": [0] * 6, "mixed": [0, 0, 1, 1, 2, 3]}


@pytest.mark.parametrize("which", list(RING_LABELS))
def test_shared_twin_recovers_the_ring_scene(which):
    """The thresholds of test_gpu_freekd.py::test_recovery_of_the_ring_scene, which the GPU test of the shared route
    asserts too: final <= 1e-15 init, f <= 1e-9, k1 <= 1e-8, k2 <= 1e-7 (relative to the truth's size as there)."""
    lab = RING_LABELS[which]
    start, kc0, K_true, kc_true = sr.shared_ring(lab)
    t = sr.SharedTwin(start, lab, kc0, BAL)
    res, log = t.levmar_shared(max_iter=30, stop_small=False)
    f = np.abs(t.cams[:, 0] / K_true[:, 0] - 1).max()
    k1 = np.abs(t.cams[:, 5] - kc_true[:, 0]).max()
    k2 = np.abs(t.cams[:, 6] - kc_true[:, 1]).max()
    print(f"{which}: iterations {res.iters}, cost {res.final_err:.2e} of {res.init_err:.2e}, f {f:.1e}, k1 {k1:.1e}, "
          f"k2 {k2:.1e}")
    assert res.final_err <= 1e-15 * res.init_err
    assert f <= 1e-9 and k1 <= 1e-8 and k2 <= 1e-7
    assert np.array_equal(t.cams[:, :10], t.cams[t.rep][:, :10])
