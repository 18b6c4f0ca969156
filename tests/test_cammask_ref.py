"""Per-camera intrinsics masks on the 16-block route (psba_set_camera_masks) on the host: the reference of
tests/cammask_ref.py against itself (the reduced statement against the embedded one, equal rows against the global
mask), its judges against a plain fp64 evaluation and against injected faults, the fold with a table constant on every
group, the dense LM of the recovery scene, and the existence of the entry points.  No GPU."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import cammask_ref as cm
import free_ref as fr
import held_ref as hr
import shared_ref as sr
import weight_ref as wr
from freekd_twin import BAL, CNP, tiny_problem, wide_problem
from test_freekd_twin import scaled_tol
from test_gpu_dense_solve import ETA_MAX

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

RULES = {"identity": fr.NO_RULE, "marquardt": fr.Rule(fr.MARQUARDT)}


@functools.lru_cache(maxsize=None)
def prob(name):
    return tiny_problem() if name == "tiny" else wide_problem(65)


@functools.lru_cache(maxsize=None)
def route(name):
    """the mixed table, all ten free globally, poses 0 and 2 held (camera 2 has the row none: wholly fixed; tiny has
    two cameras: pose 1)"""
    p = prob(name)
    nC = int(p["nC"])
    rt = cm.CamMaskRoute(p, cm.mixed_table(nC), fr.ALL, hr.flags(nC, [1] if name == "tiny" else [0, 2]))
    return rt, wr.sums(rt)


def mu_of(rt, sm, rule):
    return 1e-3 if rule.marquardt else hr.dampings(rt, sm)[0]["big"]


def judged(rt, sm, mu, rule, tr):
    """weight_ref.judge (every judge the GPU test applies to a try) -> the ratios above 1; its exact parts assert"""
    out = wr.judge(rt, sm, mu, rule, tr, scaled_tol(rt.p), ETA_MAX)
    assert {"S", "e_a", "g", "max_diag", "dp_a eta", "dp_b", "dp_l2", "gain_den", "new_cost"} <= set(out)
    return {k: v for k, v in out.items() if not v <= 1.0}


def test_the_route_masks_what_the_table_says():
    rt, sm = route("wide")
    nC = rt.nC
    assert rt.cam_free.sum(axis=1).tolist() == [(10, 3, 0, 1)[j % 4] for j in range(nC)]
    assert rt.held_global.size == 0 and rt.held_table.size == 10 * nC - int(rt.cam_free.sum())
    assert rt.held.size == rt.held_table.size + 12 and rt.fixed_cams.tolist() == [2]
    e, A, B, _ = rt.blocks()
    assert np.all(A[:, :, :10][np.repeat(~rt.cam_free[rt.j][:, None, :], 2, axis=1)] == 0.0)
    assert np.all(A[:, :, 0][rt.cam_free[rt.j][:, 0]] != 0.0)
    assert np.all(sm["diagU"][rt.held] == 1.0) and np.all(sm["g"][rt.held] == 0)
    assert np.all(sm["W"][:, :10, :][~rt.cam_free[rt.j]] == 0)
    # the AND: a global mask g with rows c is the route of the global mask all free with rows g & c
    tab = cm.mixed_table(nC)
    a = cm.CamMaskRoute(rt.p, tab, BAL)
    b = cm.CamMaskRoute(rt.p, tab & np.asarray(BAL, dtype=np.uint8)[None, :], fr.ALL)
    assert np.array_equal(a.held, b.held) and np.array_equal(a.blocks()[1], b.blocks()[1])


@pytest.mark.parametrize("row", [cm.F_K1_K2, cm.NONE])
def test_equal_rows_are_the_global_mask(row):
    """a table whose rows all equal m under the global mask all free is free_ref's route of the global mask m: the
    same held set, the same blocks, the same 80-bit S and e_a"""
    p = prob("tiny")
    a = cm.CamMaskRoute(p, cm.constant_table(2, row), fr.ALL)
    b = hr.HeldRoute(p, 16, row)
    assert np.array_equal(a.held, b.held) and a.held_table.size == a.held.size
    for x, y in zip(a.blocks(), b.blocks()):
        assert np.array_equal(x, y)
    sa, sb = wr.sums(a), hr.sums(b)
    mu = hr.dampings(b, sb)[0]["big"]
    for x, y in zip(hr.schur_ref(a, sa, mu), hr.schur_ref(b, sb, mu)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_reduced_against_embedded(name):
    """The dense solve with the masked and held columns deleted, scattered back with zeros, equals the embedded solve
    with placeholders to 1e-10 relative at mu = 1e-3 max diag."""
    rt, sm = route(name)
    mu = hr.dampings(rt, sm)[0]["big"]
    red = hr.reduced_solve(rt, mu)
    emb, N, g = hr.embedded_solve(rt, mu)
    assert np.all(red[rt.held_all] == 0.0) and np.all(g[rt.held_all] == 0.0)
    off = N[rt.held_all].copy()
    off[np.arange(rt.held_all.size), rt.held_all] = 0.0
    assert np.all(off == 0.0) and np.all(N[rt.held_all, rt.held_all] == 1.0)
    err = np.abs(red - emb).max() / np.abs(red).max()
    print(f"{name}: reduced against embedded {err:.3e}")
    assert err <= 1e-10


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_judges_pass_a_plain_evaluation(name, rule):
    rt, sm = route(name)
    rule = RULES[rule]
    mu = mu_of(rt, sm, rule)
    tr = cm.plain_try(rt, mu, rule)
    bad = judged(rt, sm, mu, rule, tr)
    assert not bad, bad
    cm.check_table_parts(rt, tr["W"], tr["cams"], tr["newcams"])


@functools.lru_cache(maxsize=None)
def largest_masked():
    """wide_problem(65) with every pose held (the points and the intrinsics move) and the row none on the camera that
    holds the largest entry of the intrinsics' diagonal: a max_diag that forgets the table reports that entry"""
    p = prob("wide")
    nC = int(p["nC"])
    poses = np.ones(nC, dtype=np.uint8)
    rt0 = hr.HeldRoute(p, 16, fr.ALL, poses)
    sm0 = hr.sums(rt0)
    d = sm0["diagU"].copy()
    d[rt0.held] = 0.0
    big = int(np.argmax(d)) // CNP
    assert d.max() > 1.001 * sm0["diagV"].max()
    table = cm.constant_table(nC, fr.ALL)
    table[big] = 0
    rt = cm.CamMaskRoute(p, table, fr.ALL, poses)
    return rt, wr.sums(rt)


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("fault", ["masked-column", "no-placeholder", "max-diag-masked"])
def test_injected_faults_fail_the_judges(fault, rule):
    """one masked column left in A, the placeholder missing on one diagonal, max_diag taken over a masked coordinate:
    each must be rejected, by a ratio above 1 or by one of the exact assertions"""
    rt, sm = largest_masked() if fault == "max-diag-masked" else route("wide")
    rule = RULES[rule]
    mu = mu_of(rt, sm, rule)
    assert not judged(rt, sm, mu, rule, cm.plain_try(rt, mu, rule))
    tr = cm.plain_try(rt, mu, rule, fault)
    try:
        bad = judged(rt, sm, mu, rule, tr)
    except AssertionError as err:
        bad = {"exact": str(err)}
    print(f"{fault} {rule}: {bad}")
    assert bad, f"{fault} passed the judges"
    if fault == "max-diag-masked":
        assert set(bad) == {"max_diag"}


# ---- groups ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shared_route():
    p = prob("wide")
    lab = sr.wide_labels(65)
    rt = cm.CamMaskSharedRoute(p, lab, cm.group_table(lab), fr.ALL)
    return rt, hr.sums(rt)


def test_the_fold_with_a_table_constant_on_every_group():
    """The plain fp64 fold over the coordinates free for the group holds shared_tol against the 80-bit fold; a
    coordinate masked for a group is not shared: placeholder 1 + mu on every member, the representative included; a
    fold that sums it fails"""
    rt, sm = shared_route()
    nA, cost = rt.nA, sm["cost"]
    tab = cm.group_table(rt.labels)
    assert {tuple(r) for r in tab.tolist()} == set(cm.MIXED_ROWS)          # mixed across the groups
    assert np.array_equal(tab, tab[rt.rep])
    groups = np.bincount(rt.rep, minlength=rt.nC)
    assert np.any((groups > 1) & ~rt.cam_free.all(axis=1)) and np.any((groups > 1) & rt.cam_free.all(axis=1))
    assert not np.any(rt.away[rt.held]) and np.array_equal(rt.phi[rt.held], rt.held)
    mus, fdiag = sr.dampings(rt, sm)
    mu = mus["big"]
    S_want, ea_want = cm.shared_schur_ref(rt, sm, mu)
    d = np.sqrt(fdiag[:nA] + mu)
    S, ea = cm.plain_shared_system(rt, mu)
    eS, ee = sr.scaled_errors(S, ea, S_want, ea_want, d, cost)
    print(f"plain fold: S {eS / rt.tol:.3e}, e_a {ee / rt.tol:.3e}")
    assert eS <= rt.tol and ee <= rt.tol
    sr.check_mirror(S)
    sr.check_embedded(S, ea, rt.away, 1.0 + mu)
    hr.check_held_system(rt, S, ea, mu)
    Sf, eaf = cm.plain_shared_system(rt, mu, fault="fold-masked")
    eS, _ = sr.scaled_errors(Sf, eaf, S_want, ea_want, d, cost)
    assert eS > rt.tol
    with pytest.raises(AssertionError):
        hr.check_held_system(rt, Sf, eaf, mu)
    # the reference's own fault switch: the 80-bit fold that sums the placeholders differs from the one that does not
    Sx, _ = cm.shared_schur_ref(rt, sm, mu, fault="fold-masked")
    reps = np.intersect1d(rt.held_table, CNP * np.flatnonzero(groups > 1)[:, None] + np.arange(10)[None, :])
    assert reps.size and np.all(Sx[reps, reps] > S_want[reps, reps] + 0.5)


def test_unequal_rows_inside_a_group_are_refused():
    p = prob("wide")
    lab = sr.wide_labels(65)
    tab = cm.group_table(lab)
    tab[1] = 1 - tab[0]
    with pytest.raises(AssertionError, match="camera 1 "):
        cm.CamMaskSharedRoute(p, lab, tab, fr.ALL)


# ---- the dense LM of the recovery scene -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ring_twin_lm():
    start, kc0, poses, table, K_true, kc_true = cm.mixed_ring()
    t = cm.CamMaskTwin(start, table, kc0, fr.ALL, poses)
    c0 = t.cams.copy()
    res, log = t.levmar(max_iter=30)
    return t, c0, res, log, K_true, kc_true


def test_the_twin_recovers_the_mixed_ring():
    """cameras 0, 2, 4 at their true K and kc with the row none, cameras 1, 3, 5 from the scene's start with
    {f, k1, k2}, poses 0 and 1 held: the dense LM with the masked and held columns deleted ends on the absolute stop
    within 30 iterations; the fixed cameras keep their bits"""
    t, c0, res, log, K_true, kc_true = ring_twin_lm()
    free = list(cm.RING_FREE_CAMS)
    f = np.abs(t.cams[free, 0] - K_true[free, 0]).max()
    k1 = np.abs(t.cams[free, 5] - kc_true[free, 0]).max()
    k2 = np.abs(t.cams[free, 6] - kc_true[free, 1]).max()
    print(f"iterations {res.iters} flag {res.flag}: cost {res.final_err:.3e} of {res.init_err:.3e}, f {f:.2e}, "
          f"k1 {k1:.2e}, k2 {k2:.2e}")
    assert res.flag == 3 and res.iters <= 30 and res.final_err <= 1e-12
    assert f <= 1e-5 and k1 <= 1e-7 and k2 <= 1e-6
    fixed = list(cm.RING_FIXED_CAMS)
    assert t.cams[fixed, :10].tobytes() == c0[fixed, :10].tobytes() and t.cams[:2, 10:].tobytes() == c0[:2, 10:].tobytes()
    assert np.all(t.cams[free, 0] != c0[free, 0])
    keep = t.keep[:t.nA].reshape(6, CNP)
    assert keep[:, :10].sum(axis=1).tolist() == [0, 3, 0, 3, 0, 3] and keep[:, 10:].all(axis=1).tolist() == [False, False] + [True] * 4


def test_entry_points_exist():
    """fails on a library without the verbs: a NULL handle is PSBA_E_INVALID (-1), not a missing symbol"""
    from psba_amd import capi
    assert capi.lib.psba_set_camera_masks(None, None) == -1
    assert capi.lib.psba_camera_masks(None, None) == -1
    assert hasattr(capi.Psba, "set_camera_masks") and hasattr(capi.Psba, "camera_masks")
