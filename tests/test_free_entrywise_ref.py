"""The inputs and judges of tests/test_gpu_free_entrywise.py on the host (no GPU): the fp64 twin against its own sums
in extended precision on the new inputs, the closed-form 3 x 3 inverse against the L D L^T substitution where it
matters (why kernels_free.hip forms Y and dp_b by substitution), the dp_b / dp_a / try-scalar judges of
tests/free_ref.py applied to a plain fp64 evaluation, and injected faults each judge must catch -- under N + mu I and
under Marquardt's N + mu D (psba_set_damping)."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
from freekd_twin import BAL, TwinKD, WIDE_COUNTS, many_obs_problem, start_kc, tiny_problem, wide_problem
from test_freekd_twin import P7, scaled_tol
from test_gpu_dense_solve import ETA_MAX

needs_ld = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")
MASKS = {"all": fr.ALL, "bal": BAL, "k-only": fr.K_ONLY}


@functools.lru_cache(maxsize=None)
def wide(nC):
    return wide_problem(nC)


def two_mus(t, N):
    return 1e-3 * t.max_diag(N), 1e-6 * float(np.median(np.diag(N)))


@pytest.mark.parametrize("nC", [64, 65, 93, 94])
def test_wide_problem_is_what_it_claims(nC):
    p = wide(nC)
    per_cam = np.bincount(p["jidx"], minlength=nC)
    per_pt = np.bincount(p["iidx"], minlength=p["nP"])
    assert tuple(per_cam[:5]) == WIDE_COUNTS == (64, 65, 63, 1, 0) and np.all(per_cam[5:] > 0)
    assert per_pt[-1] == 0 and (per_pt == 0).sum() == 1 and (per_pt == 1).sum() >= 0.1 * p["nP"]
    key = p["iidx"].astype(np.int64) * nC + p["jidx"]
    assert np.all(np.diff(key) > 0)                       # point-major, cameras ascending
    K = np.asarray(p["K"])
    assert np.all(np.abs(K[:, 0] / 800.0 - 1.0) <= 0.02) and np.all(np.abs(K[:, 3] - 1.0) <= 0.01)
    assert np.all(np.abs(K[:, 4]) <= 0.3) and np.all(K[:, 4] != 0.0) and np.all(K[:, 1:3] != 0.0)
    # the boundary the size is for: the finalize kernels run min(ceil(nA^2 / 256), 4096) workgroups of 256
    for cnp, first in ((16, 65), (11, 94)):
        assert ((cnp * (first - 1)) ** 2 <= 4096 * 256) and ((cnp * first) ** 2 > 4096 * 256)


def test_many_obs_problem_is_what_it_claims():
    p = many_obs_problem()
    assert p["nC"] == 65 and p["nO"] > 256 * 256            # the residual kernels' 256 workgroups of 256 stride
    per_cam = np.bincount(p["jidx"], minlength=65)
    assert per_cam.min() > 14 * 64                          # 15 units or more per camera
    assert np.all(np.bincount(p["iidx"], minlength=p["nP"]) == 10)
    assert p["nP"] * 55 / (65 * 66 // 2) > 2 * 64           # products per block: several segments of 64


@needs_ld
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("nC", [64, 65, 93, 94])
def test_twin_sums_against_extended_precision_wide(nC, mask):
    """As test_freekd_twin.py::test_twin_sums_against_extended_precision: within a quarter of the tolerance."""
    p = wide(nC)
    t = TwinKD(p, start_kc(nC), MASKS[mask])
    cost, N, g = t.normal()
    worst = 0.0
    for mu in two_mus(t, N):
        S, ea = t.schur(N, g, mu)
        Sx, eax = t.schur_blocks(mu)
        d = np.sqrt(np.diag(N)[:t.nA] + mu)
        eS = (np.abs(S - Sx.astype(np.float64)) / np.outer(d, d)).max()
        ee = (np.abs(ea - eax.astype(np.float64)) / (d * np.sqrt(cost))).max()
        print(f"wide({nC}) {mask} mu {mu:.3e}: twin S {eS:.2e}, e_a {ee:.2e} (tol {scaled_tol(p):.2e})")
        worst = max(worst, eS, ee)
    assert worst <= 0.25 * scaled_tol(p)


@needs_ld
def test_twin_sums_against_extended_precision_many_obs():
    """many_obs_problem has 20 840 unknowns: the dense twin does not fit, so the fp64 side is the same block route
    (schur_blocks in double) -- all ten intrinsics free, at the damping the GPU test assembles with."""
    p = many_obs_problem()
    rt = fr.Route(p, 16, fr.ALL)
    sm = fr.sums(rt)
    mu = 1e-3 * max(sm["diagU"].max(), sm["diagV"].max())
    S, ea = rt.twin.schur_blocks(mu, dtype=np.float64)
    Sx, eax = rt.twin.schur_blocks(mu)
    d = np.sqrt(sm["diagU"] + mu)
    eS = (np.abs(S - Sx.astype(np.float64)) / np.outer(d, d)).max()
    ee = (np.abs(ea - eax.astype(np.float64)) / (d * np.sqrt(sm["cost"]))).max()
    print(f"many_obs mu {mu:.3e}: twin S {eS:.2e}, e_a {ee:.2e} (tol {scaled_tol(p):.2e})")
    assert max(eS, ee) <= 0.25 * scaled_tol(p)


@needs_ld
def test_closed_form_inverse_loses_the_single_view_points():
    """tiny_problem (points 1 and 2 seen once), the five intrinsics free, mu = 1e-6 median diag N: W times the
    closed-form inverse of V + mu I misses scaled_tol by more than 100x in S and e_a, the L D L^T substitution of the
    same fp64 blocks stays inside it.  At the large damping both are inside."""
    p = tiny_problem()
    rt = fr.Route(p, 11)
    cost, N, g = rt.twin.normal()
    Nr, _ = rt.pick_full(N, g)
    tol = scaled_tol(p)
    for which, mu in zip(("big", "small"), two_mus(rt.twin, N)):
        Sx, eax = rt.pick(*rt.twin.schur_blocks(mu))
        d = np.sqrt(np.diag(Nr)[:rt.nA] + mu)
        out = {}
        for name, solve in (("closed form", fr.closed_form_solve), ("L D L^T", fr.ldl_solve)):
            S, ea, _ = fr.plain_schur(rt, mu, solve)
            out[name] = ((np.abs(S - Sx.astype(np.float64)) / np.outer(d, d)).max(),
                         (np.abs(ea - eax.astype(np.float64)) / (d * np.sqrt(cost))).max())
            print(f"{which} mu {mu:.3e} {name}: S {out[name][0]:.2e}, e_a {out[name][1]:.2e} (tol {tol:.2e})")
        assert max(out["L D L^T"]) <= tol
        if which == "small":
            assert min(out["closed form"]) > 100 * tol
        else:
            assert max(out["closed form"]) <= tol


@functools.lru_cache(maxsize=None)
def plain(name, cnp, which):
    """(route, sums, mu, plain fp64 try) of a named input; shared, never modified"""
    p = tiny_problem() if name == "tiny" else wide(int(name))
    rt = fr.Route(p, cnp, fr.ALL if cnp == 16 else None)
    cost, N, g = rt.twin.normal()
    Nr, gr = rt.pick_full(N, g)
    mu = 1e-3 * rt.twin.max_diag(N) if which == "big" else 1e-6 * float(np.median(np.diag(Nr)))
    return rt, fr.sums(rt), mu, fr.plain_try(rt, mu), Nr, gr


def ratios(rt, sm, mu, dp, newcams, newpts, sc):
    """worst bound ratio of dp_b and of each scalar"""
    r, b = fr.dpb_residual(rt, sm, dp, mu)
    out = {"dp_b": ar.excess(r, np.zeros(r.shape, ar.LD), b)[0]}
    for what, (x, bound) in fr.scalars(rt, sm, dp, newcams, newpts, mu).items():
        out[what] = float(abs(ar.LD(sc[what]) - x) / bound)
    return out


@needs_ld
@pytest.mark.parametrize("which", ["big", "small"])
@pytest.mark.parametrize("name,cnp", [("tiny", 16), ("tiny", 11), ("65", 16), ("94", 11)])
def test_judges_pass_a_plain_evaluation(name, cnp, which):
    rt, sm, mu, tr, _, _ = plain(name, cnp, which)
    out = ratios(rt, sm, mu, tr["dp"], tr["newcams"], tr["newpts"], tr["sc"])
    eta, fe, kappa = fr.solve_judge(tr["S"], tr["ea"], tr["dp"][:rt.nA])
    print(f"{name} / {cnp} {which}: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items())
          + f", eta {eta:.2e}, forward {fe:.2e} (cond {kappa:.1e})")
    assert max(out.values()) <= 0.5
    assert eta <= 0.5 * ETA_MAX and fe <= 0.5 * 2 * kappa * 1e-14
    empty = rt.nA + 3 * (rt.nP - 1)
    if name != "tiny":
        assert np.all(tr["dp"][empty:] == 0.0)              # the point without observations


# ---- Marquardt's damping (psba_set_damping): the judges with a rule ------------------------------------------
MQ_MUS = {"big": 1e-3, "small": 1e-6}       # Marquardt's mu is relative (test_gpu_damping.py)
MQ_CLAMPS = {"default": (fr.DMIN, fr.DMAX), "1e5": (1e-6, 1e5)}
MQ_INPUTS = [("tiny", 16, "all"), ("tiny", 16, "bal"), ("P7", 16, "all"), ("P7", 16, "bal"), ("65", 16, "all"),
             ("65", 16, "bal"), ("94", 11, "k-only")]
MQ_CASES = ([(n, c, m, "default") for n, c, m in MQ_INPUTS]
            + [(n, c, m, "1e5") for n, c, m in MQ_INPUTS if n in ("65", "94")])


@functools.lru_cache(maxsize=None)
def mq_ref(name, cnp, mask):
    """(route, sums) of a named input: shared, never modified"""
    p = tiny_problem() if name == "tiny" else P7() if name == "P7" else wide(int(name))
    rt = fr.Route(p, cnp, MASKS[mask] if cnp == 16 else None)
    return rt, fr.sums(rt)


@functools.lru_cache(maxsize=None)
def mq_plain(name, cnp, mask, which, clamps):
    rt, sm = mq_ref(name, cnp, mask)
    rule = fr.Rule(fr.MARQUARDT, *MQ_CLAMPS[clamps])
    return rule, MQ_MUS[which], fr.plain_try(rt, MQ_MUS[which], rule)


@functools.lru_cache(maxsize=None)
def mq_schur_ref(name, cnp, mask, which, clamps):
    rt, sm = mq_ref(name, cnp, mask)
    return fr.schur_ref(rt, sm, MQ_MUS[which], fr.Rule(fr.MARQUARDT, *MQ_CLAMPS[clamps]))


def c1_ratios(rt, sm, mu, rule, S, ea, S_want, ea_want):
    """C1's scaled measure over the tolerance"""
    d, tol = fr.scale_diag(rt, sm, mu, rule), scaled_tol(rt.p)
    return ((np.abs(S - S_want) / np.outer(d, d)).max() / tol,
            (np.abs(ea - ea_want) / (d * np.sqrt(sm["cost"]))).max() / tol)


def mq_ratios(rt, sm, mu, rule, tr):
    out = {}
    free_diag = np.concatenate([sm["diagUx"], sm["diagVx"]])
    envN = np.concatenate([sm["envdU"], sm["envdV"]])
    out["D"], _, nlow, nhigh = fr.check_damp_diag(tr["D"], free_diag, envN, rule, rt.held)
    r, b = fr.dpb_residual(rt, sm, tr["dp"], mu, rule)
    out["dp_b"] = ar.excess(r, np.zeros(r.shape, ar.LD), b)[0]
    for what, (x, bound) in fr.scalars(rt, sm, tr["dp"], tr["newcams"], tr["newpts"], mu, D=tr["D"]).items():
        out[what] = float(abs(ar.LD(tr["sc"][what]) - x) / bound)
    return out, nlow, nhigh


@needs_ld
@pytest.mark.parametrize("which", ["big", "small"])
@pytest.mark.parametrize("name,cnp,mask,clamps", MQ_CASES)
def test_judges_pass_a_plain_evaluation_under_marquardt(name, cnp, mask, clamps, which):
    """The plain fp64 evaluation stays inside every bound of C1 to C4 and of D; its ratios are the headroom the kernels
    have (DESIGN 7g keeps the table)."""
    rt, sm = mq_ref(name, cnp, mask)
    rule, mu, tr = mq_plain(name, cnp, mask, which, clamps)
    out, nlow, nhigh = mq_ratios(rt, sm, mu, rule, tr)
    out["S"], out["e_a"] = c1_ratios(rt, sm, mu, rule, tr["S"], tr["ea"], *mq_schur_ref(name, cnp, mask, which, clamps))
    fr.check_exact_parts(rt, tr["S"], tr["ea"], mu, rule)
    eta, fe, kappa = fr.solve_judge(tr["S"], tr["ea"], tr["dp"][:rt.nA])
    out["dp_a eta"], out["dp_a forward"] = eta / ETA_MAX, fe / (2 * kappa * 1e-14)
    print(f"{name} / {cnp} {mask} {which} {rule}: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items())
          + f" (cond {kappa:.1e}; {nlow} entries at dmin, {nhigh} at dmax)")
    assert max(out.values()) <= 1.0, out
    if name in ("65", "94"):
        # the clamps are not idle: the camera without observations (its free coordinates) and the unseen point
        D = tr["D"]
        n_free = cnp - (rt.held < cnp).sum()
        assert n_free == {"all": 16, "bal": 9, "k-only": 11}[mask]
        assert (D[:rt.nA] == rule.dmin).sum() >= n_free and (D[rt.nA:] == rule.dmin).sum() >= 3
        assert np.all(tr["dp"][rt.nA + 3 * (rt.nP - 1):] == 0.0) and np.all(tr["dp"][cnp * 4:cnp * 5] == 0.0)
        if clamps == "1e5":
            seen = np.bincount(rt.j, minlength=rt.nC) > 0
            assert np.all((D[:rt.nA].reshape(-1, cnp) == rule.dmax).sum(axis=1)[seen] >= 1)


@needs_ld
def test_injected_marquardt_faults_fail_their_judge():
    """wide_problem(65), all ten intrinsics free, mu = 1e-3, default clamps: (a) to (d); (e) is grouped, below."""
    name, cnp, mask, which = "65", 16, "all", "big"
    rt, sm = mq_ref(name, cnp, mask)
    rule, mu, tr = mq_plain(name, cnp, mask, which, "default")
    S_want, ea_want = mq_schur_ref(name, cnp, mask, which, "default")
    # (a) the back-substitution solves with V + mu I while Y used V + mu D: C3
    bad = fr.plain_try(rt, mu, rule, fault="backsub-identity")
    r, b = fr.dpb_residual(rt, sm, bad["dp"], mu, rule)
    ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), b)
    print(f"(a) dp_b ratio {ratio:.2e} at point {k // 3}")
    assert ratio > 1.0
    assert np.array_equal(bad["S"], tr["S"])                # (nothing else moved)
    # (b) D not clamped below: the empty camera's block and the unseen point get 0 -- C1's exact-block check
    S, ea, pc = fr.plain_schur(rt, mu, rule=rule, fault="no-low-clamp")
    assert np.all(pc["D"][16 * 4:16 * 5] == 0.0) and np.all(pc["D"][-3:] == 0.0)
    with pytest.raises(AssertionError, match="camera 4"):
        fr.check_exact_parts(rt, S, ea, mu, rule)
    # (c) gain_den with mu sum dp^2: C4
    x, bound = fr.scalars(rt, sm, tr["dp"], tr["newcams"], tr["newpts"], mu, D=tr["D"])["gain_den"]
    wrong = float(tr["dp"] @ (mu * tr["dp"] + fr.plain_schur(rt, mu, rule=rule)[2]["g"]))
    print(f"(c) gain_den off by {float(abs(ar.LD(wrong) - x) / bound):.2e} bounds")
    assert abs(ar.LD(wrong) - x) > bound
    # (d) D of camera j read from camera j mod 64 (the second trip of a grid-stride loop): C1, 65 cameras only
    S, ea, pc = fr.plain_schur(rt, mu, rule=rule, fault="cam-mod-64")
    assert np.array_equal(pc["D"][:16 * 64], tr["D"][:16 * 64])
    eS, ee = c1_ratios(rt, sm, mu, rule, S, ea, S_want, ea_want)
    print(f"(d) S {eS:.2e} of the tolerance")
    assert eS > 1.0
    rt64 = fr.Route(wide(64), 16, fr.ALL)                   # ... with 64 cameras the same fault changes nothing
    U0, V0 = np.zeros((64, 16, 16)), np.zeros((rt64.nP, 3, 3))
    assert np.array_equal(fr.plain_damp_diag(rt64, U0, V0, rule, "cam-mod-64"), fr.plain_damp_diag(rt64, U0, V0, rule))


@needs_ld
def test_injected_group_fault_fails_its_judge():
    """(e) wide_problem(65) with shared_ref.wide_labels, BAL mask: D of a representative from its own U_kk instead of
    the members' sum -- C1 on the grouped input; the plain grouped evaluation itself is inside."""
    import shared_ref as sr
    rt = sr.SharedRoute(wide(65), sr.wide_labels(65), BAL)
    sm = fr.sums(rt)
    rule, mu = fr.Rule(fr.MARQUARDT), 1e-3
    S_want, ea_want = sr.schur_ref(rt, sm, mu, rule)
    D_ref = sr.damp_ref(rt, sm, rule)[0]
    fdiag, _ = rt.folded_diag(sm)
    d = np.sqrt(fdiag[:rt.nA] + mu * D_ref[:rt.nA])
    out = {}
    for fault in (None, "rep-own-diag"):
        tr = sr.plain_try_damped(rt, mu, rule, fault)
        eS, ee = sr.scaled_errors(tr["S"], tr["ea"], S_want, ea_want, d, sm["cost"])
        out[fault] = eS / rt.tol
        print(f"grouped, fault {fault}: S {eS / rt.tol:.2e}, e_a {ee / rt.tol:.2e} of the tolerance")
        assert ee <= rt.tol
    assert out[None] <= 1.0 and out["rep-own-diag"] > 1.0


def block_max_rule(rt, dp, dp_want):
    """what tests/test_freek.py and test_gpu_freekd.py hold dp to: 1e-6 of each block's largest entry"""
    nA = rt.nA
    return all(np.abs(dp[sl] - dp_want[sl]).max() <= 1e-6 * np.abs(dp_want[sl]).max()
               for sl in (slice(0, nA), slice(nA, rt.nT)))


@needs_ld
@pytest.mark.parametrize("name,cnp", [("65", 16), ("94", 11)])
def test_injected_faults_fail_their_judge(name, cnp):
    rt, sm, mu, tr, Nr, gr = plain(name, cnp, "big")
    nA = rt.nA
    dp_want = np.linalg.solve(Nr + mu * np.eye(rt.nT), gr)
    assert block_max_rule(rt, tr["dp"], dp_want)
    # 1. one entry of dp_b of the observed point with the smallest step, off by 1e-9 relative
    dpb = tr["dp"][nA:].reshape(-1, 3)
    seen = np.bincount(rt.i, minlength=rt.nP) > 0
    i = int(np.argmin(np.where(seen, np.abs(dpb).max(axis=1), np.inf)))
    c = int(np.argmax(np.abs(dpb[i])))
    bad = tr["dp"].copy()
    bad[nA + 3 * i + c] *= 1.0 + 1e-9
    r, b = fr.dpb_residual(rt, sm, bad, mu)
    ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), b)
    print(f"dp_b fault at point {i}: ratio {ratio:.2e} at entry {k}")
    assert ratio > 1.0 and k // 3 == i
    assert block_max_rule(rt, bad, dp_want)
    # 2. one k5 entry of dp_a (16 wide; the skew s on the 11-block route, its smallest intrinsic column), 1e-9 relative
    col = 9 if cnp == 16 else 4
    j = int(np.argmax(np.abs(tr["dp"][:nA].reshape(-1, cnp)[:, col])))
    bad = tr["dp"].copy()
    bad[cnp * j + col] *= 1.0 + 1e-9
    eta, fe, kappa = fr.solve_judge(tr["S"], tr["ea"], bad[:nA])
    print(f"dp_a fault at camera {j} column {col}: eta {eta:.2e}, forward {fe:.2e} (bound {2 * kappa * 1e-14:.2e})")
    assert eta > ETA_MAX
    assert block_max_rule(rt, bad, dp_want)
    # 3. dp_l2 without the point part
    want = fr.scalars(rt, sm, tr["dp"], tr["newcams"], tr["newpts"], mu)["dp_l2"]
    short = float(tr["dp"][:nA] @ tr["dp"][:nA])
    assert abs(ar.LD(short) - want[0]) > want[1]
