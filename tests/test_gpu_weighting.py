"""psba_set_obs_weighting on the GPU: a robust loss and per-observation sigmas on the free-intrinsics routes
(PSBA_CAMERA_FREE_K, blocks of 11, and PSBA_CAMERA_FREE_KD, blocks of 16).  The reference and its judges are
tests/weight_ref.py (on prior_ref.py, held_ref.py and free_ref.py, their constants, scaled_tol and ETA_MAX unchanged; no
constant is fitted to a GPU result).  Needs an MI355X.  The inputs, holds, priors, dampings and mus are those of
test_gpu_priors.py; the weighting is weight_ref.draw_weighting: sigma log-uniform in [0.5, 2], c the root of the median
of s, so that both branches of Huber occur on every input.

  1  one damping try entry by entry (C1 to C4) for Huber, Cauchy, soft-L1 and no loss, all with sigmas, under both
     dampings and both mus, with psba_get_gradient, psba_max_diag, psba_get_damping_diag, psba_residual,
     psba_prior_cost and psba_get_obs_weights at both parameter sets, and the exact parts of the holds.
  2  psba_get_free_obs_blocks: W and B | e entry by entry against the weighted blocks.
  3  psba_linearize(2, -2): g = -2 g_1 entry by entry; the held diagonals are exactly 2 + mu.
  4  no weighting is no weighting: (PSBA_LOSS_NONE, 5, NULL), and a weighting set and cleared, against a handle that
     never called the verb.
  5  two weighted runs are bit-identical.
  6  the look-ahead linearization takes its weights at the proposal; a rejected step leaves the current one untouched.
  7  composition with the mask, the groups, Marquardt's damping, holds and priors, in two orders of calls.
  8  psba_levmar on the contaminated ring scene against the dense twin; a plain handle on the same data.
  9  the interface.
The module prints the worst ratio (found / allowed) per route, input and quantity; DESIGN 7k keeps the table."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import held_ref as hr
import prior_ref as pr
import shared_ref as sr
import weight_ref as wr
from freekd_twin import BAL, ring_problem, start_kc
from test_freekd_twin import scaled_tol
from test_gpu_dense_solve import ETA_MAX
from test_gpu_priors import MQ_MUS, ROUTES, RULES, check_padding, full_try, holds, plain_handle, prob, read_system, try_and_log

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

KINDS = {"none": wr.NONE, "huber": wr.HUBER, "cauchy": wr.CAUCHY, "soft-l1": wr.SOFT_L1}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        keys = sorted({(r, n) for r, n, _ in WORST})
        lines = [f"  {r} {n}: " + ", ".join(f"{q} {v:.2e}" for (rr, nn, q), v in WORST.items() if (rr, nn) == (r, n))
                 for r, n in keys]
        print("\nweighting: worst ratio found / allowed per route, input and quantity:\n" + "\n".join(lines))


def note(route, name, what, ratio):
    WORST[(route, name, what)] = max(WORST.get((route, name, what), 0.0), float(ratio))
    print(f"{route} {name} {what}: {float(ratio):.3e}")


def assert_judged(route, label, out):
    for what, ratio in out.items():
        note(route, label, what, ratio)
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, f"{route} {label}: found / allowed above 1: {bad}"


@functools.lru_cache(maxsize=None)
def ref(name, route, kind):
    """(WeightRoute, its extended-precision sums) of one input: computed once, shared, never modified"""
    cnp, free = ROUTES[route]
    p = prob(name, cnp)
    poses, pts = holds(name, route)
    rt0 = hr.HeldRoute(p, cnp, free, poses, pts)
    sigma, c = wr.draw_weighting(rt0, KINDS[kind])
    rt = wr.WeightRoute(p, cnp, pr.draw_priors(rt0), (KINDS[kind], c), sigma, free, poses, pts)
    return rt, wr.sums(rt)


def weigh(h, rt):
    h.set_obs_weighting(rt.kind, rt.c, rt.sigma if rt.has_sigma else None)
    assert h.obs_weighting() == (rt.kind, rt.c, rt.has_sigma)


def handle(rt, rule=fr.NO_RULE):
    h = plain_handle(rt.p, rt.cnp, rt.free, rule)
    h.set_held(rt.held_poses, rt.held_pts)
    h.set_priors(**rt.pri.args())
    weigh(h, rt)
    return h


def device_try(h, rt, mu, rule, coeff=1.0, coeff_g=1.0):
    """one damping try on the device with everything weight_ref.judge reads"""
    got = {}
    got["cost"] = h.residual()
    got["prior_cur"] = h.prior_cost()
    got["w_cur"] = h.get_obs_weights(0)
    h.linearize(coeff, coeff_g)
    got["max_diag"] = h.max_diag()
    got["g"] = h.get_gradient() if rt.cnp == 16 else None
    got["D"] = h.get_damping_diag() if rule.marquardt else None
    h.schur_assemble(mu)
    got["S"], got["ea"], M = read_system(h, rt.nA)
    check_padding(M, rt.nA)
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    got["sc"] = dict(dp_l2=sc.dp_l2, gain_den=sc.gain_den, newp_l2=sc.newp_l2, new_cost=sc.new_cost)
    got["dp"] = h.get_dp()
    got["cams"], got["pts"] = h.get_params(0)
    got["newcams"], got["newpts"] = h.get_params(1)
    got["cost_new"] = h.residual(1)
    got["prior_new"] = h.prior_cost(1)
    got["w_new"] = h.get_obs_weights(1)
    return got


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ["tiny", "P7", "wide"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_one_damping_try_entrywise(route, name, kind, rule, which_mu):
    """case 1"""
    rt, sm = ref(name, route, kind)
    rule = RULES[rule]
    mus, _ = hr.dampings(rt, sm)
    mu = (MQ_MUS if rule.marquardt else mus)[which_mu]
    h = handle(rt, rule)
    try:
        got = device_try(h, rt, mu, rule)
    finally:
        h.close()
    assert got["prior_cur"][0] > 0.0 and got["prior_cur"][1] > 0.0
    out = wr.judge(rt, sm, mu, rule, got, scaled_tol(rt.p), ETA_MAX)
    assert {"S", "e_a", "dp_b", "new_cost", "residual cost", "residual cost_new", "w_cur s", "w_new w"} <= set(out)
    assert_judged(route, f"{name} {kind}", out)


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
@pytest.mark.parametrize("name", ["tiny", "P7", "wide"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_the_weighted_observation_blocks(route, name, kind):
    """case 2: psba_get_free_obs_blocks returns the weighted W and B | e; the holds' zeros stay exact"""
    rt, sm = ref(name, route, kind)
    h = handle(rt)
    try:
        h.linearize(1.0, 1.0)
        W, B, e = h.free_obs_blocks()
    finally:
        h.close()
    hp, hq = rt.held_poses[rt.j], rt.held_pts[rt.i]
    assert np.all(W[hp][:, rt.ni:, :] == 0.0) and np.all(W[hq] == 0.0) and np.all(B[hq] == 0.0)
    assert_judged(route, f"{name} {kind} blocks", wr.blocks_judge(rt, sm, W, B, e))


@pytest.mark.parametrize("route", list(ROUTES))
def test_linearize_with_coefficients(route):
    """case 3: psba_linearize(2, -2) on 7camsvarK under Huber: S(mu) = 2 S_1(mu / 2), e_a(mu) = -2 e_a,1(mu / 2),
    g = -2 g_1 entry by entry (the weights do not depend on the coefficients); the held diagonals are exactly 2 + mu."""
    rt, sm = ref("P7", route, "huber")
    nA = rt.nA
    mus, _ = hr.dampings(rt, sm)
    mu, cost = 2.0 * mus["big"], sm["cost"]
    h = handle(rt)
    try:
        h.linearize(2.0, -2.0)
        want_md = 2.0 * float(np.concatenate([sm["diagU"], sm["diagV"]])[rt.free_all].max())
        assert abs(h.max_diag() - want_md) <= 1e-11 * want_md
        if rt.cnp == 16:
            ratio, k = ar.excess(h.get_gradient() / -2.0, sm["g"], sm["envg"])
            note(route, "P7 (2, -2)", "g", ratio)
            assert ratio <= 1.0, f"g[{k}]"
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        S_want, ea_want = pr.schur_ref(rt, sm, mu / 2.0)
        eS, ee = sr.scaled_errors(S / 2.0, ea / -2.0, S_want, ea_want, pr.scale_diag(rt, sm, mu / 2.0), cost)
        tol = scaled_tol(rt.p)
        note(route, "P7 (2, -2)", "S", eS / tol)
        note(route, "P7 (2, -2)", "e_a", ee / tol)
        assert eS <= tol and ee <= tol
        check_padding(M, nA)
        hr.check_held_system(rt, S, ea, mu, coeff=2.0)
        assert np.all(S[rt.held, rt.held] == 2.0 + mu)
        h.schur_reduce()
        h.schur_solve()
        assert h.backsub(mu).status == 0
        assert np.all(h.get_dp()[rt.held_all] == 0.0)
    finally:
        h.close()


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("route", ["kd-bal", "fk"])
def test_no_weighting_is_no_weighting(route, rule):
    """case 4: (PSBA_LOSS_NONE, 5.0, NULL), and a weighting set, run and then cleared, are bit for bit the handle that
    never called the verb: the reduce buffer (S, e_a), dp and the four scalars of one try, the maximum of the diagonal
    and the whole log of a 5-iteration psba_levmar."""
    cnp, free = ROUTES[route]
    rt, _ = ref("P7", route, "cauchy")
    rule = RULES[rule]
    runs = {}
    for which in ("never", "none", "cleared"):
        h = plain_handle(rt.p, cnp, free, rule)
        try:
            if which == "none":
                h.set_obs_weighting(wr.NONE, 5.0, None)
                assert h.obs_weighting() == (wr.NONE, 5.0, False)
            elif which == "cleared":
                weigh(h, rt)
                h.linearize(1.0, 1.0)
                full_try(h, 1e-3 if rule.marquardt else 1e-3 * h.max_diag())
                h.levmar(max_iter=2, tr_handoff=False, log_cap=64)
                h.reset_params()
                h.set_obs_weighting(wr.NONE, 1.0, None)
            s, w = h.get_obs_weights()
            assert np.all(w == 1.0) and abs(s.sum() - h.residual()) <= 1e-12 * s.sum()
            runs[which] = try_and_log(h, 1e-3)
        finally:
            h.close()
    assert len(runs["never"][4]) > 0
    for which in ("none", "cleared"):
        for k, what in enumerate(("reduce buffer", "dp", "scalars", "max diag", "LM log")):
            assert runs[which][k] == runs["never"][k], f"{which}: {what}"


def test_two_weighted_runs_are_bit_identical():
    """case 5: wide_problem(65), {f, k1, k2}, holds, priors, Cauchy with sigmas, Marquardt: the reduce buffer, dp, the
    scalars, D, the costs, the weights and the log of psba_levmar -- no floating-point atomics."""
    rt, _ = ref("wide", "kd-bal", "cauchy")
    rule = RULES["marquardt"]
    out = []
    for _ in range(2):
        h = handle(rt, rule)
        try:
            cost = h.residual()
            h.linearize(1.0, 1.0)
            D = h.get_damping_diag().tobytes()
            one = full_try(h, MQ_MUS["big"]) + (D, cost, h.residual(1), h.get_gradient().tobytes(),
                                               h.get_obs_weights(1)[1].tobytes())
            h.reset_params()
            _, log = h.levmar(max_iter=5, tr_handoff=False, log_cap=256)
            out.append(one + (log.tobytes(),))
        finally:
            h.close()
    assert out[0] == out[1] and len(out[0][-1]) > 0


def test_the_look_ahead_takes_its_weights_at_the_proposal():
    """case 6: psba_backsub_async, psba_linearize_ahead, psba_backsub_wait, psba_accept: the linearization then current
    is bit for bit a fresh psba_linearize at the accepted parameters (W, B | e, the gradient, D and, through the next
    try, U, g and PV in the reduce buffer, dp and the scalars).  A rejected step leaves the current W, Be, U, g
    untouched."""
    rt, _ = ref("wide", "kd-bal", "cauchy")
    rule, mu = RULES["marquardt"], MQ_MUS["big"]
    h, h2 = handle(rt, rule), None
    try:
        cost, _ = h.begin()
        h.linearize(1.0, 1.0)
        D0, g0 = h.get_damping_diag(), h.get_gradient()
        w0 = h.get_obs_weights(0)[1]
        first = full_try(h, mu)
        # a rejected step: the look-ahead is queued and dropped, the same try again gives the same bits
        h.schur_assemble(mu)
        h.schur_reduce()
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        sc = h.backsub_wait()
        assert sc.status == 0 and (sc.dp_l2, sc.gain_den, sc.newp_l2, sc.new_cost) == first[2]
        assert h.get_gradient().tobytes() == g0.tobytes() and h.get_damping_diag().tobytes() == D0.tobytes()
        assert full_try(h, mu) == first
        # an accepted step
        h.schur_assemble(mu)
        h.schur_reduce()
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        sc = h.backsub_wait()
        assert sc.status == 0 and sc.new_cost < cost
        cams, pts = h.get_params(1)
        w_new = h.get_obs_weights(1)[1]
        h.accept()
        D1 = h.get_damping_diag()
        h.linearize(1.0, 1.0)                               # (nothing left to do: the linearization came with the accept)
        blocks1 = h.free_obs_blocks()
        g1 = h.get_gradient()
        assert g1.tobytes() != g0.tobytes() and h.get_damping_diag().tobytes() == D1.tobytes()
        assert abs(h.residual() - sc.new_cost) <= 1e-12 * sc.new_cost
        assert h.get_obs_weights(0)[1].tobytes() == w_new.tobytes() and w_new.tobytes() != w0.tobytes()
        got = full_try(h, mu)
        h2 = handle(rt, rule)
        h2.set_params(cams, pts)
        h2.linearize(1.0, 1.0)
        assert h2.get_damping_diag().tobytes() == D1.tobytes() and h2.get_gradient().tobytes() == g1.tobytes()
        for a, b, what in zip(blocks1, h2.free_obs_blocks(), ("W", "B", "e")):
            assert a.tobytes() == b.tobytes(), what
        assert full_try(h2, mu) == got
    finally:
        h.close()
        if h2 is not None:
            h2.close()


@functools.lru_cache(maxsize=None)
def shared_ref_ring():
    """the shared ring of test_gpu_priors.py (two groups of three cameras, {f, k1, k2}, poses 0 and 1 held, drawn priors)
    with Cauchy and drawn sigmas"""
    labels = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    start, kc0, _, _ = sr.shared_ring(labels)
    poses = hr.flags(6, [0, 1])
    rt0 = hr.HeldSharedRoute(start, labels, BAL, kc0, poses)
    sigma, c = wr.draw_weighting(rt0, wr.CAUCHY)
    rt = wr.WeightSharedRoute(start, labels, pr.draw_priors(rt0), (wr.CAUCHY, c), sigma, BAL, kc0, poses)
    return rt, wr.sums(rt)


def shared_handle(rt, rule, order):
    import psba_amd
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(rt.p)
    h.set_distortion(rt.kc)
    calls = {"mask": lambda: h.set_intrinsics_mask(rt.free), "groups": lambda: h.set_intrinsics_groups(rt.labels),
             "damping": lambda: h.set_damping(rule.kind, rule.dmin, rule.dmax),
             "holds": lambda: h.set_held(rt.held_poses, rt.held_pts), "priors": lambda: h.set_priors(**rt.pri.args()),
             "weights": lambda: weigh(h, rt)}
    for c in order:
        calls[c]()
    return h


def test_composition_with_mask_groups_damping_holds_and_priors():
    """case 7: both orders of calls give the same bytes; the result passes the entrywise judge of case 1 against
    WeightSharedRoute within shared_tol; the exact parts of the holds and the groups."""
    rt, sm = shared_ref_ring()
    rule, mu = RULES["marquardt"], MQ_MUS["big"]
    bufs = []
    for order in (("mask", "groups", "damping", "holds", "priors", "weights"),
                  ("weights", "priors", "holds", "groups", "mask", "damping")):
        h = shared_handle(rt, rule, order)
        try:
            assert h.held_counts() == (2, 0) and h.intrinsics_groups()[1] == 2 and h.prior_counts() == rt.pri.counts()
            assert h.obs_weighting() == (rt.kind, rt.c, True)
            got = device_try(h, rt, mu, rule)
            if not bufs:
                assert_judged("kd-bal", "shared ring", wr.judge(rt, sm, mu, rule, got, rt.tol, ETA_MAX))
            h.accept()
            acc, _ = h.get_params(0)
            assert acc.tobytes() == got["newcams"].tobytes()
            assert np.array_equal(acc[:, :10], acc[rt.rep][:, :10]) and acc[:2, 10:].tobytes() == got["cams"][:2, 10:].tobytes()
            bufs.append((got["S"].tobytes(), got["ea"].tobytes(), got["dp"].tobytes(), got["D"].tobytes(), got["g"].tobytes(),
                         tuple(got["sc"].values()), got["cost"], got["cost_new"], got["prior_cur"], got["prior_new"],
                         got["w_cur"][0].tobytes(), got["w_cur"][1].tobytes(), got["w_new"][1].tobytes()))
        finally:
            h.close()
    assert bufs[0] == bufs[1], "the order of the calls changes the bits"


LM_ITERS = 30


@functools.lru_cache(maxsize=None)
def ring_twin_lm(kind):
    start, kc0, poses, bad = wr.contaminated_ring()
    t = wr.WeightTwin(start, (kind, 2.0), None, kc0, BAL, poses)
    res, log = t.levmar(max_iter=LM_ITERS)
    return start, kc0, poses, bad, res, log, t.cams.copy()


def test_levmar_on_the_contaminated_ring():
    """case 8: the ring scene with 45 of 571 observations moved by 20 to 50 px, {f, k1, k2} free, poses 0 and 1 held,
    Cauchy c = 2, against the dense twin's log by the rules of test_gpu_priors.py's LM case; the focal lengths end at
    most twice as far from the truth as the twin's; s > 9 c^2 at the end flags exactly the moved observations; a plain
    handle on the same data ends at least 20 times farther from the true focal lengths."""
    start, kc0, poses, bad, want, wlog, tcams = ring_twin_lm(wr.CAUCHY)
    _, _, K, _ = ring_problem()
    far = {}
    for kind in (wr.CAUCHY, wr.NONE):
        h = plain_handle(start, 16, BAL, kc=kc0)
        try:
            h.set_held(poses, None)
            if kind != wr.NONE:
                h.set_obs_weighting(kind, 2.0)
            res, log = h.levmar(max_iter=LM_ITERS, tr_handoff=False, log_cap=512)
            c1, _ = h.get_params(0)
            far[kind] = float(np.abs(c1[:, 0] - K[:, 0]).max())
            if kind == wr.CAUCHY:
                assert abs(res.init_err - want.init_err) <= 1e-12 * want.init_err
                n = min(len(log), len(wlog), 6)
                assert n >= 4 and np.array_equal(log[:n, 4], wlog[:n, 4])
                np.testing.assert_allclose(log[:n, 1], wlog[:n, 1], rtol=1e-6)
                rel = abs(res.final_err - want.final_err) / want.final_err
                note("kd-bal", "contaminated ring", "LM final cost", rel / 1e-5)
                assert rel <= 1e-5, f"final cost {res.final_err!r}, the twin's {want.final_err!r}"
                assert abs(h.residual() - res.final_err) <= 1e-12 * res.final_err
                s, w = h.get_obs_weights()
                assert np.array_equal(np.flatnonzero(s > 9.0 * 2.0 ** 2), bad)
                assert np.all(w[bad] < 0.32) and np.all(w <= 1.0)
        finally:
            h.close()
    twin_far = float(np.abs(tcams[:, 0] - K[:, 0]).max())
    note("kd-bal", "contaminated ring", "max |fu - true| over twice the twin's", far[wr.CAUCHY] / (2.0 * twin_far))
    assert far[wr.CAUCHY] <= 2.0 * twin_far, (far, twin_far)
    assert far[wr.NONE] >= 20.0 * far[wr.CAUCHY], far


def test_interface():
    """case 9"""
    import psba_amd
    from psba_amd import capi
    rt, _ = ref("P7", "kd-bal", "cauchy")
    p, nC, nO = rt.p, rt.nC, rt.nO
    h = psba_amd.Psba(0)

    def refused(call, code, *words):
        with pytest.raises(psba_amd.PsbaError) as ei:
            call()
        assert ei.value.code == code, str(ei.value)
        for w in words:
            assert w in str(ei.value), str(ei.value)
    try:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        refused(lambda: h.set_obs_weighting(wr.CAUCHY, 2.0), -6, "no problem uploaded")     # before an upload
        refused(h.obs_weighting, -6)
        h.upload_problem(p)
        h.set_distortion(start_kc(nC))
        h.set_intrinsics_mask(BAL)
        assert h.obs_weighting() == (wr.NONE, 1.0, False)
        s0, w0 = h.get_obs_weights()                          # no weighting: s = |e|^2, w = 1
        assert np.all(w0 == 1.0) and abs(s0.sum() - h.residual()) <= 1e-12 * s0.sum()
        weigh(h, rt)
        h.set_obs_weighting(wr.HUBER, 3.0)
        assert h.obs_weighting() == (wr.HUBER, 3.0, False)
        h.set_obs_weighting(wr.NONE, 1.0, rt.sigma)
        assert h.obs_weighting() == (wr.NONE, 1.0, True)
        s1, w1 = h.get_obs_weights()
        # (s1: the scaling, the squares, the add, three roundings on a path; s0 w w: the squares, the add, two products, four)
        assert np.array_equal(w1, 1.0 / rt.sigma) and np.all(np.abs(s1 - s0 * w1 * w1) <= ar.gamma(8) * s1)
        assert abs(s1.sum() - h.residual()) <= 1e-12 * s1.sum()
        weigh(h, rt)
        before = h.obs_weighting()
        cost = h.residual()
        # an unknown kind, a bad scale (for every kind) and a bad sigma, naming the observation; a refused call changes nothing
        refused(lambda: h.set_obs_weighting(4, 1.0), -1, "unknown loss kind 4")
        refused(lambda: h.set_obs_weighting(-1, 1.0), -1, "unknown loss kind")
        for kind in (wr.NONE, wr.HUBER, wr.CAUCHY, wr.SOFT_L1):
            for scale in (0.0, -1.0, np.inf, np.nan):
                refused(lambda: h.set_obs_weighting(kind, scale, rt.sigma), -1, "scale must be finite and > 0")
        for a, v in ((7, 0.0), (nO - 2, -2.0), (3, np.nan), (0, np.inf)):
            bad = rt.sigma.copy()
            bad[a], bad[nO - 1] = v, -1.0                    # (two offenders: the first is named)
            refused(lambda: h.set_obs_weighting(wr.CAUCHY, 2.0, bad), -1, f"observation {a} ", "finite and > 0")
        assert h.obs_weighting() == before and h.residual() == cost
        refused(lambda: h.get_obs_weights(7), -1)
        refused(lambda: h.get_obs_weights(1), -6, "no proposal")                           # before any proposal
        # the fixed-K verbs keep refusing these models
        refused(lambda: h.set_robust_loss(wr.HUBER, 1.0), -6)
        refused(lambda: h.set_obs_covariance(np.tile(np.eye(2).reshape(-1), nO)), -6)
        refused(h.obs_sq_residuals, -6)
        # setting the weighting discards a queued linearization and invalidates the two test hooks
        h.set_damping(psba_amd.DAMPING_MARQUARDT)
        h.linearize(1.0, 1.0)
        h.free_obs_blocks()
        h.get_damping_diag()
        weigh(h, rt)
        for call in (h.free_obs_blocks, h.get_damping_diag, lambda: h.schur_assemble(1e-3)):
            refused(call, -6)
        h.linearize(1.0, 1.0)
        mu = 1e-3
        h.schur_assemble(mu)
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        refused(lambda: h.set_obs_weighting(wr.NONE, 1.0), -6, "in flight")   # a try is in flight: refused, nothing changes
        refused(h.get_obs_weights, -6, "in flight")
        assert h.obs_weighting() == before
        assert h.backsub_wait().status == 0
        assert h.get_obs_weights(1)[0].shape == (nO,)
        h.set_obs_weighting(wr.HUBER, rt.c, rt.sigma)        # ... discards the linearization queued ahead
        h.accept()
        for call in (h.free_obs_blocks, h.get_damping_diag, lambda: h.schur_assemble(mu)):
            refused(call, -6)
        assert capi.lib.psba_obs_weighting(h._h, None, None, None) == 0
        assert capi.lib.psba_get_obs_weights(h._h, 0, None, None) == 0
        # a new upload resets to (none, 1, no sigmas)
        h.upload_problem(p)
        assert h.obs_weighting() == (wr.NONE, 1.0, False)
    finally:
        h.close()
    # blocks of 11 take the verb; six-parameter blocks refuse it and name the fixed-K verbs
    for model, ok in ((psba_amd.CAMERA_FREE_K, True), (psba_amd.CAMERA_FIXED_K, False)):
        ho = psba_amd.Psba(0)
        try:
            ho.set_camera_model(model)
            ho.upload_problem(p)
            if ok:
                weigh(ho, rt)
            else:
                refused(lambda: ho.set_obs_weighting(wr.CAUCHY, 2.0), -6, "psba_set_robust_loss", "psba_set_obs_covariance")
                refused(ho.obs_weighting, -6, "free-intrinsics models only")
                refused(ho.get_obs_weights, -6, "free-intrinsics models only")
                ho.set_robust_loss(wr.HUBER, 1.0)             # (the fixed-K verb is the one that works there)
        finally:
            ho.close()
