"""psba_set_held on the GPU: held poses and points on the free-intrinsics routes (PSBA_CAMERA_FREE_K, blocks of 11, and
PSBA_CAMERA_FREE_KD, blocks of 16).  The reference and its judges are tests/held_ref.py (on free_ref.py's
constants, scaled_tol and ETA_MAX unchanged; no constant is fitted to a GPU result).  Needs an MI355X.

  1  one damping try entry by entry (C1 to C4 of test_gpu_free_entrywise.py) under both dampings and both mus, on
     tiny_problem (pose 1, point 1), 7camsvarK (poses 0, 1 and the camera with the largest pose diagonal; a point with
     three views) and wide_problem(65 / 94) (cameras 0, 1, 3, 4 and the last; point 0, the last point, one with three
     views), with the exact parts: g, e_a, dp 0.0 at held entries, held rows and columns of S, the proposal's bits,
     the zero W and B of psba_get_free_obs_blocks, the mirror and the padding.
  2  psba_linearize(2, -2): the held diagonals are exactly 2 + mu.
  3  Gauss-Newton: psba_schur_assemble(0.0) with poses 0 and 1 held is solvable and equals the twin's reduced solve.
  4  against the fixed-K route with psba_set_fixed of the same blocks.
  5  no mask is no mask: all-zero masks, and masks set and cleared, against a handle that never called the verb.
  6  two runs with holds are bit-identical.
  7  the look-ahead linearization with holds.
  8  composition with the mask, the groups and Marquardt's damping, in two orders of calls.
  9  psba_levmar against the dense LM with the held columns deleted on the ring scene.
  10 the interface.
The module prints the worst ratio (found / allowed) per route, input, rule and quantity; DESIGN 7i keeps the table."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import held_ref as hr
import shared_ref as sr
from freekd_twin import BAL, CNP, start_kc, tiny_problem, wide_problem
from test_freekd_twin import P7, scaled_tol
from test_gpu_dense_solve import ETA_MAX

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

ROUTES = {"kd-all": (16, fr.ALL), "kd-bal": (16, BAL), "fk": (11, None)}
NONE = (0,) * 10
WIDE = {16: 65, 11: 94}
RULES = {"identity": fr.NO_RULE, "marquardt": fr.Rule(fr.MARQUARDT)}
MQ_MUS = {"big": 1e-3, "small": 1e-6}   # Marquardt's mu is relative (test_gpu_damping.py)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        keys = sorted({(r, n) for r, n, _ in WORST})
        lines = [f"  {r} {n}: " + ", ".join(f"{q} {v:.2e}" for (rr, nn, q), v in WORST.items() if (rr, nn) == (r, n))
                 for r, n in keys]
        print("\nheld blocks: worst ratio found / allowed per route, input and quantity:\n" + "\n".join(lines))


def note(route, name, what, ratio):
    WORST[(route, name, what)] = max(WORST.get((route, name, what), 0.0), float(ratio))
    print(f"{route} {name} {what}: {float(ratio):.3e}")


@functools.lru_cache(maxsize=None)
def prob(name, cnp=16):
    if name == "wide":
        return wide_problem(WIDE[cnp])
    return {"tiny": tiny_problem, "P7": P7}[name]()


@functools.lru_cache(maxsize=None)
def holds(name, route):
    """(pose flags [nC], point flags [nP]) of the module docstring"""
    cnp, free = ROUTES[route]
    p = prob(name, cnp)
    nC, nP = int(p["nC"]), int(p["nP"])
    if name == "tiny":
        poses, pts = [1], [1]
    elif name == "P7":
        big, is_max = hr.largest_pose_camera(p, cnp, free)
        assert is_max                                       # a max_diag that forgets the mask reports this entry
        poses, pts = sorted({0, 1, big}), [hr.point_with_views(p)]
    else:
        poses, pts = [0, 1, 3, 4, nC - 1], [0, nP - 1, hr.point_with_views(p)]
        assert np.bincount(p["iidx"], minlength=nP)[[0, nP - 1]].tolist() == [1, 0]
    return hr.flags(nC, poses), hr.flags(nP, pts)


@functools.lru_cache(maxsize=None)
def ref(name, route, two_poses=False):
    """(HeldRoute, its extended-precision sums) of one input: computed once, shared, never modified.  two_poses: poses
    0 and 1 alone"""
    cnp, free = ROUTES[route]
    p = prob(name, cnp)
    poses, pts = (hr.flags(p["nC"], [0, 1]), None) if two_poses else holds(name, route)
    rt = hr.HeldRoute(p, cnp, free, poses, pts)
    return rt, hr.sums(rt)


@functools.lru_cache(maxsize=None)
def schur_ref(name, route, mu, rule=fr.NO_RULE, two_poses=False):
    rt, sm = ref(name, route, two_poses)
    S, ea = hr.schur_ref(rt, sm, mu, rule)
    S.setflags(write=False)
    ea.setflags(write=False)
    return S, ea


def plain_handle(p, cnp, free, rule=fr.NO_RULE, kc="start"):
    import psba_amd
    h = psba_amd.Psba(0)
    if cnp == 16:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        h.upload_problem(p)
        h.set_distortion(start_kc(p["nC"]) if isinstance(kc, str) else kc)
        h.set_intrinsics_mask(free)
    else:
        h.set_camera_model(psba_amd.CAMERA_FREE_K)
        h.upload_problem(p)
    assert h.camera_block() == cnp and h.schur_path() == 5
    if rule.marquardt:
        h.set_damping(rule.kind, rule.dmin, rule.dmax)
    return h


def handle(rt, rule=fr.NO_RULE):
    h = plain_handle(rt.p, rt.cnp, rt.free, rule)
    h.set_held(rt.held_poses, rt.held_pts)
    assert h.held_counts() == (int(rt.held_poses.sum()), int(rt.held_pts.sum()))
    return h


def read_system(h, nA):
    n32 = (nA + 31) // 32 * 32
    M = h.get_reduce_buffer().reshape(n32 + 1, n32)
    return M[:nA, :nA].copy(), M[n32, :nA].copy(), M


def check_padding(M, nA):
    n32 = M.shape[1]
    pad = np.zeros((n32 - nA, n32))
    pad[np.arange(n32 - nA), nA + np.arange(n32 - nA)] = 1.0
    assert np.array_equal(M[nA:n32], pad) and np.all(M[:nA, nA:] == 0.0) and np.all(M[n32, nA:] == 0.0)


def check_S_ea(route, label, rt, S, ea, S_want, ea_want, d, cost):
    """C1's scaled measure over the whole square; the blocks above the diagonal are copies of those below"""
    tol = scaled_tol(rt.p)
    eS = (np.abs(S - S_want) / np.outer(d, d)).max()
    ee = (np.abs(ea - ea_want) / (d * np.sqrt(cost))).max()
    note(route, label, "S", eS / tol)
    note(route, label, "e_a", ee / tol)
    assert eS <= tol and ee <= tol, f"{route} {label}: scaled S {eS:.3e}, e_a {ee:.3e}, tol {tol:.3e}"
    blk = np.arange(S.shape[0]) // rt.cnp
    upper = blk[:, None] < blk[None, :]
    assert np.array_equal(S[upper], S.T[upper])


def check_obs_blocks(h, rt):
    """psba_get_free_obs_blocks: zero W rows for held pose coordinates, a whole zero W and zero B for a held point
    while its e is non-zero"""
    W, B, e = h.free_obs_blocks()
    hp, hq = rt.held_poses[rt.j], rt.held_pts[rt.i]
    assert np.all(W[hp][:, rt.ni:, :] == 0.0) and np.all(W[hq] == 0.0) and np.all(B[hq] == 0.0)
    assert np.all(np.abs(e[hq]).sum(axis=1) > 0.0) and np.all(np.abs(e[hp]).sum(axis=1) > 0.0)
    free = ~hp & ~hq
    assert np.all(np.abs(W[free][:, rt.ni:, :]).sum(axis=(1, 2)) > 0.0) and np.all(np.abs(B[~hq]).sum(axis=(1, 2)) > 0.0)
    if hp.any() and (hp & ~hq).any():                       # the intrinsics of a held pose stay in W
        assert np.all(np.abs(W[hp & ~hq][:, 0, :]).sum(axis=1) > 0.0)


def one_try(route, name, which_mu, rule):
    rt, sm = ref(name, route)
    cnp, nA, nC = rt.cnp, rt.nA, rt.nC
    mus, diag = hr.dampings(rt, sm)
    mu, cost = (MQ_MUS if rule.marquardt else mus)[which_mu], sm["cost"]
    tol = scaled_tol(rt.p)
    label = f"{name} {rule}"
    h = handle(rt, rule)
    D = None
    try:
        if name == "wide":                                   # the local rotations of this scene are 0.0: those of held
            cams, pts = h.get_params(0)                      # camera 0 become -0.0, which a proposal formed as
            assert np.all(cams[0, rt.ni:rt.ni + 3] == 0.0)   # p + 0.0 would turn into +0.0 (the problem is the same)
            cams[0, rt.ni:rt.ni + 3] = -0.0
            h.set_params(cams, pts)
            assert h.held_counts() == (int(rt.held_poses.sum()), int(rt.held_pts.sum()))
        assert abs(h.residual() - cost) <= 1e-12 * cost      # the cost is untouched: every observation counts
        h.linearize(1.0, 1.0)
        hr.check_max_diag(rt, sm, h.max_diag())
        check_obs_blocks(h, rt)
        gg = None
        if cnp == 16:
            gg = h.get_gradient()
            dg, allowed = np.abs(gg - sm["g"].astype(np.float64)), tol * np.sqrt(diag) * np.sqrt(cost)
            note(route, label, "g", (dg[allowed > 0] / allowed[allowed > 0]).max())
            assert np.all(dg <= allowed)
        if rule.marquardt:
            D = h.get_damping_diag()
            ratio, k, _, _ = fr.check_damp_diag(D, np.concatenate([sm["diagUx"], sm["diagVx"]]),
                                                np.concatenate([sm["envdU"], sm["envdV"]]), rule, rt.held_all)
            note(route, label, "D", ratio)
            assert ratio <= 1.0, f"{route} {label}: D[{k}] = {D[k]!r} outside its envelope"
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        # ---- C1
        S_want, ea_want = schur_ref(name, route, mu, rule)
        check_S_ea(route, label, rt, S, ea, S_want, ea_want, fr.scale_diag(rt, sm, mu, rule), cost)
        check_padding(M, nA)
        hr.check_held_system(rt, S, ea, mu, rule)
        if not rule.marquardt:
            assert np.all(S[rt.held, rt.held] == 1.0 + mu)
        h.schur_reduce()
        h.schur_solve()
        sc = h.backsub(mu)
        assert sc.status == 0
        dp = h.get_dp()
        newcams, newpts = h.get_params(1)
        cams, pts = h.get_params(0)
        hr.check_held_step(rt, gg, dp, hr.flat(cams, pts), hr.flat(newcams, newpts))
        if name == "wide":
            assert np.all(np.signbit(newcams[0, rt.ni:rt.ni + 3])) and np.all(np.signbit(cams[0, rt.ni:rt.ni + 3]))
            h.accept()
            assert np.all(np.signbit(h.get_params(0)[0][0, rt.ni:rt.ni + 3]))
        for j in np.flatnonzero(np.bincount(rt.j, minlength=nC) == 0):
            assert np.all(dp[cnp * j:cnp * j + cnp] == 0.0)
        # ---- C2
        eta, fe, kappa = fr.solve_judge(S, ea, dp[:nA])
        note(route, label, "dp_a eta", eta / ETA_MAX)
        note(route, label, "dp_a forward", fe / (2 * kappa * 1e-14))
        assert eta <= ETA_MAX, f"{route} {label}: backward error {eta:.3e} of the scaled system"
        assert fe <= 2 * kappa * 1e-14, f"{route} {label}: forward error {fe:.3e} (cond {kappa:.2e})"
        # ---- C3
        r, bound = fr.dpb_residual(rt, sm, dp, mu, rule)
        ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), bound)
        note(route, label, "dp_b", ratio)
        assert ratio <= 1.0, (f"{route} {label}: point {k // 3} entry {k % 3}: residual {float(r[k]):.3e} > bound "
                              f"{bound[k]:.3e}")
        # ---- C4
        got = dict(dp_l2=sc.dp_l2, gain_den=sc.gain_den, newp_l2=sc.newp_l2, new_cost=sc.new_cost)
        bad = []
        for what, (x, b) in fr.scalars(rt, sm, dp, newcams, newpts, mu, D=D).items():
            ratio = float(abs(ar.LD(got[what]) - x) / b)
            note(route, label, what, ratio)
            if not ratio <= 1.0:
                bad.append(f"{what} = {got[what]!r}, exact {float(x)!r}, bound {b:.3e}")
        assert not bad, f"{route} {label}: " + "; ".join(bad)
    finally:
        h.close()


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("name", ["tiny", "P7", "wide"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_one_damping_try_entrywise(route, name, rule, which_mu):
    """case 1"""
    one_try(route, name, which_mu, RULES[rule])


@pytest.mark.parametrize("route", list(ROUTES))
def test_linearize_with_coefficients(route):
    """case 2 (C6): psba_linearize(2, -2) on 7camsvarK.  S(mu) = 2 S_1(mu / 2), e_a(mu) = -2 e_a,1(mu / 2) exactly;
    the placeholder of a held coordinate is the coefficient, so the held diagonals are exactly 2 + mu."""
    rt, sm = ref("P7", route)
    nA = rt.nA
    mus, diag = hr.dampings(rt, sm)
    mu, cost = 2.0 * mus["big"], sm["cost"]
    h = handle(rt)
    try:
        h.linearize(2.0, -2.0)
        assert abs(h.max_diag() - 2e3 * mus["big"]) <= 1e-11 * 2e3 * mus["big"]
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        check_S_ea(route, "P7 (2, -2)", rt, S / 2.0, ea / -2.0, *schur_ref("P7", route, mu / 2.0),
                   np.sqrt(diag[:nA] + mu / 2.0), cost)
        check_padding(M, nA)
        hr.check_held_system(rt, S, ea, mu, coeff=2.0)
        assert np.all(S[rt.held, rt.held] == 2.0 + mu) and rt.held_pose.size == 6 * int(rt.held_poses.sum())
        h.schur_reduce()
        h.schur_solve()
        assert h.backsub(mu).status == 0
        assert np.all(h.get_dp()[rt.held_all] == 0.0)
    finally:
        h.close()


def test_gauss_newton():
    """case 3: 7camsvarK, {f, k1, k2}, poses 0 and 1 held, mu = 0 (without holds S is singular there:
    test_held_ref.py).  The status is 0, the solve of the scaled system holds free_ref.solve_judge's bounds, and dp_a
    equals the twin's reduced dense solve within that forward bound, 2 cond(D S D) 1e-14 in the scaling of S.  The
    point part is judged twice: free_ref.dpb_residual at mu = 0, and against the reduced solve in the scaling
    sqrt(diag V) within 2 cond 1e-14 of the system that solve inverts (the reduced N scaled by its own diagonal: the
    rule of test_gpu_dense_solve.py applied to the reference's own system, whose condition bounds that of S)."""
    import dense_ref as dr
    rt, sm = ref("P7", "kd-bal", True)
    nA, cost = rt.nA, sm["cost"]
    h = handle(rt)
    try:
        h.linearize(1.0, 1.0)
        h.schur_assemble(0.0)
        S, ea, M = read_system(h, nA)
        _, diag = hr.dampings(rt, sm)
        check_S_ea("kd-bal", "P7 mu = 0", rt, S, ea, *schur_ref("P7", "kd-bal", 0.0, fr.NO_RULE, True), np.sqrt(diag[:nA]),
                   cost)
        hr.check_held_system(rt, S, ea, 0.0)
        h.schur_reduce()
        h.schur_solve()
        sc = h.backsub(0.0)
        assert sc.status == 0
        dp = h.get_dp()
        assert np.all(dp[rt.held_all] == 0.0)
        eta, fe, kappa = fr.solve_judge(S, ea, dp[:nA])
        note("kd-bal", "P7 mu = 0", "dp_a eta", eta / ETA_MAX)
        note("kd-bal", "P7 mu = 0", "dp_a forward", fe / (2 * kappa * 1e-14))
        assert eta <= ETA_MAX and fe <= 2 * kappa * 1e-14, f"eta {eta:.3e}, forward {fe:.3e}, cond {kappa:.3e}"
        want = hr.reduced_solve(rt, 0.0, scaled=True)
        d = np.sqrt(np.diag(S))
        err = np.linalg.norm(d * (dp[:nA] - want[:nA])) / np.linalg.norm(d * want[:nA])
        note("kd-bal", "P7 mu = 0", "dp_a against the reduced solve", err / (2 * kappa * 1e-14))
        assert err <= 2 * kappa * 1e-14, f"dp_a against the reduced dense solve {err:.3e} (cond {kappa:.3e})"
        r, bound = fr.dpb_residual(rt, sm, dp, 0.0)
        ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), bound)
        note("kd-bal", "P7 mu = 0", "dp_b", ratio)
        assert ratio <= 1.0, f"point {k // 3} entry {k % 3}: residual {float(r[k]):.3e} > bound {bound[k]:.3e}"
        N, _ = hr.dense_normal(rt, rt.unheld_blocks())
        Nf = N[np.ix_(rt.free_all, rt.free_all)]
        dn = np.sqrt(np.diag(Nf))
        kappa_n = dr.cond2(Nf / np.outer(dn, dn))
        assert kappa_n >= kappa
        db = np.sqrt(sm["diagV"])
        err = np.linalg.norm(db * (dp[nA:] - want[nA:])) / np.linalg.norm(db * want[nA:])
        note("kd-bal", "P7 mu = 0", "dp_b against the reduced solve", err / (2 * kappa_n * 1e-14))
        assert err <= 2 * kappa_n * 1e-14, f"dp_b against the reduced dense solve {err:.3e} (cond {kappa_n:.3e})"
    finally:
        h.close()


def test_against_the_fixed_k_route():
    """case 4: all ten intrinsics masked at start_kc, poses 0 and 1 and one point held, against PSBA_CAMERA_FIXED_K with
    psba_set_distortion(start_kc) and psba_set_fixed of the same blocks, on 7camsvarK."""
    import psba_amd
    p = prob("P7")
    kc = start_kc(p["nC"])
    poses, pts = hr.flags(p["nC"], [0, 1]), hr.flags(p["nP"], [hr.point_with_views(p)])
    rt = hr.HeldRoute(p, 16, NONE, poses, pts)
    sm = hr.sums(rt)
    h = plain_handle(p, 16, NONE)
    h6 = psba_amd.Psba(0)
    try:
        h.set_held(poses, pts)
        h6.upload_problem(p)
        h6.set_distortion(kc)
        h6.set_fixed(poses, pts)
        h.linearize(1.0, 1.0)
        h6.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        assert abs(h6.max_diag() - h.max_diag()) <= 1e-11 * h.max_diag()
        h.schur_assemble(mu)
        h6.schur_assemble(mu)
        S, ea, _ = read_system(h, rt.nA)
        S6, ea6, _ = read_system(h6, 6 * p["nC"])
        rows = (CNP * np.arange(p["nC"])[:, None] + np.arange(10, 16)[None, :]).reshape(-1)
        d = np.sqrt(sm["diagU"] + mu)[rows]
        tol = 2 * scaled_tol(p)
        eS = (np.abs(S[np.ix_(rows, rows)] - S6) / np.outer(d, d)).max()
        ee = (np.abs(ea[rows] - ea6) / (d * np.sqrt(sm["cost"]))).max()
        note("kd-none", "P7 against fixed K", "S", eS / tol)
        note("kd-none", "P7 against fixed K", "e_a", ee / tol)
        assert eS <= tol and ee <= tol
        for hh in (h, h6):
            hh.schur_reduce()
            hh.schur_solve()
            assert hh.backsub(mu).status == 0
        dp, dp6 = h.get_dp(), h6.get_dp()
        dp = np.r_[dp[:rt.nA][rows], dp[rt.nA:]]
        err = np.abs(dp - dp6).max() / np.abs(dp6).max()
        note("kd-none", "P7 against fixed K", "dp", err / 1e-9)
        assert err <= 1e-9
        h.reset_params()
        h6.reset_params()
        res, _ = h.levmar(max_iter=8, tr_handoff=False)
        res6, _ = h6.levmar(max_iter=8, tr_handoff=False)
        assert abs(res.final_err - res6.final_err) <= 1e-6 * res6.final_err
    finally:
        h.close()
        h6.close()


def full_try(h, mu):
    h.schur_assemble(mu)
    buf = h.get_reduce_buffer().tobytes()
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    return buf, h.get_dp().tobytes(), (sc.dp_l2, sc.gain_den, sc.newp_l2, sc.new_cost)


def try_and_log(h, mu_rel):
    h.linearize(1.0, 1.0)
    md = h.max_diag()
    out = full_try(h, mu_rel if h.damping()[0] == fr.MARQUARDT else mu_rel * md)
    h.reset_params()
    _, log = h.levmar(max_iter=5, tr_handoff=False, log_cap=256)
    return out + (md, log.tobytes())


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("route", ["kd-bal", "fk"])
def test_no_mask_is_no_mask(route, rule):
    """case 5: all-zero masks, and masks set and then cleared, are bit for bit the handle that never called the verb:
    the reduce buffer, dp and the four scalars of one try and the whole log of a 5-iteration psba_levmar."""
    cnp, free = ROUTES[route]
    p = prob("P7")
    rule = RULES[rule]
    runs = {}
    for which in ("never", "zeros", "cleared"):
        h = plain_handle(p, cnp, free, rule)
        try:
            if which == "zeros":
                h.set_held(np.zeros(p["nC"]), np.zeros(p["nP"]))
            elif which == "cleared":
                h.set_held(hr.flags(p["nC"], [0, 1]), hr.flags(p["nP"], [3]))
                h.linearize(1.0, 1.0)
                h.set_held(None, None)
            assert which == "never" or h.held_counts() == (0, 0)
            runs[which] = try_and_log(h, 1e-3)
        finally:
            h.close()
    assert len(runs["never"][4]) > 0
    for which in ("zeros", "cleared"):
        for k, what in enumerate(("reduce buffer", "dp", "scalars", "max diag", "LM log")):
            assert runs[which][k] == runs["never"][k], f"{which}: {what}"


def test_two_runs_with_holds_are_bit_identical():
    """case 6: wide_problem(65), {f, k1, k2}, Marquardt (so that D is compared as well): no floating-point atomics."""
    rt, _ = ref("wide", "kd-bal")
    rule = RULES["marquardt"]
    out = []
    for _ in range(2):
        h = handle(rt, rule)
        try:
            h.linearize(1.0, 1.0)
            D = h.get_damping_diag().tobytes()
            out.append(full_try(h, MQ_MUS["big"]) + (D,))
        finally:
            h.close()
    assert out[0] == out[1] and len(out[0][3]) > 0


def test_the_look_ahead_with_holds():
    """case 7: the sequence of test_gpu_free_entrywise.py::test_the_second_diagonal_set_beyond_64_cameras with holds
    set: the try after the accepted look-ahead equals, bit for bit, that of a fresh handle set to the accepted
    parameters with the same holds; the held entries of the accepted parameters are the start's bits."""
    rt, _ = ref("wide", "kd-bal")
    rule, mu = RULES["marquardt"], MQ_MUS["big"]
    h, h2 = handle(rt, rule), None
    try:
        start = hr.flat(*h.get_params(0))
        cost, _ = h.begin()
        h.linearize(1.0, 1.0)
        D0 = h.get_damping_diag()
        h.schur_assemble(mu)
        h.schur_reduce()
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        sc = h.backsub_wait()
        assert sc.status == 0 and sc.new_cost < cost
        cams, pts = h.get_params(1)
        h.accept()
        now = hr.flat(*h.get_params(0))
        assert now[rt.held_all].tobytes() == start[rt.held_all].tobytes() and np.any(now != start)
        D1 = h.get_damping_diag()
        assert D1.tobytes() != D0.tobytes() and np.all(D1[rt.held_all] == 1.0)
        h.linearize(1.0, 1.0)                               # (nothing left to do: the linearization came with the accept)
        assert h.get_damping_diag().tobytes() == D1.tobytes()
        check_obs_blocks(h, rt)
        got = full_try(h, mu)
        h2 = handle(rt, rule)
        h2.set_params(cams, pts)
        h2.linearize(1.0, 1.0)
        assert h2.get_damping_diag().tobytes() == D1.tobytes()
        want = full_try(h2, mu)
        assert got[0] == want[0], "the reduce buffer after the accepted look-ahead"
        assert got[1] == want[1] and got[2] == want[2]
    finally:
        h.close()
        if h2 is not None:
            h2.close()


@functools.lru_cache(maxsize=None)
def shared_ref_ring():
    labels = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    start, kc0, _, _ = sr.shared_ring(labels)
    rt = hr.HeldSharedRoute(start, labels, BAL, kc0, hr.flags(6, [0, 1]))
    return rt, hr.sums(rt)


def shared_handle(rt, rule, order):
    import psba_amd
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(rt.p)
    h.set_distortion(rt.kc)
    calls = {"mask": lambda: h.set_intrinsics_mask(rt.free), "groups": lambda: h.set_intrinsics_groups(rt.labels),
             "damping": lambda: h.set_damping(rule.kind, rule.dmin, rule.dmax),
             "holds": lambda: h.set_held(rt.held_poses, rt.held_pts)}
    for c in order:
        calls[c]()
    return h


def test_composition_with_mask_groups_and_damping():
    """case 8: shared_ring with two groups of three cameras, {f, k1, k2}, Marquardt, poses 0 and 1 held (both members
    of the first group, camera 0 its representative).  S and e_a against shared_ref's fold of the held route's blocks
    within shared_tol; the held pose entries exact; the members' intrinsics bit-identical after an accepted step; the
    opposite order of calls gives the same bits."""
    rt, sm = shared_ref_ring()
    rule, mu = RULES["marquardt"], MQ_MUS["big"]
    nA, cost = rt.nA, sm["cost"]
    assert rt.rep[:3].tolist() == [0, 0, 0] and rt.held_poses[:2].all()
    bufs = []
    for order in (("mask", "groups", "damping", "holds"), ("holds", "groups", "mask", "damping")):
        h = shared_handle(rt, rule, order)
        try:
            assert h.held_counts() == (2, 0) and h.intrinsics_groups()[1] == 2
            c0, md = h.begin(1.0, 1.0)
            fdiag, ffree = rt.folded_diag(sm)
            want_md = float(fdiag[ffree].max())
            assert abs(c0 - cost) <= 1e-12 * cost and abs(md - want_md) <= 1e-11 * want_md
            h.linearize(1.0, 1.0)
            D = h.get_damping_diag()
            assert np.all(D[rt.held] == 1.0)
            h.schur_assemble(mu)
            S, ea, M = read_system(h, nA)
            buf = M.tobytes()
            if not bufs:
                S_want, ea_want = hr.shared_schur_ref(rt, sm, mu, rule)
                Dr = sr.damp_ref(rt, sm, rule)[0]
                eS, ee = sr.scaled_errors(S, ea, S_want, ea_want, np.sqrt(fdiag[:nA] + mu * Dr[:nA]), cost)
                note("kd-bal", "shared ring", "S", eS / rt.tol)
                note("kd-bal", "shared ring", "e_a", ee / rt.tol)
                assert eS <= rt.tol and ee <= rt.tol, f"scaled S {eS:.3e}, e_a {ee:.3e}, tol {rt.tol:.3e}"
                check_padding(M, nA)
                sr.check_mirror(S)
                sr.check_embedded(S, ea, rt.away, 1.0 + mu * 1.0)
                hr.check_held_system(rt, S, ea, mu, rule)
            h.schur_reduce()
            h.schur_solve()
            sc = h.backsub(mu)
            assert sc.status == 0 and sc.new_cost < cost
            dp = h.get_dp()
            cams, pts = h.get_params(0)
            newcams, newpts = h.get_params(1)
            hr.check_held_step(rt, None, dp, hr.flat(cams, pts), hr.flat(newcams, newpts))
            assert np.any(dp[:nA].reshape(-1, CNP)[:2, 0] != 0.0)   # the intrinsics of a held pose move
            h.accept()
            acc, _ = h.get_params(0)
            assert acc.tobytes() == newcams.tobytes()
            assert np.array_equal(acc[:, :10], acc[rt.rep][:, :10]) and acc[:2, 10:].tobytes() == cams[:2, 10:].tobytes()
            bufs.append((buf, dp.tobytes(), D.tobytes(), (sc.dp_l2, sc.gain_den, sc.newp_l2, sc.new_cost)))
        finally:
            h.close()
    assert bufs[0] == bufs[1], "the order of the calls changes the bits"


LM_ITERS = 15


@functools.lru_cache(maxsize=None)
def ring_twin_lm():
    start, kc0, poses = hr.held_ring()
    t = hr.HeldTwin(start, kc0, BAL, poses)
    res, log = t.levmar(max_iter=LM_ITERS)
    return start, kc0, poses, res, log


def test_levmar_on_the_ring_scene_with_two_poses_held():
    """case 9: the ring scene with the true poses of cameras 0 and 1 written into the start and held, {f, k1, k2}.
    The dense LM with the held columns deleted falls below 1e-6 of the starting cost within 15 iterations without
    ending on a stop test (asserted first); the device's final cost is within 1e-5 relative of it (the rule of
    test_gpu_freekd.py::test_levmar_against_the_twin) and poses 0 and 1 are the start's bits after the run."""
    start, kc0, poses, want, wlog = ring_twin_lm()
    assert want.flag == 0 and want.iters == LM_ITERS and want.final_err <= 1e-6 * want.init_err
    h = plain_handle(start, 16, BAL, kc=kc0)
    try:
        h.set_held(poses, None)
        c0, _ = h.get_params(0)
        res, log = h.levmar(max_iter=LM_ITERS, tr_handoff=False, log_cap=256)
        c1, _ = h.get_params(0)
        assert abs(res.init_err - want.init_err) <= 1e-12 * want.init_err
        n = min(len(log), len(wlog), 6)
        assert n >= 4 and np.array_equal(log[:n, 4], wlog[:n, 4])
        np.testing.assert_allclose(log[:n, 1], wlog[:n, 1], rtol=1e-6)
        rel = abs(res.final_err - want.final_err) / want.final_err
        note("kd-bal", "ring", "LM final cost", rel / 1e-5)
        assert rel <= 1e-5, f"final cost {res.final_err!r}, the twin's {want.final_err!r}"
        assert c1[:2, 10:].tobytes() == c0[:2, 10:].tobytes() and np.any(c1[2:, 10:] != c0[2:, 10:])
        assert np.all(c1[:, 0] != c0[:, 0])
    finally:
        h.close()


def test_interface():
    """case 10"""
    import psba_amd
    from psba_amd import capi
    p = prob("P7")
    nC, nP = int(p["nC"]), int(p["nP"])
    poses, pts = hr.flags(nC, [0, 1]), hr.flags(nP, [5])
    h = psba_amd.Psba(0)
    try:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        for call in (lambda: h.set_held(None, None), lambda: h.set_held(poses, pts)):     # before an upload
            with pytest.raises(psba_amd.PsbaError) as ei:
                call()
            assert ei.value.code == -6
        h.upload_problem(p)
        assert h.held_counts() == (0, 0)
        h.set_held(poses, pts)
        assert h.held_counts() == (2, 1)
        h.set_held(None, pts)
        assert h.held_counts() == (0, 1)
        h.set_held(poses, None)
        assert h.held_counts() == (2, 0)
        assert capi.lib.psba_held_counts(h._h, None, None) == 0
        # every pose and every point: refused, and nothing changes
        with pytest.raises(psba_amd.PsbaError) as ei:
            h.set_held(np.ones(nC), np.ones(nP))
        assert ei.value.code == -1 and h.held_counts() == (2, 0)
        h.set_held(np.ones(nC), None)                        # every pose alone is legal (points and intrinsics move)
        h.set_held(None, np.ones(nP))
        h.set_held(poses, pts)
        # psba_set_fixed and the covariance keep refusing the model
        with pytest.raises(psba_amd.PsbaError) as ei:
            h.set_fixed(poses, None)
        assert ei.value.code == -6 and "PSBA_CAMERA_FREE_KD" in str(ei.value) and "fixed-intrinsics camera block only" in str(ei.value)
        with pytest.raises(psba_amd.PsbaError) as ei:
            h.covariance(mu=0.0, scale=1.0)
        assert ei.value.code == -6
        # setting the masks discards a queued linearization and invalidates the two test hooks
        h.set_damping(psba_amd.DAMPING_MARQUARDT)
        h.linearize(1.0, 1.0)
        h.free_obs_blocks()
        h.get_damping_diag()
        h.set_held(poses, pts)
        for call in (h.free_obs_blocks, h.get_damping_diag, lambda: h.schur_assemble(1e-3)):
            with pytest.raises(psba_amd.PsbaError) as ei:
                call()
            assert ei.value.code == -6
        h.linearize(1.0, 1.0)
        mu = 1e-3
        h.schur_assemble(mu)
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        with pytest.raises(psba_amd.PsbaError) as ei:       # a try is in flight: refused, nothing changes
            h.set_held(None, None)
        assert ei.value.code == -6 and "in flight" in str(ei.value) and h.held_counts() == (2, 1)
        sc = h.backsub_wait()
        assert sc.status == 0
        h.set_held(poses, None)                              # ... discards the linearization queued ahead
        assert h.held_counts() == (2, 0)
        h.accept()
        for call in (h.free_obs_blocks, h.get_damping_diag, lambda: h.schur_assemble(mu)):   # (they came with an
            with pytest.raises(psba_amd.PsbaError) as ei:                                    # accepted look-ahead)
                call()
            assert ei.value.code == -6
        h.linearize(1.0, 1.0)
        W, B, _ = h.free_obs_blocks()
        assert np.all(np.abs(B).sum(axis=(1, 2)) > 0.0)      # no point is held any more
        assert np.all(W[np.asarray(p["jidx"]) <= 1][:, 10:, :] == 0.0)
        # psba_set_params may move a held block
        cams, pts3 = h.get_params(0)
        moved = cams.copy()
        moved[0, 10:] += 1e-3
        h.set_params(moved, pts3)
        assert np.array_equal(h.get_params(0)[0], moved) and h.held_counts() == (2, 0)
        # a new upload resets to none
        h.upload_problem(p)
        assert h.held_counts() == (0, 0)
    finally:
        h.close()
    # blocks of 11 take the verb; six-parameter blocks refuse it and name psba_set_fixed
    for model, ok in ((psba_amd.CAMERA_FREE_K, True), (psba_amd.CAMERA_FIXED_K, False)):
        ho = psba_amd.Psba(0)
        try:
            ho.set_camera_model(model)
            ho.upload_problem(p)
            if ok:
                ho.set_held(poses, pts)
                assert ho.held_counts() == (2, 1)
                with pytest.raises(psba_amd.PsbaError) as ei:
                    ho.set_fixed(poses, None)
                assert ei.value.code == -6 and "fixed-intrinsics camera block only" in str(ei.value)
            else:
                with pytest.raises(psba_amd.PsbaError) as ei:
                    ho.set_held(poses, pts)
                assert ei.value.code == -6 and "psba_set_fixed" in str(ei.value) and ho.held_counts() == (0, 0)
        finally:
            ho.close()
