"""psba_set_camera_masks on the GPU: per-camera masks of the ten intrinsics on the 16-block route (PSBA_CAMERA_FREE_KD;
DESIGN 7n).  The reference and its judges are tests/cammask_ref.py (on weight_ref.py, prior_ref.py, held_ref.py,
shared_ref.py, free_ref.py, freecov_ref.py and freepcg_ref.py, their constants, scaled_tol and ETA_MAX unchanged; no
constant is fitted to a GPU result except the measured gaps of case 8, which are named as such).  Needs an MI355X.

Inputs: tiny_problem (2 cameras), 7camsvarK, wide_problem(64) and wide_problem(65) (the second trip of the finalize grid
for blocks of 16), the first 450 points of 54camsvarK, and the ring scenes of freekd_twin / held_ref.  The mixed table
cycles by j % 4 through the rows all free, {f, k1, k2}, none, {f}; poses 0 and 2 are held with it, so camera 2 (row
none) is wholly fixed.

  1  equal rows are the global mask, bit for bit, on both solvers; the AND with the global mask.
  2  one damping try entry by entry with the mixed table, under both dampings and both mus.
  3  groups: the entrywise judges of test_gpu_shared_intrinsics.py with a table constant on each group, the fold judged
     alone; unequal rows inside a group are refused by whichever setter comes second.
  4  composition on 54camsvarK: the mixed table, held poses and a held point, priors, Huber with sigmas.
  5  PSBA_SOLVER_SPARSE: the stored blocks are the dense route's bits, the block of a wholly fixed camera, dp, two runs.
  6  the covariance: exact zeros at masked coordinates, the live part by freecov_ref's judges.
  7  no table is no table; the look-ahead linearization; a table set between two psba_levmar calls.
  8  recovery of the mixed ring scene against cammask_ref.CamMaskTwin.
  9  the interface.
The module prints the worst ratio (found / allowed) per case and quantity; DESIGN 7n keeps the table."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import cammask_ref as cm
import free_ref as fr
import freecov_ref as fc
import freepcg_ref as fp
import held_ref as hr
import prior_ref as pr
import shared_ref as sr
import weight_ref as wr
from freekd_twin import BAL, CNP, start_kc, tiny_problem, wide_problem
from test_freekd_twin import P7, P54, scaled_tol
from test_gpu_dense_solve import ETA_MAX

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

LD = ar.LD
RULES = {"identity": fr.NO_RULE, "marquardt": fr.Rule(fr.MARQUARDT)}
MQ_MUS = {"big": 1e-3, "small": 1e-6}    # Marquardt's mu is relative (test_gpu_damping.py)
DENSE, SPARSE = 0, 2
TRY_TOL = 1e-12                          # of the conjugate gradients, as in test_gpu_free_sparse.py
TWIN_FLAG = {0: 3, 1: 5, 2: 4, 3: 6}     # freekd_twin's LM flags -> PSBA_ITER_CONTINUE, _DP_NO_CHANGE, _ERR, _ERR_SMALL_ENOUGH
E_INVALID, E_STATE = -1, -6
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        keys = sorted({k for k, _ in WORST})
        lines = [f"  {k}: " + ", ".join(f"{q} {v:.2e}" for (kk, q), v in WORST.items() if kk == k) for k in keys]
        print("\ncamera masks: worst ratio found / allowed per case and quantity:\n" + "\n".join(lines))


def note(case, what, ratio):
    WORST[(case, what)] = max(WORST.get((case, what), 0.0), float(ratio))
    print(f"{case} {what}: {float(ratio):.3e}")


def assert_judged(case, out):
    for what, ratio in out.items():
        note(case, what, ratio)
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, f"{case}: found / allowed above 1: {bad}"


@functools.lru_cache(maxsize=None)
def prob(name):
    return {"tiny": tiny_problem, "P7": P7, "P54": P54, "wide-below": lambda: wide_problem(64),
            "wide-above": lambda: wide_problem(65)}[name]()


def mixed_holds(name):
    p = prob(name)
    return hr.flags(p["nC"], [1] if name == "tiny" else [0, 2])


def open_handle(p, free=fr.ALL, rule=fr.NO_RULE, solver=DENSE, kc=None, model=None):
    import psba_amd
    h = psba_amd.Psba(0)
    if solver:
        h.set_solver(solver, tol=TRY_TOL, max_iter=500)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD if model is None else model)
    h.upload_problem(p)
    if model is None:
        h.set_distortion(start_kc(p["nC"]) if kc is None else kc)
        h.set_intrinsics_mask(free)
        assert h.camera_block() == CNP and h.schur_path() == (6 if solver == SPARSE else 5)
        if rule.marquardt:
            h.set_damping(rule.kind, rule.dmin, rule.dmax)
    return h


def handle(rt, rule=fr.NO_RULE, solver=DENSE, table=True):
    """the device's handle of a route: mask, damping, the table, holds, priors, weighting"""
    h = open_handle(rt.p, rt.free, rule, solver, getattr(rt, "kc", None))
    if table:
        h.set_camera_masks(rt.table)
        assert np.array_equal(h.camera_masks(), rt.table.astype(np.uint8))
    if rt.held_poses.any() or rt.held_pts.any():
        h.set_held(rt.held_poses, rt.held_pts)
    if hasattr(rt, "pri") and sum(rt.pri.counts()):
        h.set_priors(**rt.pri.args())
    if getattr(rt, "weighted", False):
        h.set_obs_weighting(rt.kind, rt.c, rt.sigma if rt.has_sigma else None)
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


def mu_for(h, rule, rel=1e-3):
    return rel if rule.marquardt else rel * h.max_diag()


def snapshot(h, rule, solver=DENSE, iters=10):
    """everything one try and a psba_levmar of `iters` iterations return, as bytes: the system ([S | e_a] of the reduce
    buffer, or the stored blocks and e_a with the iteration count and relres), D, max_diag, dp, the four scalars, the
    proposal and the log"""
    out = {}
    h.linearize(1.0, 1.0)
    md = h.max_diag()
    out["max_diag"] = md
    out["D"] = h.get_damping_diag().tobytes() if rule.marquardt else b""
    mu = mu_for(h, rule)
    h.schur_assemble(mu)
    if solver == SPARSE:
        jk, val, ea = h.get_sparse_S()
        out["system"] = (jk.tobytes(), val.tobytes(), ea.tobytes())
    else:
        out["system"] = h.get_reduce_buffer().tobytes()
    h.schur_reduce()
    assert h.schur_solve() == 0
    if solver == SPARSE:
        out["pcg"] = h.pcg_info()[:2]
    sc = h.backsub(mu)
    assert sc.status == 0
    out["dp"] = h.get_dp().tobytes()
    out["scalars"] = (sc.dp_l2, sc.gain_den, sc.newp_l2, sc.new_cost)
    out["proposal"] = tuple(x.tobytes() for x in h.get_params(1))
    h.reset_params()
    _, log = h.levmar(max_iter=iters, tr_handoff=False, log_cap=256)
    assert len(log) > 0
    out["log"] = log.tobytes()
    return out


def assert_same(a, b, label):
    assert set(a) == set(b)
    for k in a:
        assert a[k] == b[k], f"{label}: {k} differs"


# ---- 1. equal rows are the global mask ------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", [DENSE, SPARSE], ids=["dense", "sparse"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("row", [cm.F_K1_K2, cm.NONE], ids=["f-k1-k2", "none"])
@pytest.mark.parametrize("name", ["P7", "wide-above"])
def test_equal_rows_are_the_global_mask(name, row, rule, solver):
    """case 1: handle A has a table whose rows all equal m under the global mask all free, handle B the global mask m and
    no table: bit-identical systems, D, max_diag, dp, scalars, proposals and 10-iteration LM logs"""
    p, rule = prob(name), RULES[rule]
    runs = []
    for which in ("table", "global"):
        h = open_handle(p, fr.ALL if which == "table" else row, rule, solver)
        try:
            if which == "table":
                h.set_camera_masks(cm.constant_table(p["nC"], row))
                assert h.intrinsics_mask() == fr.ALL                # the global flags stay what they were
            runs.append(snapshot(h, rule, solver))
        finally:
            h.close()
    assert_same(runs[0], runs[1], f"{name} {row} {rule}")


@pytest.mark.parametrize("rule", list(RULES))
def test_the_table_is_anded_with_the_global_mask(rule):
    """case 1, the AND: the global mask g with rows c equals the global mask all free with rows g & c, bit for bit"""
    p, rule = prob("P7"), RULES[rule]
    c = cm.mixed_table(p["nC"])
    runs = []
    for free, table in ((BAL, c), (fr.ALL, c & np.asarray(BAL, dtype=np.uint8)[None, :])):
        h = open_handle(p, free, rule)
        try:
            h.set_camera_masks(table)
            runs.append(snapshot(h, rule))
        finally:
            h.close()
    assert_same(runs[0], runs[1], "the AND")


# ---- 2. one damping try, entry by entry -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mixed_ref(name):
    """(CamMaskRoute with the mixed table and the holds of the module docstring, its extended-precision sums)"""
    p = prob(name)
    rt = cm.CamMaskRoute(p, cm.mixed_table(p["nC"]), fr.ALL, mixed_holds(name))
    return rt, wr.sums(rt)


def test_the_mixed_table_holds_every_kind_of_row():
    kinds = set()
    for name in ("P7", "wide-below", "wide-above", "P54"):
        rt, _ = mixed_ref(name)
        kinds |= {tuple(r) for r in rt.table.astype(int).tolist()}
        assert rt.fixed_cams.tolist() == [2]                        # one camera is wholly fixed
        assert {tuple(r) for r in rt.table.astype(int).tolist()} == set(cm.MIXED_ROWS)
    assert kinds == set(cm.MIXED_ROWS)
    assert {tuple(r) for r in mixed_ref("tiny")[0].table.astype(int).tolist()} == {fr.ALL, cm.F_K1_K2}


def device_try(h, rt, mu, rule):
    """one damping try on the device with everything weight_ref.judge reads, and W of psba_get_free_obs_blocks"""
    got = {}
    got["cost"] = h.residual()
    got["prior_cur"] = h.prior_cost()
    got["w_cur"] = h.get_obs_weights(0)
    h.linearize(1.0, 1.0)
    got["max_diag"] = h.max_diag()
    got["g"] = h.get_gradient()
    got["D"] = h.get_damping_diag() if rule.marquardt else None
    got["W"] = h.free_obs_blocks()[0]
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


def judge_try(case, rt, sm, mu, rule, got):
    """weight_ref.judge: S and e_a against the 80-bit schur_ref of the route with scaled_tol, the exact parts
    (check_exact_parts and the held columns: zeros, placeholders, the mirror), check_damp_diag, g, max_diag, dp_a by
    solve_judge, dp_b by dpb_residual, the try scalars and the costs; then the table's own exact parts"""
    out = wr.judge(rt, sm, mu, rule, got, scaled_tol(rt.p), ETA_MAX)
    assert {"S", "e_a", "g", "max_diag", "dp_a eta", "dp_a forward", "dp_b", "dp_l2", "gain_den", "newp_l2", "new_cost"} <= set(out)
    assert not rule.marquardt or "D" in out
    assert_judged(case, out)
    cm.check_table_parts(rt, got["W"], got["cams"], got["newcams"])
    dh = mu * float(rule.clamp(1.0)) if rule.marquardt else mu
    assert np.all(got["S"][rt.held_table, rt.held_table] == 1.0 + dh)
    for j in rt.fixed_cams:                                         # a wholly fixed camera: a diagonal block, nothing else
        rows = np.arange(CNP * j, CNP * j + CNP)
        assert np.array_equal(got["S"][np.ix_(rows, rows)], (1.0 + dh) * np.eye(CNP))
        assert np.all(got["dp"][rows] == 0.0) and got["newcams"][j].tobytes() == got["cams"][j].tobytes()


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("name", ["tiny", "P7", "wide-below", "wide-above", "P54"])
def test_one_damping_try_entrywise(name, rule, which_mu):
    """case 2"""
    rt, sm = mixed_ref(name)
    rule = RULES[rule]
    mus, _ = hr.dampings(rt, sm)
    mu = (MQ_MUS if rule.marquardt else mus)[which_mu]
    h = handle(rt, rule)
    try:
        got = device_try(h, rt, mu, rule)
    finally:
        h.close()
    judge_try(f"{name} {rule}", rt, sm, mu, rule, got)


# ---- 3. groups ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shared_ref_wide(nC):
    p = wide_problem(nC)
    lab = sr.wide_labels(nC).astype(np.int32)
    rt = cm.CamMaskSharedRoute(p, lab, cm.group_table(lab), fr.ALL)
    sm = hr.sums(rt)
    mus, fdiag = sr.dampings(rt, sm)
    return rt, sm, mus, fdiag


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("nC", [64, 65])
def test_groups_with_a_table_constant_on_each_group(nC, which_mu):
    """case 3: shared_ref's labelling of wide_problem(64 / 65), the table constant on each group and mixed across them:
    G1 to G4 of test_gpu_shared_intrinsics.py on the reduced system, and the fold alone against the 80-bit fold of the
    same handle's unfolded buffer"""
    rt, sm, mus, fdiag = shared_ref_wide(nC)
    nA, mu, cost = rt.nA, mus[which_mu], sm["cost"]
    case = f"groups wide({nC}) {which_mu}"
    assert {tuple(r) for r in rt.table.astype(int).tolist()} == set(cm.MIXED_ROWS)
    h = handle(rt)
    try:
        h.linearize(1.0, 1.0)
        h.schur_assemble(mu)
        M0 = h.get_reduce_buffer().reshape(-1, (nA + 31) // 32 * 32).copy()
        h.set_intrinsics_groups(rt.labels)
        assert np.array_equal(h.intrinsics_groups()[0], rt.rep)
        h.linearize(1.0, 1.0)
        want_md = float(fdiag[rt.folded_diag(sm)[1]].max())
        assert abs(h.max_diag() - want_md) <= 1e-11 * want_md
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        # ---- G1
        S_want, ea_want = cm.shared_schur_ref(rt, sm, mu)
        eS, ee = sr.scaled_errors(S, ea, S_want, ea_want, np.sqrt(fdiag[:nA] + mu), cost)
        note(case, "S", eS / rt.tol)
        note(case, "e_a", ee / rt.tol)
        assert eS <= rt.tol and ee <= rt.tol, f"{case}: scaled S {eS:.3e}, e_a {ee:.3e}, tol {rt.tol:.3e}"
        check_padding(M, nA)
        sr.check_mirror(S)
        sr.check_embedded(S, ea, rt.away, 1.0 + mu)
        hr.check_held_system(rt, S, ea, mu)
        # ---- G2
        Fx, Fb, ex, eb, _ = cm.fold_bound(M0, rt, mu)
        low = np.tril(np.ones((nA, nA), dtype=bool))
        rS, kS = ar.excess(S[low], Fx[low], Fb[low])
        re, ke = ar.excess(ea, ex, eb)
        note(case, "the fold alone S", rS)
        note(case, "the fold alone e_a", re)
        assert rS <= 1.0 and re <= 1.0, f"{case}: fold S {rS:.3e} (lower entry {kS}), e_a {re:.3e} (entry {ke})"
        # ---- G3
        h.schur_reduce()
        h.schur_solve()
        sc = h.backsub(mu)
        assert sc.status == 0
        dp = h.get_dp()
        newcams, newpts = h.get_params(1)
        cams, _ = h.get_params(0)
        dpa = dp[:nA].reshape(-1, CNP)
        assert np.array_equal(dpa[:, :10], dpa[rt.rep][:, :10]) and np.array_equal(newcams[:, :10], newcams[rt.rep][:, :10])
        assert np.all(dp[:nA][rt.held] == 0.0)
        assert newcams[:, :10][~rt.cam_free].tobytes() == cams[:, :10][~rt.cam_free].tobytes()
        emb = dp[:nA].copy()
        emb[rt.away] = 0.0
        eta, fe, kappa = fr.solve_judge(S, ea, emb)
        note(case, "dp_a eta", eta / ETA_MAX)
        note(case, "dp_a forward", fe / (2 * kappa * 1e-14))
        assert eta <= ETA_MAX and fe <= 2 * kappa * 1e-14, f"{case}: eta {eta:.3e}, forward {fe:.3e} (cond {kappa:.2e})"
        r, bound = fr.dpb_residual(rt, sm, dp, mu)
        ratio, k = ar.excess(r, np.zeros(r.shape, LD), bound)
        note(case, "dp_b", ratio)
        assert ratio <= 1.0, f"{case}: point {k // 3} entry {k % 3}: residual {float(r[k]):.3e} > {bound[k]:.3e}"
        got = dict(dp_l2=sc.dp_l2, gain_den=sc.gain_den, newp_l2=sc.newp_l2, new_cost=sc.new_cost)
        out = {what: float(abs(LD(got[what]) - x) / b) for what, (x, b) in sr.scalars(rt, sm, dp, newcams, newpts, mu).items()}
        assert_judged(case, out)
    finally:
        h.close()


@pytest.mark.parametrize("second", ["masks", "groups"])
def test_unequal_rows_inside_a_group_are_refused(second):
    """case 3: either setter called second returns PSBA_E_INVALID with the camera and the coordinate; the next try gives
    the bits it gave before the refused call"""
    import psba_amd
    rt, _, _, _ = shared_ref_wide(65)
    bad = rt.table.astype(np.uint8).copy()
    j = int(np.flatnonzero(rt.rep != np.arange(rt.nC))[0])           # the first camera that is not its group's representative
    bad[j, 6] = 1 - bad[j, 6]
    h = open_handle(rt.p, fr.ALL, kc=rt.kc)
    try:
        if second == "masks":
            h.set_camera_masks(rt.table)
            h.set_intrinsics_groups(rt.labels)
            call = lambda: h.set_camera_masks(bad)                  # noqa: E731
        else:
            h.set_camera_masks(bad)
            call = lambda: h.set_intrinsics_groups(rt.labels)       # noqa: E731
        before = snapshot(h, fr.NO_RULE, iters=3)
        h.reset_params()
        with pytest.raises(psba_amd.PsbaError) as ei:
            call()
        text = str(ei.value)
        assert ei.value.code == E_INVALID and f"camera {j} " in text and "coordinate 6 (k2)" in text, text
        want = rt.table.astype(np.uint8) if second == "masks" else bad
        assert np.array_equal(h.camera_masks(), want)
        assert h.intrinsics_groups()[1] == (np.unique(rt.rep).size if second == "masks" else rt.nC)
        assert_same(snapshot(h, fr.NO_RULE, iters=3), before, "after the refused call")
    finally:
        h.close()


# ---- 4. composition -----------------------------------------------------------------------------------------------------------

MASKED_PRIOR_CAM, FREE_PRIOR_CAM = 6, 4      # rows none (its pose is free) and all free of the mixed table


@functools.lru_cache(maxsize=None)
def composed_ref():
    """54camsvarK: the mixed table, poses 0 and 2 and one point held, weight_ref's drawn priors (by j % 4: full,
    diagonal, none, rank 2) and a full block on camera 6, whose ten intrinsics are masked; Huber with drawn sigmas"""
    p = prob("P54")
    nC = int(p["nC"])
    table, poses = cm.mixed_table(nC), hr.flags(nC, [0, 2])
    pts = hr.flags(p["nP"], [hr.point_with_views(p)])
    rt0 = cm.CamMaskRoute(p, table, fr.ALL, poses, pts)
    pri = pr.draw_priors(rt0)
    rng = np.random.default_rng(11)
    j = MASKED_PRIOR_CAM
    assert not np.any(pri.cam_info[j]) and np.any(pri.cam_info[FREE_PRIOR_CAM]) and not rt0.cam_free[j].any()
    w = np.sqrt(hr.sums(rt0)["diagU"].reshape(nC, CNP)[j])
    u = rng.standard_normal(CNP)
    u /= np.linalg.norm(u)
    pri.cam_info[j] = np.outer(w, w) * (0.7 * np.eye(CNP) + 0.3 * CNP * np.outer(u, u))
    pri.cam_mean[j] = rt0.current()[0][j] + rng.uniform(-3.0, 3.0, CNP) / np.sqrt(np.diag(pri.cam_info[j]))
    sigma, c = wr.draw_weighting(rt0, wr.HUBER)
    rt = cm.CamMaskRoute(p, table, fr.ALL, poses, pts, pri, (wr.HUBER, c), sigma)
    return rt, wr.sums(rt)


@pytest.mark.parametrize("rule", list(RULES))
def test_composition_on_54camsvarK(rule):
    """case 4: judged entrywise by weight_ref.judge.  The prior's rows and columns at the masked coordinates of camera 6
    are dropped (its intrinsic rows of S are the placeholder alone) while g of its free coordinates takes the whole d:
    the reference's g carries L d with the masked deviations in it, and differs from the one without them by more
    than the envelope g is judged with"""
    rt, sm = composed_ref()
    rule = RULES[rule]
    mus, _ = hr.dampings(rt, sm)
    mu = MQ_MUS["big"] if rule.marquardt else mus["big"]
    h = handle(rt, rule)
    try:
        assert h.prior_counts() == rt.pri.counts() and h.held_counts() == (2, 1)
        got = device_try(h, rt, mu, rule)
    finally:
        h.close()
    judge_try(f"P54 composed {rule}", rt, sm, mu, rule, got)
    j = MASKED_PRIOR_CAM
    pose = np.arange(CNP * j + 10, CNP * j + CNP)
    dC = rt.pri.cam_mean[j] - got["cams"][j]
    assert np.all(dC[:10] != 0.0)
    masked_part = rt.pri.cam_info[j][10:, :10] @ dC[:10]              # what g of the pose would lose with d cut to the free part
    assert np.all(np.abs(masked_part) > 4.0 * sm["envg"][pose])
    assert np.all(got["g"][CNP * j:CNP * j + 10] == 0.0)


# ---- 5. the sparse solver -------------------------------------------------------------------------------------------------------

def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def sparse_try(h, mu):
    h.schur_assemble(mu)
    jk, val, ea = h.get_sparse_S()
    h.schur_reduce()
    rc = h.schur_solve()
    iters, relres, _, _ = h.pcg_info()
    sc = h.backsub(mu)
    return dict(jk=jk, val=val, ea=ea, rc=rc, iters=iters, relres=relres, sc=sc, dp=h.get_dp())


def one_step(M, x):
    """the solve of x u = 1 by one step of the conjugate gradients with the preconditioner entry M, every product and
    the quotient rounded once, as k_fpcg_start, k_fpcg_spmv and k_fpcg_update form them when one entry of the
    right-hand side is 1.0 and every other term of every sum is an exact zero: z = p = M, q = x p, alpha = (1 M) /
    (p q), u = alpha p"""
    M, x = np.float64(M), np.float64(x)
    q = x * M
    alpha = M / (M * q)
    return float(alpha * M)


def fixed_block_solves(h, rt, t, mu):
    """The device's inverse of the wholly fixed camera's diagonal block, observed through psba_schur_solve on
    overwritten blocks (the constructed-system path of test_gpu_free_sparse.py): the fixed camera keeps the block the
    device stored, every other diagonal block is the identity, the off-diagonal blocks are zero, and the right-hand
    side is 1.0 at ONE coordinate of the fixed camera.  Then x = alpha M e_r: -> [(r, the block's entry, x_r, whether
    every other entry of x is exactly 0 after exactly one iteration)]"""
    nA = rt.nA
    j = int(rt.fixed_cams[0])
    val = np.zeros_like(t["val"])
    for s, (a, b) in enumerate(t["jk"]):
        if a == b:
            val[s] = t["val"][s] if a == j else np.eye(CNP)
    slot = np.flatnonzero((t["jk"][:, 0] == j) & (t["jk"][:, 1] == j))[0]
    out = []
    for r in (0, 6, 9, 10, 15):                                     # intrinsics, distortion, the held pose
        b = np.zeros(nA)
        b[CNP * j + r] = 1.0
        h.schur_assemble(mu)
        h.set_sparse_S(val, b)
        assert h.schur_solve() == 0
        x = h.get_dp()[:nA].copy()
        iters = h.pcg_info()[0]
        h.backsub(mu)
        got = float(x[CNP * j + r])
        x[CNP * j + r] = 0.0
        out.append((r, float(t["val"][slot][r, r]), got, bool(iters == 1 and np.all(x == 0.0))))
    return out


@pytest.mark.parametrize("rule", list(RULES))
def test_sparse_blocks_are_the_dense_routes_bits(rule):
    """case 5 with the settings of case 4: the stored blocks and e_a are the bits the dense route stores at the same
    places; the diagonal block of the wholly fixed camera is (coeff + mu d) I; the device's inverse of it, observed
    through a solve with a unit right-hand side (fixed_block_solves), couples no two coordinates (exact zeros) and its
    diagonal is (1 / sqrt(x))^2, the form M = X^T X of k_fbsr_diag_inverse takes for a diagonal block -- at most one
    unit in the last place from the issue's 1 / x, which that kernel does not form; dp_a meets freepcg_ref's residual
    judge on the blocks read back, and is exactly 0 at every held coordinate"""
    rt, sm = composed_ref()
    rule = RULES[rule]
    nA, nC = rt.nA, rt.nC
    hs, hd = handle(rt, rule, SPARSE), handle(rt, rule)
    try:
        hs.linearize(1.0, 1.0)
        hd.linearize(1.0, 1.0)
        mu = mu_for(hd, rule)
        assert hs.max_diag() == hd.max_diag()
        D = hd.get_damping_diag() if rule.marquardt else np.ones(rt.nT)
        t = sparse_try(hs, mu)
        hd.schur_assemble(mu)
        S, ea, _ = read_system(hd, nA)
        fixed = fixed_block_solves(hs, rt, t, mu)
    finally:
        hs.close()
        hd.close()
    low = np.tril_indices(CNP)
    for (j, k), B in zip(t["jk"], t["val"]):
        want = S[CNP * j:CNP * j + CNP, CNP * k:CNP * k + CNP]
        assert bits_equal(B[low], want[low]) if j == k else bits_equal(B, want), f"block ({j}, {k}) differs"
    assert bits_equal(t["ea"], ea) and t["sc"].status == 0 and t["rc"] == 0
    j = int(rt.fixed_cams[0])
    blk = t["val"][np.flatnonzero((t["jk"][:, 0] == j) & (t["jk"][:, 1] == j))[0]]
    x = 1.0 + mu * D[CNP * j:CNP * j + CNP]
    assert np.array_equal(blk, np.diag(x)), "the block of the wholly fixed camera"
    for r, xr, got, alone in fixed:                                # the device's inverse of that block, through one solve
        assert alone, f"coordinate {r}: the inverse couples it to another coordinate"
        M = (1.0 / np.sqrt(xr)) * (1.0 / np.sqrt(xr))
        assert got == one_step(M, xr), f"coordinate {r}: x = {got!r}, M = (1 / sqrt(x))^2 gives {one_step(M, xr)!r}"
        print(f"coordinate {r}: the solve's x {got!r}; with M = 1 / x it would be {one_step(1.0 / xr, xr)!r}")
    assert np.all(t["dp"][:nA][rt.held] == 0.0) and np.all(t["dp"][nA + rt.held_b] == 0.0)
    case = f"sparse P54 composed {rule}"
    op = fp.ListOp(nC, t["jk"], t["val"], CNP)
    tr, gap = fp.list_relres_and_gap(op, t["dp"][:nA], t["ea"], t["iters"])
    note(case, "relres / tol", t["relres"] / TRY_TOL)
    note(case, "true relres / allowed", tr / (t["relres"] + fp.C_GAP * gap))
    assert t["relres"] <= TRY_TOL and tr <= t["relres"] + fp.C_GAP * gap
    r, bound = fr.dpb_residual(rt, sm, t["dp"], mu, rule)
    ratio, q = ar.excess(r, np.zeros(r.shape, LD), bound)
    note(case, "dp_b", ratio)
    assert ratio <= 1.0, f"point {q // 3} entry {q % 3}"


def test_two_sparse_runs_are_bit_identical():
    """case 5: wide_problem(65), the mixed table, Marquardt"""
    rt, _ = mixed_ref("wide-above")
    rule = RULES["marquardt"]
    runs = []
    for _ in range(2):
        h = handle(rt, rule, SPARSE)
        try:
            runs.append(snapshot(h, rule, SPARSE, iters=5))
        finally:
            h.close()
    assert_same(runs[0], runs[1], "two runs")


# ---- 6. the covariance ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", list(RULES))
def test_covariance_with_the_mixed_table(rule):
    """case 6: 7camsvarK, the mixed table, poses 0 and 2 held, dense solver, mu = 1e-6 of the largest diagonal entry:
    rows and columns of masked and held coordinates exactly 0 and sigma 0.0 there; the live part by
    freecov_ref.inverse_judge on the device's own S, the points by freecov_ref.point_judges on the device's own inputs"""
    rt, _ = mixed_ref("P7")
    rule = RULES[rule]
    scale = 2.5
    h = handle(rt, rule)
    try:
        h.linearize(1.0, 1.0)
        mu = mu_for(h, rule, 1e-6)
        assert h.free_covariance(mu, scale) == 0
        S, _, _ = read_system(h, rt.nA)
        C, P, sg = h.free_covariance_matrix(), h.free_point_covariance(), h.free_sigmas()
        V, Y = h.free_point_blocks()
    finally:
        h.close()
    src = fc.coord_map(rt)
    dead, live = src < 0, np.flatnonzero(src == np.arange(rt.nA))
    assert np.array_equal(np.flatnonzero(dead), rt.held) and dead[rt.held_table].all()
    assert np.array_equal(C, C.T) and np.all(C[dead] == 0.0) and np.all(C[:, dead] == 0.0)
    assert np.all(np.diag(C)[live] > 0.0)
    assert np.all(sg[rt.held_all] == 0.0) and np.all(sg[rt.free_all] > 0.0)
    assert np.array_equal(sg, np.sqrt(np.r_[np.diag(C), np.einsum("ikk->ik", P).reshape(-1)]))
    S = np.tril(S) + np.tril(S, -1).T
    dev, yard, allowed, kappa = fc.inverse_judge(S[np.ix_(live, live)], C[np.ix_(live, live)] / scale)
    print(f"n = {live.size}, kappa of the scaled S {kappa:.2e}, yardstick {yard:.2e}, device {dev:.2e}")
    note(f"covariance {rule}", "inverse", dev / allowed)
    assert dev <= allowed
    J = fc.point_judges(rt.i, rt.j, V, Y, C, mu, rule, scale, np.arange(rt.nP), CNP)
    worst = 0.0
    for q, (want, bound, want_ld) in J.items():
        worst = max(worst, ar.excess(P[q], want_ld, bound)[0])
    note(f"covariance {rule}", "points", worst)
    assert worst <= 1.0


# ---- 7. no table is no table ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", [DENSE, SPARSE], ids=["dense", "sparse"])
@pytest.mark.parametrize("rule", list(RULES))
def test_no_table_is_no_table(rule, solver):
    """case 7: a handle that never called the setter, one that set the mixed table, ran with it and then set NULL, and
    one that set all ones: bit-identical systems, D, dp, scalars and 10-iteration LM logs"""
    p, rule = prob("P7"), RULES[rule]
    runs = {}
    for which in ("never", "cleared", "ones"):
        h = open_handle(p, BAL, rule, solver)
        try:
            if which == "cleared":
                h.set_camera_masks(cm.mixed_table(p["nC"]))
                mixed = snapshot(h, rule, solver, iters=2)
                h.reset_params()
                h.set_camera_masks(None)
            elif which == "ones":
                h.set_camera_masks(np.ones((p["nC"], 10)))
            assert np.all(h.camera_masks() == 1)
            runs[which] = snapshot(h, rule, solver)
        finally:
            h.close()
    assert mixed["system"] != runs["never"]["system"]
    assert_same(runs["cleared"], runs["never"], "set and cleared")
    assert_same(runs["ones"], runs["never"], "all ones")


def full_try(h, mu):
    h.schur_assemble(mu)
    buf = h.get_reduce_buffer().tobytes()
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    return buf, h.get_dp().tobytes(), (sc.dp_l2, sc.gain_den, sc.newp_l2, sc.new_cost)


def test_the_look_ahead_with_the_table():
    """case 7: the sequence of test_gpu_held.py::test_the_look_ahead_with_holds with the mixed table (the free route's
    look-ahead has no switch of its own: the linearization queued ahead is held against a fresh psba_linearize): the
    try after the accepted look-ahead equals, bit for bit, that of a fresh handle set to the accepted parameters with
    the same table; the masked entries of the accepted parameters are the start's bits"""
    rt, _ = mixed_ref("wide-above")
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
        h.linearize(1.0, 1.0)                                       # (nothing left to do: it came with the accept)
        W1 = h.free_obs_blocks()[0]
        assert np.all(W1[:, :10, :][~rt.cam_free[rt.j]] == 0.0)
        got = full_try(h, mu)
        h2 = handle(rt, rule)
        h2.set_params(cams, pts)
        h2.linearize(1.0, 1.0)
        assert h2.get_damping_diag().tobytes() == D1.tobytes() and h2.free_obs_blocks()[0].tobytes() == W1.tobytes()
        assert full_try(h2, mu) == got
    finally:
        h.close()
        if h2 is not None:
            h2.close()


def test_a_table_set_between_two_levmar_calls():
    """case 7: psba_levmar, psba_reset_params, the table, psba_levmar gives the log of a fresh handle with the table"""
    rt, _ = mixed_ref("P7")
    logs = []
    for which in ("between", "fresh"):
        h = handle(rt, table=which == "fresh")
        try:
            if which == "between":
                _, plain = h.levmar(max_iter=10, tr_handoff=False, log_cap=256)
                h.reset_params()
                h.set_camera_masks(rt.table)
            _, log = h.levmar(max_iter=10, tr_handoff=False, log_cap=256)
            logs.append((log.tobytes(), tuple(x.tobytes() for x in h.get_params(0))))
        finally:
            h.close()
    assert logs[0] == logs[1] and len(logs[0][0]) > 0 and plain.tobytes() != logs[1][0]


# ---- 8. recovery ------------------------------------------------------------------------------------------------------------------

LM_ITERS = 30
# measured once on an MI355X: |device - twin| / twin of the final cost and of the three parameter errors
# max |f - f_true|, |k1 - k1_true|, |k2 - k2_true| over cameras 1, 3 and 5, per solver.  The bound is four times the
# measurement, the margin of LM_GAP in test_gpu_free_sparse.py: two correct LM runs differ by rounding that the twin's
# single run does not span
RING_GAP = {
    "dense": {"cost": 1.702e-07, "f": 3.053e-07, "k1": 1.094e-07, "k2": 3.026e-07},
    "sparse": {"cost": 7.296e-07, "f": 3.053e-07, "k1": 6.988e-08, "k2": 1.625e-07},
}


@functools.lru_cache(maxsize=None)
def ring_twin():
    start, kc0, poses, table, K_true, kc_true = cm.mixed_ring()
    t = cm.CamMaskTwin(start, table, kc0, fr.ALL, poses)
    res, _ = t.levmar(max_iter=LM_ITERS)
    return start, kc0, poses, table, K_true, kc_true, res, ring_errors(t.cams, K_true, kc_true)


def ring_errors(cams, K_true, kc_true):
    free = list(cm.RING_FREE_CAMS)
    return {"f": float(np.abs(cams[free, 0] - K_true[free, 0]).max()), "k1": float(np.abs(cams[free, 5] - kc_true[free, 0]).max()),
            "k2": float(np.abs(cams[free, 6] - kc_true[free, 1]).max())}


def ring_run(solver):
    """(the device's LM result, its start and final cameras) on the mixed ring"""
    start, kc0, poses, table = ring_twin()[:4]
    h = open_handle(start, fr.ALL, solver=solver, kc=kc0)
    try:
        h.set_camera_masks(table)
        h.set_held(poses, None)
        c0, _ = h.get_params(0)
        res, _ = h.levmar(max_iter=LM_ITERS, tr_handoff=False, log_cap=256)
        return res, c0, h.get_params(0)[0]
    finally:
        h.close()


def ring_gaps(solver):
    _, _, _, _, K_true, kc_true, want, werr = ring_twin()
    res, c0, c1 = ring_run(solver)
    err = ring_errors(c1, K_true, kc_true)
    gaps = {"cost": abs(res.final_err - want.final_err) / want.final_err}
    gaps.update({k: abs(err[k] - werr[k]) / werr[k] for k in err})
    return res, c0, c1, want, gaps


@pytest.mark.parametrize("solver", ["dense", "sparse"])
def test_recovery_of_the_mixed_ring(solver):
    """case 8: held_ring (poses 0 and 1 held); cameras 0, 2, 4 start at their true K and kc with the row none, cameras 1,
    3, 5 from the scene's start with {f, k1, k2}.  The same stop reason as the twin within 30 iterations, the intrinsics
    of cameras 0, 2 and 4 unchanged to the bit, and the four gaps within four times their measured values"""
    res, c0, c1, want, gaps = ring_gaps(SPARSE if solver == "sparse" else DENSE)
    print(f"{solver}: iterations {res.iters} flag {res.flag} (twin {want.iters}, {want.flag}), cost {res.final_err:.3e} "
          f"(twin {want.final_err:.3e}); gaps " + ", ".join(f"{k} {v:.3e}" for k, v in gaps.items()))
    assert want.flag == 3 and want.iters == 18
    assert res.flag == TWIN_FLAG[want.flag] and res.iters <= LM_ITERS
    fixed = list(cm.RING_FIXED_CAMS)
    assert c1[fixed, :10].tobytes() == c0[fixed, :10].tobytes() and c1[:2, 10:].tobytes() == c0[:2, 10:].tobytes()
    assert np.all(c1[list(cm.RING_FREE_CAMS), 0] != c0[list(cm.RING_FREE_CAMS), 0])
    for k, v in gaps.items():
        note(f"ring {solver}", f"gap {k} / (4 x measured)", v / (4.0 * RING_GAP[solver][k]))
        assert v <= 4.0 * RING_GAP[solver][k], f"{solver}: gap of {k} {v:.3e}, measured {RING_GAP[solver][k]:.3e}"


# ---- 9. the interface ---------------------------------------------------------------------------------------------------------------

def test_interface():
    """case 9"""
    import psba_amd
    from psba_amd import capi
    p = prob("P7")
    nC = int(p["nC"])
    table = cm.mixed_table(nC)

    def refused(call, code, *words):
        with pytest.raises(psba_amd.PsbaError) as ei:
            call()
        assert ei.value.code == code, str(ei.value)
        for w in words:
            assert w in str(ei.value), str(ei.value)
    h = psba_amd.Psba(0)
    try:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        refused(lambda: h.set_camera_masks(None), E_STATE, "no problem uploaded")       # before an upload
        refused(lambda: h.set_camera_masks(table), E_STATE, "no problem uploaded")
        assert capi.lib.psba_camera_masks(h._h, None) == E_STATE
        h.upload_problem(p)
        h.set_distortion(start_kc(nC))
        assert np.all(h.camera_masks() == 1) and h.camera_masks().shape == (nC, 10) and h.camera_masks().dtype == np.uint8
        h.set_camera_masks(table)                                   # the getter round-trips
        assert np.array_equal(h.camera_masks(), table)
        h.set_camera_masks(table * 7)                               # non-zero = optimised
        assert np.array_equal(h.camera_masks(), table)
        assert capi.lib.psba_camera_masks(h._h, None) == 0
        h.set_intrinsics_mask(BAL)                                  # the global flags are their own
        assert h.intrinsics_mask() == BAL and np.array_equal(h.camera_masks(), table)
        h.set_intrinsics_mask(None)
        refused(lambda: h.set_camera_masks(table[:3]), E_INVALID, "flags for 7 cameras")  # a wrong size: nothing changes
        assert np.array_equal(h.camera_masks(), table)
        h.set_camera_masks(np.ones((nC, 10)))                       # no zero entry is no table
        assert np.all(h.camera_masks() == 1)
        h.set_camera_masks(table)
        # setting the table discards what was derived: the two test hooks and the assembled system
        h.set_damping(psba_amd.DAMPING_MARQUARDT)
        h.linearize(1.0, 1.0)
        h.free_obs_blocks()
        h.get_damping_diag()
        h.set_camera_masks(table)
        for call in (h.free_obs_blocks, h.get_damping_diag, lambda: h.schur_assemble(1e-3)):
            refused(call, E_STATE)
        h.linearize(1.0, 1.0)
        mu = 1e-3
        before = full_try(h, mu)
        h.schur_assemble(mu)
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        refused(lambda: h.set_camera_masks(None), E_STATE, "in flight")   # a try is in flight: refused, nothing changes
        assert capi.lib.psba_camera_masks(h._h, None) == 0          # (the getter runs at any time)
        assert np.array_equal(h.camera_masks(), table)
        assert h.backsub_wait().status == 0
        assert full_try(h, mu) == before                            # a refused call leaves the next try's bits unchanged
        h.schur_assemble(mu)
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        assert h.backsub_wait().status == 0
        h.set_camera_masks(table)                                   # ... discards the linearization queued ahead
        h.accept()
        for call in (h.free_obs_blocks, h.get_damping_diag, lambda: h.schur_assemble(mu)):
            refused(call, E_STATE)
        h.upload_problem(p)                                         # an upload resets the table
        assert np.all(h.camera_masks() == 1)
    finally:
        h.close()
    # blocks of 11 and six-parameter blocks refuse both verbs; the text says that blocks of 11 have no mask
    for model in (psba_amd.CAMERA_FREE_K, psba_amd.CAMERA_FIXED_K):
        ho = open_handle(p, model=model)
        try:
            refused(lambda: ho.set_camera_masks(table), E_STATE, "PSBA_CAMERA_FREE_KD only", "blocks of 11", "have no mask")
            refused(lambda: ho.set_camera_masks(None), E_STATE, "PSBA_CAMERA_FREE_KD only")
            refused(ho.camera_masks, E_STATE, "PSBA_CAMERA_FREE_KD only")
        finally:
            ho.close()
