"""PSBA_SOLVER_SPARSE under PSBA_CAMERA_FREE_K (camera blocks of 11) and PSBA_CAMERA_FREE_KD (blocks of 16, masks ALL
and BAL) on the GPU: the block-sparse S of kernels_free_pcg.hip and its conjugate gradients.  Needs an
MI355X.  tests/freepcg_ref.py holds the references and derives every constant; tests/free_ref.py the judges of one try.

  a  the mode: uploads under both models, psba_schur_path = 6, the dense verbs refuse with the solver's name,
     PSBA_SOLVER_PCG still fails at the upload, and with six-parameter blocks PSBA_SOLVER_SPARSE is PSBA_SOLVER_PCG.
  b  one damping try entry by entry (the inputs and dampings of test_gpu_free_entrywise.py; Marquardt on P54 and
     wide-above): the block list, every stored block and e_a by C1's scaled measure, the exact parts, dp_a by its true
     relative residual in long double, dp_b and the four scalars by free_ref's C3 / C4 judges.
  c  constructed systems through psba_set_sparse_S on pcg_ref's patterns and on `trip` (walked rows of 3 .. 9 blocks:
     both sides of one and two trips of the product kernel's FSPMV_TRIP = 4 blocks): the product bound, NaN in the strict
     upper triangles, block-diagonal systems, the stop rule at iterations 7, 8, 9, 16, 17.
  d  the failure protocol: a bad pivot, an indefinite S, NaN, a budget of 3 -- and a good solve after each.
  e  fixed order: two assemble + solve runs are bit-identical on wide-above, on 512 / 513 cameras (the product's grid
     stops growing at FPCG_CAP = 128 workgroups of four block rows: 513 cameras take a second trip, and the partial sums
     of p.Sp stay at 128), on 2048 / 2050 cameras of 16 and 2978 / 2979 of 11 (the vector kernels' grid stops growing at
     128 workgroups of 256 unknowns: 32 768).
  f  read-before-write: the try of P54 and wide-above in a process started with PSBA_DEBUG_POISON=1 gives the same bits.
  g  psba_levmar against the dense solver on P54 and the ring scene with two poses held.
  h  size: the band scene of 2050 cameras of 16 (nA = 32 800).
The module prints the worst found / allowed per quantity."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import freepcg_ref as fp
import held_ref as hr
import pcg_ref as pr
import test_gpu_free_entrywise as fe
from freekd_twin import start_kc, wide_problem
from test_freekd_twin import P54, scaled_tol

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

PSBA_OK, PSBA_NOT_SPD, PSBA_PCG_MAXIT, PSBA_E_STATE = 0, 1, 4, -6
ROUTES = fe.ROUTES
TRY_TOL = 1e-12
WORST = {}
# g: |cost(sparse) - cost(dense)| / cost(dense) after the same psba_levmar, measured on an MI355X; the bound
# is four times the measurement (the solve is deterministic: the margin is for another compiler) and never above 1e-6
LM_GAP = {("fk", "P54"): 1.688e-11, ("kd-bal", "P54"): 3.765e-12, ("kd-bal", "ring"): 6.291e-15, ("fk", "ring"): 6.405e-10}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for c in _CONSTRUCTED.values():
        c.close()
    _CONSTRUCTED.clear()
    if WORST:
        print("\nworst found / allowed per case and quantity:")
        for key in sorted({k[0] for k in WORST}):
            print(f"  {key}: " + ", ".join(f"{q} {v:.2e}" for (kk, q), v in WORST.items() if kk == key))


def note(case, what, ratio):
    WORST[(case, what)] = max(WORST.get((case, what), 0.0), float(ratio))
    print(f"{case} {what}: {float(ratio):.3e}")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def open_handle(p, route, solver, tol=TRY_TOL, max_iter=500, rule=fr.NO_RULE, kc=None):
    import psba_amd
    cnp, free = ROUTES[route]
    h = psba_amd.Psba(0)
    if solver:
        h.set_solver(solver, tol=tol, max_iter=max_iter)
    if cnp == 16:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        h.upload_problem(p)
        h.set_distortion(start_kc(p["nC"]) if kc is None else kc)
        h.set_intrinsics_mask(free)
    else:
        h.set_camera_model(psba_amd.CAMERA_FREE_K)
        h.upload_problem(p)
    assert h.camera_block() == cnp and h.schur_path() == (6 if solver == 2 else 5)
    if rule.marquardt:
        h.set_damping(rule.kind, rule.dmin, rule.dmax)
    return h


# ---- a. the mode ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["fk", "kd-all"])
def test_mode_and_refusals(route):
    import psba_amd
    from psba_amd.capi import PsbaError
    cnp, _ = ROUTES[route]
    p = fe.prob("tiny")
    h = open_handle(p, route, psba_amd.SOLVER_SPARSE)
    try:
        assert h.pcg_info()[2:] == (3, 3)
        h.linearize(1.0, 1.0)
        h.schur_assemble(1.0)
        buf = np.zeros(h.reduce_buffer_size())
        verbs = {
            "psba_SPDinv_matVec": h.SPDinv_matVec,
            "psba_set_reduce_buffer": lambda: h.set_reduce_buffer(buf),
            "psba_get_reduce_buffer": h.get_reduce_buffer,
            "psba_chol_dist_begin": h.chol_dist_begin,
            "psba_chol_dist_superpanel": lambda: h.chol_dist_superpanel(0),
            "psba_chol_dist_block (get)": lambda: h.chol_dist_get_block(0),
            "psba_chol_dist_block (set)": lambda: h.chol_dist_set_block(0, buf),
            "psba_chol_dist_finish": h.chol_dist_finish,
            "psba_get_cholmod_factor": h.cholmod_factor,
            "psba_free_covariance_compute": lambda: h.free_covariance(mu=1.0),
            "psba_free_covariance_compute (reassemble = 0)": lambda: h.free_covariance(mu=1.0, reassemble=False),
            "psba_get_free_camera_covariance": h.free_camera_covariance,
            "psba_get_free_covariance_matrix": h.free_covariance_matrix,
            "psba_get_free_point_covariance": h.free_point_covariance,
            "psba_get_free_sigmas": h.free_sigmas,
            "psba_free_covariance_times": h.free_covariance_times,
        }
        if cnp == 16:
            verbs["psba_set_intrinsics_groups"] = lambda: h.set_intrinsics_groups(np.zeros(p["nC"], dtype=np.int32))
        for verb, call in verbs.items():
            with pytest.raises(PsbaError) as e:
                call()
            assert e.value.code == PSBA_E_STATE, f"{verb}: {e.value}"
            assert "PSBA_SOLVER_SPARSE" in str(e.value), f"{verb} refused without naming the solver: {e.value}"
        assert h.schur_solve() == PSBA_OK and h.backsub(1.0).status == 0      # the refusals changed nothing
    finally:
        h.close()
    hp = psba_amd.Psba(0)                                                      # PSBA_SOLVER_PCG stays refused
    hp.set_camera_model(psba_amd.CAMERA_FREE_KD if cnp == 16 else psba_amd.CAMERA_FREE_K)
    hp.set_solver(psba_amd.SOLVER_PCG)
    with pytest.raises(PsbaError):
        hp.upload_problem(p)
    hp.set_solver(psba_amd.SOLVER_SPARSE)                                      # ... and the same handle may still ask for this one
    hp.upload_problem(p)
    assert hp.schur_path() == 6
    with pytest.raises(PsbaError):
        hp.set_solver(psba_amd.SOLVER_DENSE)                                   # not after the upload
    hp.close()


def test_six_parameter_blocks_take_the_pcg_route():
    import psba_amd
    n, blocks = pr.pattern("five")
    prob = pr.pattern_problem(n, blocks)
    out = []
    for solver in (psba_amd.SOLVER_PCG, psba_amd.SOLVER_SPARSE):
        h = psba_amd.Psba(0)
        h.set_solver(solver, tol=1e-10, max_iter=100)
        h.upload_problem(prob)
        assert h.schur_path() == 4
        h.linearize(1.0, 1.0)
        h.schur_assemble(1e-3 * h.max_diag())
        out.append(h.get_sparse_S())
        h.close()
    for a, b in zip(*out):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- b. one try, entry by entry ------------------------------------------------------------------------------------

def run_try(h, mu):
    """One assemble + solve + back-substitution: dict of everything the device returned."""
    h.schur_assemble(mu)
    jk, val, ea = h.get_sparse_S()
    h.schur_reduce()
    rc = h.schur_solve()
    iters, relres, nblk, _ = h.pcg_info()
    sc = h.backsub(mu)
    return dict(jk=jk, val=val, ea=ea, rc=rc, iters=iters, relres=relres, nblk=nblk, sc=sc, dp=h.get_dp(),
                scal=np.array([sc.status, sc.dp_l2, sc.gain_den, sc.new_cost, sc.newp_l2]))


def same_bits(a, b):
    return (a["jk"].tobytes() == b["jk"].tobytes() and bits_equal(a["val"], b["val"]) and bits_equal(a["ea"], b["ea"]) and
            bits_equal(a["dp"], b["dp"]) and (a["rc"], a["iters"]) == (b["rc"], b["iters"]) and
            bits_equal([a["relres"]], [b["relres"]]) and bits_equal(a["scal"], b["scal"]))


def judge_dpa(case, op, t):
    """relres_reported <= tol and the true relative residual (long double, from the blocks read back) within
    relres_reported + C_gap gap_unit"""
    nA = op.n_cams * op.c
    tr, gap = fp.list_relres_and_gap(op, t["dp"][:nA], t["ea"], t["iters"])
    note(case, "relres / tol", t["relres"] / TRY_TOL)
    note(case, "true relres / allowed", tr / (t["relres"] + fp.C_GAP * gap))
    assert t["rc"] == PSBA_OK and t["relres"] <= TRY_TOL, f"{case}: rc {t['rc']}, relres {t['relres']:.3e} after {t['iters']}"
    assert tr <= t["relres"] + fp.C_GAP * gap, f"{case}: true relres {tr:.6e}, reported {t['relres']:.6e}, gap unit {gap:.3e}"


def one_try(route, name, which_mu, rule=fr.NO_RULE):
    rt, sm = fe.ref(name, route)
    cnp, nA, nC = rt.cnp, rt.nA, rt.nC
    mus, diag = fe.dampings(rt, sm)
    mu, cost = (fe.MQ_MUS if rule.marquardt else mus)[which_mu], sm["cost"]
    tol = scaled_tol(rt.p)
    case = f"{route} {name} {which_mu}" + (f" {rule}" if rule.marquardt else "")
    h = open_handle(rt.p, route, 2, rule=rule)
    D = None
    try:
        assert abs(h.residual() - cost) <= 1e-12 * cost
        h.linearize(1.0, 1.0)
        if rule.marquardt:
            D = h.get_damping_diag()
        t = run_try(h, mu)
        # the block list: the co-visibility pattern plus every diagonal, ascending
        want_jk = fp.rows_enumeration(nC, rt.p["iidx"], rt.p["jidx"])["jk"]
        assert np.array_equal(t["jk"], want_jk) and t["nblk"] == len(want_jk)
        # every stored block and e_a (C1's scaled measure; outside the list the reference is exactly zero)
        S = fp.dense_of(nC, t["jk"], t["val"], cnp)
        ea = t["ea"]
        S_want, ea_want = fe.schur_ref(name, route, mu, rule)
        d = fr.scale_diag(rt, sm, mu, rule) if rule.marquardt else np.sqrt(diag[:nA] + mu)
        eS = (np.abs(S - S_want) / np.outer(d, d)).max()
        ee = (np.abs(ea - ea_want) / (d * np.sqrt(cost))).max()
        note(case, "S", eS / tol)
        note(case, "e_a", ee / tol)
        assert eS <= tol and ee <= tol, f"{case}: scaled S {eS:.3e}, e_a {ee:.3e}, tol {tol:.3e}"
        # the exact parts: held coordinates, the camera without observations
        held = rt.held
        empty = np.flatnonzero(np.bincount(rt.j, minlength=nC) == 0)
        if rule.marquardt:
            assert np.array_equal(fr.check_exact_parts(rt, S, ea, mu, rule), empty)
        else:
            off = S[held].copy()
            off[np.arange(held.size), held] = 0.0
            assert np.all(off == 0.0) and np.all(S[held, held] == 1.0 + mu) and np.all(ea[held] == 0.0)
            for j in empty:
                rows = np.arange(cnp * j, cnp * j + cnp)
                want = mu * np.eye(cnp)
                hj = held[(held >= rows[0]) & (held <= rows[-1])] - rows[0]
                want[hj, hj] = 1.0 + mu
                blk = t["val"][np.flatnonzero((t["jk"][:, 0] == j) & (t["jk"][:, 1] == j))[0]]
                assert np.array_equal(blk, want)                     # written whole, both triangles
                assert np.all(np.delete(S[rows], rows, axis=1) == 0.0)
        assert t["sc"].status == 0
        dp = t["dp"]
        assert np.all(dp[:nA][held] == 0.0)
        for j in empty:
            assert np.all(ea[cnp * j:cnp * j + cnp] == 0.0) and np.all(dp[cnp * j:cnp * j + cnp] == 0.0)
        judge_dpa(case, fp.ListOp(nC, t["jk"], t["val"], cnp), t)
        # dp_b and the four scalars from the device's own dp_a (free_ref's C3 / C4)
        r, bound = fr.dpb_residual(rt, sm, dp, mu, rule)
        ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), bound)
        note(case, "dp_b", ratio)
        assert ratio <= 1.0, f"{case}: point {k // 3} entry {k % 3}: residual {float(r[k]):.3e} > bound {bound[k]:.3e}"
        newcams, newpts = h.get_params(1)
        sc = t["sc"]
        got = dict(dp_l2=sc.dp_l2, gain_den=sc.gain_den, newp_l2=sc.newp_l2, new_cost=sc.new_cost)
        bad = []
        for what, (x, b) in fr.scalars(rt, sm, dp, newcams, newpts, mu, D=D).items():
            ratio = float(abs(ar.LD(got[what]) - x) / b)
            note(case, what, ratio)
            if not ratio <= 1.0:
                bad.append(f"{what} = {got[what]!r}, exact {float(x)!r}, bound {b:.3e}")
        assert not bad, f"{case}: " + "; ".join(bad)
        return t
    finally:
        h.close()


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name", fe.INPUTS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_one_damping_try_entrywise(route, name, which_mu):
    one_try(route, name, which_mu)


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name", ["P54", "wide-above"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_one_damping_try_entrywise_marquardt(route, name, which_mu):
    one_try(route, name, which_mu, fe.MQ["default"])


@pytest.mark.parametrize("marquardt", [False, True])
@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_settings_compose_and_the_blocks_are_the_dense_routes_bits(route, marquardt):
    """Held poses and a held point, priors on cameras and points, a Huber loss with sigmas (and Marquardt's rule) on P54:
    they change only what the linearization stores, so the list holds the bits the dense route puts into the same
    places of its square (the same products in the same order, + U, + mu), e_a is the dense route's, and the solve
    meets its residual bound; held coordinates of dp_a are exactly zero."""
    import psba_amd
    p = fe.prob("P54")
    cnp = ROUTES[route][0]
    nC, nP, nA = p["nC"], p["nP"], cnp * p["nC"]
    rng = np.random.default_rng(3)
    poses, pts = np.zeros(nC, dtype=np.uint8), np.zeros(nP, dtype=np.uint8)
    poses[[0, 7]] = 1
    pts[5] = 1
    sigma = rng.uniform(0.5, 2.0, p["nO"])
    out = []
    for solver in (2, 0):
        h = open_handle(p, route, solver, rule=fe.MQ["default"] if marquardt else fr.NO_RULE)
        try:
            cams, pts0 = h.get_params(0)
            h.set_held(poses, pts)
            h.set_priors(cams * (1.0 + 1e-3), np.full((nC, cnp), 1e-2), pts0 + 1e-3, np.full((nP, 3), 1e-1))
            h.set_obs_weighting(psba_amd.LOSS_HUBER, 2.0, sigma)
            h.linearize(1.0, 1.0)
            mu = 1e-3 if marquardt else 1e-3 * h.max_diag()
            if solver:
                out.append(run_try(h, mu))
            else:
                h.schur_assemble(mu)
                out.append(fe.read_system(h, nA)[:2])
        finally:
            h.close()
    t, (S, ea) = out
    low = np.tril_indices(cnp)
    for (j, k), B in zip(t["jk"], t["val"]):
        want = S[cnp * j:cnp * j + cnp, cnp * k:cnp * k + cnp]
        assert bits_equal(B[low], want[low]) if j == k else bits_equal(B, want), f"{route}: block ({j}, {k}) differs"
    assert bits_equal(t["ea"], ea) and t["sc"].status == 0
    for j in np.flatnonzero(poses):
        assert np.all(t["dp"][cnp * j + cnp - 6:cnp * j + cnp] == 0.0)
    assert np.all(t["dp"][nA + 15:nA + 18] == 0.0)
    judge_dpa(f"{route} P54 composed" + (" marquardt" if marquardt else ""), fp.ListOp(nC, t["jk"], t["val"], cnp), t)


# ---- c. constructed systems ----------------------------------------------------------------------------------------

MU = 1.0  # of psba_schur_assemble and psba_backsub: plays no part, the blocks are overwritten
C_NAMES = ["one", "two", "five", "hubs", "trip", "band43", "arrow257", "arrow260"]
C_ROUTES = ["fk", "kd-all"]
_CONSTRUCTED = {}


class Constructed:
    """A PSBA_SOLVER_SPARSE handle on the pattern problem of a named pattern, linearized once."""

    def __init__(self, name, route):
        self.name, self.route, self.c = name, route, ROUTES[route][0]
        self.n_cams, self.blocks = fp.fpattern(name)
        self.nA = self.c * self.n_cams
        self.h = open_handle(fp.pattern_problem(self.n_cams, self.blocks), route, 2, tol=fp.TOL, max_iter=fp.MAXIT)
        self.h.linearize(1.0, 1.0)
        self.h.schur_assemble(MU)
        self.jk = self.h.get_sparse_S()[0]
        want = sorted([(j, j) for j in range(self.n_cams)] + list(self.blocks))
        assert list(map(tuple, self.jk.tolist())) == want, f"{name}: the handle's block list is not the pattern"
        self.m = fp.entry_row_lengths(self.n_cams, self.blocks, self.c)

    def load(self, S, b, poison=False, val=None):
        self.h.schur_assemble(MU)
        if val is None:
            val = fp.blocks_of(S, self.jk, self.c)
        if poison:
            val = fp.poison_upper(val, self.jk, self.c)
        self.h.set_sparse_S(val, b)

    def solve(self, S, b, tol=fp.TOL, max_iter=fp.MAXIT, poison=False, val=None):
        """-> (rc of psba_schur_solve, x, iters, relres, PSBA_NOT_SPD bit of the try)"""
        self.h.set_solver(2, tol=tol, max_iter=max_iter)
        self.load(S, b, poison, val)
        rc = self.h.schur_solve()
        x = self.h.get_dp()[:self.nA].copy()
        iters, relres, _, _ = self.h.pcg_info()
        return rc, x, iters, relres, self.h.backsub(MU).status & PSBA_NOT_SPD

    def good(self, what):
        """The first system of the quality sweep on this handle: converged, and the true residual within the gap."""
        sy = fp.quality_system(self.name, *fp.QUALITY[0], self.c)
        rc, x, iters, relres, bad = self.solve(sy["S"], sy["b"])
        tag = f"{self.route} {self.name} {what}"
        assert rc == PSBA_OK and not bad and np.all(np.isfinite(x)) and relres <= fp.TOL, f"{tag}: rc {rc}, relres {relres}"
        gap = fp.C_GAP * fp.gap_unit(sy["S"], x, sy["b"], iters)
        tr = fp.true_relres(sy["S"], x, sy["b"])
        note(f"{self.route} {self.name}", "residual gap / allowed", abs(tr - relres) / gap)
        assert abs(tr - relres) <= gap, f"{tag}: true relres {tr:.6e}, reported {relres:.6e}, gap allowed {gap:.3e}"
        n64 = sy["t64"]["iters"]
        assert iters <= n64 + 2, f"{tag}: {iters} iterations, the float64 twin {n64}"
        return x

    def close(self):
        self.h.close()


def constructed(name, route):
    if (name, route) not in _CONSTRUCTED:
        _CONSTRUCTED[(name, route)] = Constructed(name, route)
    return _CONSTRUCTED[(name, route)]


@pytest.mark.parametrize("name", C_NAMES)
@pytest.mark.parametrize("route", C_ROUTES)
def test_product_entry_by_entry(route, name):
    c = constructed(name, route)
    S = fp.dominant(c.n_cams, c.blocks, 1e-2, c.c, 2.0, 2)
    b = np.zeros(c.nA)
    c.load(S, b)
    ys = []
    for what, x in fp.product_vectors(c.n_cams, c.c):
        y = c.h.sparse_S_times(x)
        err = np.abs(y.astype(fp.LD) - fp.spmv_exact(S, x)).astype(np.float64)
        bound = fp.spmv_bound(S, x, c.m, c.c)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        note(f"{route} {name}", "product / bound", ratio.max())
        i = int(np.argmax(ratio))
        assert ratio[i] <= 1.0, (f"{route} {name}, x = {what}: y[{i}] (camera {i // c.c}, row {i % c.c}, {c.m[i]} blocks in "
                                 f"its row) = {y[i]:.17e}, off by {err[i]:.3e}, bound {bound[i]:.3e}")
        ys.append(y)
    c.load(S, b, poison=True)  # NaN in the strict upper triangle of every diagonal block: never read
    for (what, x), y in zip(fp.product_vectors(c.n_cams, c.c), ys):
        assert bits_equal(c.h.sparse_S_times(x), y), f"{route} {name}, x = {what}: the poisoned product differs"
    x0 = c.good("after psba_sparse_S_times")
    sy = fp.quality_system(name, *fp.QUALITY[0], c.c)
    again = c.solve(sy["S"], sy["b"])
    poisoned = c.solve(sy["S"], sy["b"], poison=True)
    assert bits_equal(again[1], x0) and bits_equal(poisoned[1], x0) and again[2:4] == poisoned[2:4]


@pytest.mark.parametrize("name", ["five", "band43", "arrow257"])
@pytest.mark.parametrize("grade", [0.0, 5.0])
@pytest.mark.parametrize("route", C_ROUTES)
def test_block_inverse_solves_block_diagonal_systems_in_one_iteration(route, name, grade):
    c = constructed(name, route)
    case = fp.blockdiag_case(name, grade, c.c)
    rc, x, iters, relres, bad = c.solve(case["S"], case["b"], tol=1e-10, poison=True)
    assert rc == PSBA_OK and not bad and np.all(np.isfinite(x))
    assert iters == 1, f"{name} grade {grade}: {iters} iterations on a block-diagonal system (relres {relres:.3e})"
    ratio = fp.blockdiag_ratios(case, x) / fp.C_INV[c.c]
    note(f"{route} {name}", "block inverse / bound", ratio.max())
    j = int(np.argmax(ratio))
    assert ratio[j] <= 1.0, (f"{route} {name} grade {grade}: camera {j} (kappa {case['kap'][j]:.1f}) is {ratio[j]:.2f} x "
                             f"C_inv kappa eps away from the block solve")


@pytest.mark.parametrize("k", fp.BURST_EDGES)
@pytest.mark.parametrize("route", C_ROUTES)
def test_stop_at_chosen_iteration(route, k):
    c = constructed("band43", route)
    case = fp.burst_case("band43", k, c.c)
    assert case is not None
    tol = case["tol"]
    rc, x, iters, relres, bad = c.solve(case["S"], case["b"], tol=tol)
    print(f"\n{route} k = {k}: delta {case['delta']:.4g}, tol {tol:.3e}, twin {case['hist'][k - 1]:.3e} -> "
          f"{case['hist'][k]:.3e}; iters {iters}, relres {relres:.3e}")
    assert rc == PSBA_OK and not bad
    assert iters == k, f"{route}: stopped after {iters} iterations, the long-double twin after {k}"
    assert relres <= tol
    rc2, _, iters2, relres2, _ = c.solve(case["S"], case["b"], tol=tol, max_iter=k)
    assert rc2 == PSBA_OK and iters2 == k and relres2 <= tol, f"max_iter = {k}: rc {rc2}, {iters2}, {relres2:.3e}"
    rc3, _, iters3, relres3, bad3 = c.solve(case["S"], case["b"], tol=tol, max_iter=k - 1)
    assert rc3 == PSBA_PCG_MAXIT and not bad3, f"max_iter = {k - 1}: rc {rc3}"
    assert iters3 == k - 1 and relres3 > tol
    assert abs(relres3 - case["hist"][k - 1]) <= 1e-3 * case["hist"][k - 1] + 1e-15


# ---- d. failures are reported and forgotten ------------------------------------------------------------------------

def expect_failure(c, what, S, b, val=None):
    rc, x, iters, relres, bad = c.solve(S, b, val=val)
    assert rc != PSBA_PCG_MAXIT and iters < fp.MAXIT, f"{c.route} {c.name} {what}: ran its budget out ({iters} iterations)"
    assert bad, f"{c.route} {c.name} {what}: passed for a solve (rc {rc}, {iters} iterations, relres {relres})"
    c.good(f"after {what}")


@pytest.mark.parametrize("name", ["five", "band43"])
@pytest.mark.parametrize("route", C_ROUTES)
def test_failure_protocol(route, name):
    c = constructed(name, route)
    sy = fp.quality_system(name, *fp.QUALITY[0], c.c)
    b = sy["b"]
    for j, col in ((0, 0), (c.n_cams // 2, c.c - 1), (c.n_cams - 1, c.c // 2)):
        expect_failure(c, f"bad pivot {col} of diagonal block {j}", fp.bad_diag(c.n_cams, c.blocks, j, col, c.c), b)
    for which in ("first", "middle", "last"):
        S, pair = fp.indefinite_pd_diag(c.n_cams, c.blocks, which, c.c)
        expect_failure(c, f"indefinite on the {which} pair {pair}", S, b)
    val = fp.blocks_of(sy["S"], c.jk, c.c)
    off = [i for i, (j, k) in enumerate(c.jk) if j != k]
    diag = [i for i, (j, k) in enumerate(c.jk) if j == k]
    v = val.copy()
    v[off[len(off) // 2], 2, c.c - 1] = np.nan
    expect_failure(c, "NaN in an off-diagonal block", None, b, val=v)
    v = val.copy()
    v[diag[len(diag) // 2], c.c - 1, 1] = np.nan
    expect_failure(c, "NaN in the lower triangle of a diagonal block", None, b, val=v)
    bn = b.copy()
    bn[c.nA // 2] = np.nan
    expect_failure(c, "NaN in e_a", None, bn, val=val)
    if name == "band43":
        rc, x, iters, relres, bad = c.solve(sy["S"], b, max_iter=3)
        assert rc == PSBA_PCG_MAXIT and not bad and iters == 3 and relres > fp.TOL and np.all(np.isfinite(x))
        c.good("after a budget of 3")


# ---- e. fixed order --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def big_problem(kind, nC):
    return wide_problem(nC, nP=max(240, 2 * nC)) if kind == "wide" else fp.band_scene(nC)


def two_runs(p, route, mu_rel=1e-3):
    """(first, second) run_try on one handle, with the handle's own true residual check"""
    h = open_handle(p, route, 2)
    try:
        h.linearize(1.0, 1.0)
        mu = mu_rel * h.max_diag()
        return run_try(h, mu), run_try(h, mu), mu
    finally:
        h.close()


FIXED = [("fk", "wide", 94), ("kd-bal", "wide", 65), ("fk", "wide", 512), ("fk", "wide", 513), ("kd-all", "wide", 512),
         ("kd-all", "wide", 513), ("kd-bal", "band", 2048), ("kd-bal", "band", 2050), ("fk", "band", 2978),
         ("fk", "band", 2979)]


@pytest.mark.parametrize("route,kind,nC", FIXED)
def test_two_runs_are_bit_identical(route, kind, nC):
    cnp = ROUTES[route][0]
    assert (nC > 512) == ((nC + 3) // 4 > 128) and (cnp * nC > 32768) == ((cnp * nC + 255) // 256 > 128)
    a, b, _ = two_runs(big_problem(kind, nC), route)
    assert a["sc"].status == 0 and a["iters"] > 0
    assert same_bits(a, b), f"{route} {kind} {nC}: iterations {a['iters']} / {b['iters']}, relres {a['relres']!r} / {b['relres']!r}"
    judge_dpa(f"{route} {kind}{nC}", fp.ListOp(nC, a["jk"], a["val"], cnp), a)


# ---- f. read-before-write ---------------------------------------------------------------------------------------------

POISON_CASES = [("fk", "P54"), ("kd-bal", "P54"), ("fk", "wide-above"), ("kd-all", "wide-above")]


def poison_worker(out):
    """(in a process of its own, started with PSBA_DEBUG_POISON=1) the tries of POISON_CASES into an .npz"""
    res = {}
    for route, name in POISON_CASES:
        a, _, mu = two_runs(fe.prob(name, ROUTES[route][0]), route)
        for k in ("jk", "val", "ea", "dp", "scal"):
            res[f"{route}|{name}|{k}"] = a[k]
        res[f"{route}|{name}|info"] = np.array([a["rc"], a["iters"], a["relres"], mu])
    np.savez(out, **res)


def test_poisoned_allocations_give_the_same_bits(tmp_path):
    """The handle reads PSBA_DEBUG_POISON once per process, so the poisoned run is a child process: that is what this
    test is about."""
    out = str(tmp_path / "poisoned.npz")
    env = dict(os.environ, PSBA_DEBUG_POISON="1")
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; " \
           f"import test_gpu_free_sparse as t; t.poison_worker({out!r})"
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    got = np.load(out)
    for route, name in POISON_CASES:
        a, _, mu = two_runs(fe.prob(name, ROUTES[route][0]), route)
        for k in ("jk", "val", "ea", "dp", "scal"):
            g = got[f"{route}|{name}|{k}"]
            assert g.shape == a[k].shape and g.tobytes() == a[k].tobytes(), f"{route} {name}: {k} differs under poison"
        assert bits_equal(got[f"{route}|{name}|info"], [a["rc"], a["iters"], a["relres"], mu])


# ---- g. psba_levmar against the dense solver ------------------------------------------------------------------------------

LM_ITERS = 15


@pytest.mark.parametrize("route,name", list(LM_GAP))
def test_levmar_parity_with_the_dense_solver(route, name):
    if name == "ring":
        p, kc0, poses = hr.held_ring()
    else:
        p, kc0, poses = P54(), None, None
    out = []
    for solver in (2, 0):
        h = open_handle(p, route, solver, tol=1e-10, kc=kc0)
        try:
            if poses is not None:
                h.set_held(poses, None)
            res, log = h.levmar(max_iter=LM_ITERS, tr_handoff=False, log_cap=256)
            out.append((res, log))
        finally:
            h.close()
    (rs, ls), (rd, ld) = out
    gap = abs(rs.final_err - rd.final_err) / rd.final_err
    bound = min(4.0 * LM_GAP[(route, name)], 1e-6)
    print(f"\n{route} {name}: LM final cost sparse {rs.final_err!r}, dense {rd.final_err!r}, relative gap {gap:.3e}, "
          f"iterations {rs.iters} / {rd.iters}, flags {rs.flag} / {rd.flag}")
    note(f"{route} {name}", "LM cost gap / allowed", gap / bound)
    assert rs.flag == rd.flag and rs.pcg_unconverged == 0 and rd.pcg_unconverged == 0
    assert gap <= bound, f"{route} {name}: relative gap of the final costs {gap:.3e} > {bound:.3e}"
    assert rs.final_err < rs.init_err


# ---- h. size --------------------------------------------------------------------------------------------------------

def test_size_2050_cameras_of_16():
    """nA = 32 800: the dense route's red + chol_L alone would take (2 n32 + 16) n32 doubles each, 34 GB together"""
    import ctypes

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    p = big_problem("band", 2050)
    nC, cnp = 2050, 16
    nA = cnp * nC
    n32 = (nA + 31) // 32 * 32
    dense_bytes = 2 * 8 * (2 * n32 + 16) * n32
    assert nA == 32800 and dense_bytes > 34e9
    import psba_amd
    psba_amd.Psba(0).close()                                   # (the device is initialised before the first reading)
    free0 = free_bytes()
    h = open_handle(p, "kd-bal", 2, max_iter=2000)
    try:
        taken = free0 - free_bytes()
        nblk = h.pcg_info()[2]
        want = fp.rows_enumeration(nC, p["iidx"], p["jidx"])["jk"]
        print(f"\nband of 2050 cameras: {nblk} stored blocks of {nC * (nC + 1) // 2}, device memory taken {taken / 2**20:.1f} MiB "
              f"(dense red + chol_L: {dense_bytes / 2**30:.1f} GiB)")
        assert nblk == len(want) and taken < dense_bytes
        res, log = h.levmar(max_iter=3, tr_handoff=False, log_cap=64)
        costs = log[log[:, 4] == 1, 1]                          # the cost after every accepted step
        print(f"costs {res.init_err!r} -> {res.final_err!r} in {res.iters} iterations, {res.tries} tries, log {log.tolist()}")
        assert res.iters == 3 and res.pcg_unconverged == 0 and res.final_err < res.init_err
        assert costs.size >= 1 and np.all(np.diff(np.concatenate([[res.init_err], costs])) < 0)
        h.linearize(1.0, 1.0)                                  # the last solve again: the damping of the loop's last try
        t = run_try(h, float(log[-1, 3]))
        assert t["sc"].status == 0
        judge_dpa("kd-bal band2050 after LM", fp.ListOp(nC, t["jk"], t["val"], cnp), t)
    finally:
        h.close()
