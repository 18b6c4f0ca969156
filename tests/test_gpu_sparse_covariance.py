"""psba_sparse_camera_covariance and psba_sparse_S_times_many on the GPU (kernels_free_pcg_many.hip): the
covariance of chosen cameras under PSBA_SOLVER_SPARSE on camera blocks of 11 (fk) and 16 (kd-all / kd-bal).  Needs an
MI355X.  tests/sparsecov_ref.py holds the reference and derives the bounds from freepcg_ref.py and cov_ref.py.

  a  the product kernel on constructed systems (psba_set_sparse_S), NaN in the strict upper triangles, 1 and 3 panels
  b  every solved column by its true residual in long double from the device's own blocks
  c  C against the refined inverse in sigma-units: the ring scene with two poses held at mu = 0, P54 at mu > 0
  d  against psba_free_covariance_compute of a dense handle under composed settings and both damping rules
  e  dead coordinates: +0.0 bit for bit, C bit-symmetric, scale = 4 is 4 x scale = 1
  f  independence of the chosen set, its order and the batch; two calls, a poisoned child process, 512 / 513 cameras
  g  per-column stop: an isolated camera's columns take 1 iteration; the stop at iterations 7, 8, 9, 16, 17
  h  the failure protocol, and a good call after each failure
  i  state rules: every refusal by code and text, reassemble = 0, a solve or psba_levmar after a compute
The module prints found / allowed per judge."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import freecov_ref as fc
import freepcg_ref as fp
import held_ref as hr
import sparsecov_ref as sc
import test_gpu_free_entrywise as fe
import test_gpu_free_sparse as gs
from freekd_twin import wide_problem
from test_freekd_twin import P54
from test_gpu_free_sparse import ROUTES, bits_equal, open_handle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

PSBA_OK, PSBA_NOT_SPD, PSBA_PCG_MAXIT, PSBA_E_STATE, PSBA_E_INVALID = 0, 1, 4, -6, -1
TOL = gs.TRY_TOL
C_ROUTES = ["fk", "kd-all"]
_CONSTRUCTED = {}


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for c in _CONSTRUCTED.values():
        c.close()
    _CONSTRUCTED.clear()


def constructed(name, route):
    if (name, route) not in _CONSTRUCTED:
        _CONSTRUCTED[(name, route)] = gs.Constructed(name, route)
    return _CONSTRUCTED[(name, route)]


def live_of(route, nC, poses=None, cam_free=None):
    """[cnp nC] bool: neither masked (the route's global mask, a per-camera table) nor a held pose coordinate"""
    cnp, free = ROUTES[route]
    ni = cnp - 6
    live = np.ones((nC, cnp), dtype=bool)
    if free is not None:
        live[:, :ni] &= np.asarray(free, dtype=bool)[None, :]
    if cam_free is not None:
        live[:, :ni] &= np.asarray(cam_free, dtype=bool)
    if poses is not None:
        live[np.asarray(poses) != 0, ni:] = False
    return live.reshape(-1)


def device_S(h, cnp):
    jk, val, _ = h.get_sparse_S()
    return jk, val, fp.dense_of(h.nC, jk, val, cnp)


def judge_columns(case, S, info, sel, live, cnp, tol=TOL):
    """b: ||e_q - S x_q||_2 <= tol + C_GAP gap_unit per live chosen column; returns the allowed residuals"""
    found, allowed = sc.column_residuals(S, info["cols"], sel, live, info["iters"], tol, cnp)
    lv = live[sc.chosen_coords(sel, cnp)]
    worst = float(np.max(found[lv] / allowed[lv])) if lv.any() else 0.0
    print(f"{case}: worst true residual / allowed {worst:.3e} (iterations {info['iters'][lv].min()} .. {info['iters'][lv].max()})")
    assert np.all(info["relres"][lv] <= tol) and np.all(found <= allowed), f"{case}: {found[lv].max():.3e}"
    return allowed


# ---- a. the product ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["five", "trip", "band43"])
@pytest.mark.parametrize("route", C_ROUTES)
def test_product_of_panels(route, name):
    c = constructed(name, route)
    S = fp.dominant(c.n_cams, c.blocks, 1e-2, c.c, 2.0, 2)
    c.load(S, np.zeros(c.nA), poison=True)               # NaN in the strict upper triangle of every diagonal block
    rng = np.random.default_rng([3, c.nA])
    X = rng.choice([-1.0, 1.0], (3, c.nA, 16)) * 10.0 ** rng.uniform(-4, 4, (3, c.nA, 16))
    for k, (_, v) in enumerate(fp.product_vectors(c.n_cams, c.c)):
        X[0, :, k] = v
    Y = c.h.sparse_S_times_many(X)
    worst = 0.0
    for m in range(3):
        for n in range(16):
            err = np.abs(Y[m, :, n].astype(fp.LD) - fp.spmv_exact(S, X[m, :, n])).astype(np.float64)
            bound = fp.spmv_bound(S, X[m, :, n], c.m, c.c)
            assert np.all(err <= bound), f"{route} {name}: panel {m} column {n} row {int(np.argmax(err - bound))}"
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    print(f"{route} {name}: product / bound {worst:.3e}")
    assert bits_equal(c.h.sparse_S_times_many(X[1:2])[0], Y[1])          # one panel alone
    Z = c.h.sparse_S_times_many(X[[2, 0, 1]])                            # ... and in another position
    assert bits_equal(Z[0], Y[2]) and bits_equal(Z[1], Y[0]) and bits_equal(Z[2], Y[1])
    c.good("after psba_sparse_S_times_many")


# ---- b. columns by their true residual --------------------------------------------------------------------------------

@pytest.mark.parametrize("name,delta,grade", [("trip", 1e-2, 0.0), ("band43", 1e-2, 4.0)])
@pytest.mark.parametrize("route", C_ROUTES)
def test_columns_on_constructed_systems(route, name, delta, grade):
    c = constructed(name, route)
    S = fp.dominant(c.n_cams, c.blocks, delta, c.c, grade, 4)
    c.h.set_solver(2, tol=TOL, max_iter=fp.MAXIT)
    c.load(S, np.zeros(c.nA), poison=True)
    sel = [c.n_cams - 1, 0, c.n_cams // 2]
    live = np.ones(c.nA, dtype=bool)
    C, info = c.h.sparse_camera_covariance(sel, reassemble=False, want_cols=True)
    assert info["status"] == PSBA_OK
    judge_columns(f"{route} {name}", S, info, sel, live, c.c)
    assert sc.exact_parts(C, info["cols"], sel, live, c.c) == []
    Cw, _ = sc.assemble(info["cols"], sel, live, 1.0, c.c)
    assert bits_equal(C, Cw)                                               # the assembly rule, bit for bit


@functools.lru_cache(maxsize=None)
def assembled_problem(name, cnp):
    return P54() if name == "P54" else wide_problem(65)


@pytest.mark.parametrize("name", ["P54", "wide65"])
@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_columns_on_an_assembled_try(route, name):
    cnp = ROUTES[route][0]
    p = assembled_problem(name, cnp)
    h = open_handle(p, route, 2)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        sel = [0, p["nC"] - 1, 3]
        C, info = h.sparse_camera_covariance(sel, mu=mu, want_cols=True)
        assert info["status"] == PSBA_OK
        _, _, S = device_S(h, cnp)
        live = live_of(route, p["nC"])
        judge_columns(f"{route} {name}", S, info, sel, live, cnp)
        assert sc.exact_parts(C, info["cols"], sel, live, cnp) == []
        assert bits_equal(C, sc.assemble(info["cols"], sel, live, 1.0, cnp)[0])
    finally:
        h.close()


# ---- c. C against the inverse -------------------------------------------------------------------------------------------

def judge_C(case, S, C, info, sel, live, scale, cnp, kappa_max=None):
    rho = judge_columns(case, S, info, sel, live, cnp)
    j = sc.c_error_and_bound(S, C, sel, live, rho, scale, cnp)
    print(f"{case}: C found {j['found']:.3e} / allowed {j['allowed']:.3e} sigma-units (worst entry ratio {j['ratio']:.3e}), "
          f"kappa of the scaled S {j['kappa']:.3e}")
    if kappa_max is not None:
        assert j["kappa"] <= kappa_max, j["kappa"]
    assert j["ratio"] <= 1.0, f"{case}: {j['found']:.3e} > {j['allowed']:.3e}"
    return j


def test_C_on_the_ring_with_two_poses_held_at_mu_0():
    """kd-bal, the ring's own model ({f, k1, k2} free), as 7l's end-to-end test.  With all five intrinsics of a block of
    11 free the ring scene does not determine S at mu = 0 in fp64 (measured on an MI355X: smallest eigenvalue of the
    device's S -1.7e-10 against a largest of 6.2e6): the conjugate gradients break down with p.Sp <= 0 after 32 to 80
    iterations on every unit column, the float64 host twin does the same on the same blocks, and the verb returns
    PSBA_NOT_SPD -- so that block is judged at mu > 0 (test_C_on_P54_with_mu) and under priors (test d)."""
    route = "kd-bal"
    cnp = ROUTES[route][0]
    p, kc0, poses = hr.held_ring()
    h = open_handle(p, route, 2, kc=kc0)
    try:
        h.set_held(poses, None)
        sel = [4, 1, 2]
        C, info = h.sparse_camera_covariance(sel, mu=0.0, scale=2.0, want_cols=True)
        assert info["status"] == PSBA_OK
        _, _, S = device_S(h, cnp)
        live = live_of(route, p["nC"], poses)
        judge_C(f"{route} ring mu = 0", S, C, info, sel, live, 2.0, cnp, kappa_max=1e7)
        assert sc.exact_parts(C, info["cols"], sel, live, cnp) == []
    finally:
        h.close()


@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_C_on_P54_with_mu(route):
    cnp = ROUTES[route][0]
    p = P54()
    h = open_handle(p, route, 2)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        sel = [53, 7]
        C, info = h.sparse_camera_covariance(sel, mu=mu, want_cols=True)
        assert info["status"] == PSBA_OK
        _, _, S = device_S(h, cnp)
        judge_C(f"{route} P54 mu = {mu:.3e}", S, C, info, sel, live_of(route, p["nC"]), 1.0, cnp)
    finally:
        h.close()


# ---- d. against the dense route -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("marquardt", [False, True])
@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_against_the_dense_route_under_composed_settings(route, marquardt):
    import psba_amd
    cnp = ROUTES[route][0]
    p, kc0, poses = hr.held_ring()
    nC, nP = p["nC"], p["nP"]
    rng = np.random.default_rng(5)
    pts = np.zeros(nP, dtype=np.uint8)
    pts[5] = 1
    sigma = rng.uniform(0.5, 2.0, p["nO"])
    sel, scale = [5, 0, 3], 3.0
    mu = 1e-4 if marquardt else 0.0
    out = {}
    for solver in (2, 0):
        h = open_handle(p, route, solver, kc=kc0, rule=fe.MQ["default"] if marquardt else fr.NO_RULE)
        try:
            cams, pts0 = h.get_params(0)
            h.set_held(poses, pts)
            h.set_priors(cams * (1.0 + 1e-3), np.full((nC, cnp), 1e-2), pts0 + 1e-3, np.full((nP, 3), 1e-1))
            h.set_obs_weighting(psba_amd.LOSS_HUBER, 2.0, sigma)
            if solver:
                C, info = h.sparse_camera_covariance(sel, mu=mu, scale=scale, want_cols=True)
                assert info["status"] == PSBA_OK
                out["S"] = device_S(h, cnp)[2]
                out["C"], out["info"] = C, info
            else:
                assert h.free_covariance(mu=mu, scale=scale) == PSBA_OK
                out["dense"] = h.free_covariance_matrix()
        finally:
            h.close()
    live = live_of(route, nC, poses)
    case = f"{route} ring composed" + (" marquardt" if marquardt else "")
    j = judge_C(case, out["S"], out["C"], out["info"], sel, live, scale, cnp)
    idx = np.flatnonzero(live)
    _, _, dense_allowed, _ = fc.inverse_judge(out["S"][np.ix_(idx, idx)], out["dense"][np.ix_(idx, idx)] / scale)
    q = sc.chosen_coords(sel, cnp)
    D = out["dense"][np.ix_(q, q)]
    lv = live[q]
    assert sc.plus_zero(D[~lv, :]) and sc.plus_zero(D[:, ~lv])
    sd = np.sqrt(np.diag(j["Cref"]))
    gap = float((np.abs(out["C"][np.ix_(lv, lv)] - D[np.ix_(lv, lv)]) / np.outer(sd, sd)).max())
    print(f"{case}: sparse against dense {gap:.3e}, allowed {j['allowed']:.3e} + {dense_allowed:.3e}")
    assert gap <= j["allowed"] + dense_allowed


# ---- e. dead coordinates --------------------------------------------------------------------------------------------------

def test_dead_coordinates_are_plus_zero():
    route, cnp = "kd-bal", 16
    p = P54()
    nC = p["nC"]
    cam_free = np.ones((nC, 10), dtype=np.uint8)
    cam_free[7] = 0                                                    # camera 7: no free intrinsic ...
    cam_free[9, 5] = 0
    poses = np.zeros(nC, dtype=np.uint8)
    poses[[0, 7]] = 1                                                  # ... and a held pose: wholly fixed
    h = open_handle(p, route, 2)
    try:
        h.set_camera_masks(cam_free)
        h.set_held(poses, None)
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        sel = [7, 0, 9, 20]
        live = live_of(route, nC, poses, cam_free)
        C1, i1 = h.sparse_camera_covariance(sel, mu=mu, scale=1.0, want_cols=True)
        C4, i4 = h.sparse_camera_covariance(sel, mu=mu, scale=4.0, want_cols=True)
        assert i1["status"] == PSBA_OK and i4["status"] == PSBA_OK
        assert sc.exact_parts(C1, i1["cols"], sel, live, cnp) == [] and sc.exact_parts(C4, i4["cols"], sel, live, cnp) == []
        lv = live[sc.chosen_coords(sel, cnp)]
        assert not lv[:16].any() and np.all(i1["iters"][~lv] == 0) and np.all(i1["relres"][~lv] == 0.0)
        assert np.all(i1["iters"][lv] > 0)
        assert bits_equal(C4, 4.0 * C1) and bits_equal(i4["cols"], i1["cols"])
        _, _, S = device_S(h, cnp)
        judge_columns("kd-bal P54 with dead coordinates", S, i1, sel, live, cnp)
    finally:
        h.close()


# ---- f. independence and order ----------------------------------------------------------------------------------------------

def per_camera(info, sel, cnp):
    return {s: (info["cols"][cnp * a:cnp * a + cnp].copy(), info["iters"][cnp * a:cnp * a + cnp].copy(),
                info["relres"][cnp * a:cnp * a + cnp].copy()) for a, s in enumerate(sel)}


def same_columns(x, y):
    return bits_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and bits_equal(x[2], y[2])


def p54_run(route, sels):
    """[(C, info)] of the chosen lists on one P54 handle at mu = 1e-3 max diag"""
    h = open_handle(P54(), route, 2)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        return [h.sparse_camera_covariance(s, mu=mu, want_cols=True) for s in sels]
    finally:
        h.close()


F_SELS = [[5], [30], [5, 30], [30, 5], list(range(10, 18)), list(range(10, 19))]


@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_columns_do_not_depend_on_the_chosen_set(route):
    cnp = ROUTES[route][0]
    runs = p54_run(route, F_SELS + [[5, 30]])
    assert all(info["status"] == PSBA_OK for _, info in runs)
    cams = [per_camera(info, s, cnp) for (_, info), s in zip(runs, F_SELS + [[5, 30]])]
    a, b, ab, ba, e8, e9, again = cams
    assert same_columns(a[5], ab[5]) and same_columns(b[30], ab[30]) and same_columns(ab[5], ba[5]) and same_columns(ab[30], ba[30])
    for s in range(10, 18):                                            # the batch boundary: 8 panels against 8 + 1
        assert same_columns(e8[s], e9[s]), f"camera {s}"
    assert bits_equal(runs[4][0], runs[5][0][:8 * cnp, :8 * cnp])
    assert bits_equal(runs[2][0], runs[6][0]) and same_columns(ab[5], again[5]) and same_columns(ab[30], again[30])
    Cab, Cba = runs[2][0], runs[3][0]
    assert bits_equal(Cab[:cnp, :cnp], Cba[cnp:, cnp:]) and bits_equal(Cab[cnp:, cnp:], Cba[:cnp, :cnp])


def poison_worker(out):
    """(in a process of its own, started with PSBA_DEBUG_POISON=1)"""
    res = {}
    for route in ("fk", "kd-bal"):
        (C, info), = p54_run(route, [[5, 30]])
        res[f"{route}|C"], res[f"{route}|cols"], res[f"{route}|iters"], res[f"{route}|relres"] = C, info["cols"], info["iters"], info["relres"]
    np.savez(out, **res)


def test_poisoned_allocations_give_the_same_bits(tmp_path):
    """The handle reads PSBA_DEBUG_POISON once per process, so the poisoned run is a child process: that is what this
    test is about."""
    out = str(tmp_path / "poisoned.npz")
    env = dict(os.environ, PSBA_DEBUG_POISON="1")
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; " \
           f"import test_gpu_sparse_covariance as t; t.poison_worker({out!r})"
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    got = np.load(out)
    for route in ("fk", "kd-bal"):
        (C, info), = p54_run(route, [[5, 30]])
        assert bits_equal(got[f"{route}|C"], C) and bits_equal(got[f"{route}|cols"], info["cols"])
        assert np.array_equal(got[f"{route}|iters"], info["iters"]) and bits_equal(got[f"{route}|relres"], info["relres"])


@pytest.mark.parametrize("nC", [512, 513])
def test_two_calls_are_bit_identical_across_the_grid_trip(nC):
    """513 cameras: the product's grid of 128 workgroups of four block rows takes a second trip"""
    assert (nC > 512) == ((nC + 3) // 4 > 128)
    h = open_handle(gs.big_problem("band", nC), "kd-bal", 2)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        sel = [nC - 3, 100]
        lv = live_of("kd-bal", nC)[sc.chosen_coords(sel, 16)]
        C1, i1 = h.sparse_camera_covariance(sel, mu=mu, want_cols=True)
        C2, i2 = h.sparse_camera_covariance(sel, mu=mu, want_cols=True)
        assert i1["status"] == PSBA_OK and np.all(i1["iters"][lv] > 1) and np.all(i1["iters"][~lv] == 0)
        assert bits_equal(C1, C2) and bits_equal(i1["cols"], i2["cols"]) and np.array_equal(i1["iters"], i2["iters"])
        jk, val, _ = h.get_sparse_S()
        op = fp.ListOp(nC, jk, val, 16)
        for r, q in enumerate(sc.chosen_coords(sel, 16)):
            if not lv[r]:
                continue
            e = np.zeros(16 * nC)
            e[q] = 1.0
            tr, gap = fp.list_relres_and_gap(op, i1["cols"][r], e, int(i1["iters"][r]))
            assert tr <= TOL + fp.C_GAP * gap, f"column {r}: {tr:.3e}"
    finally:
        h.close()


# ---- g. per-column stop -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", C_ROUTES)
def test_an_isolated_camera_stops_after_one_iteration(route):
    """`trip`: leaves 8 and 9 share with no hub, so their block rows hold the diagonal block alone"""
    c = constructed("trip", route)
    S = fp.dominant(c.n_cams, c.blocks, 1e-2, c.c, 0.0, 6)
    c.h.set_solver(2, tol=1e-10, max_iter=fp.MAXIT)
    c.load(S, np.zeros(c.nA), poison=True)
    both = c.h.sparse_camera_covariance([8, 12], reassemble=False, want_cols=True)[1]
    alone = c.h.sparse_camera_covariance([12], reassemble=False, want_cols=True)[1]
    assert both["status"] == PSBA_OK and alone["status"] == PSBA_OK
    assert np.all(both["iters"][:c.c] == 1), both["iters"]
    assert np.all(both["iters"][c.c:] > 1)
    assert same_columns(per_camera(both, [8, 12], c.c)[12], per_camera(alone, [12], c.c)[12])


@pytest.mark.parametrize("k", fp.BURST_EDGES)
@pytest.mark.parametrize("route", C_ROUTES)
def test_stop_at_chosen_iteration(route, k):
    c = constructed("band43", route)
    cam = 20
    case = sc.burst_case_unit("band43", k, c.c, c.c * cam)
    assert case is not None
    c.h.set_solver(2, tol=case["tol"], max_iter=fp.MAXIT)
    c.load(case["S"], np.zeros(c.nA))
    info = c.h.sparse_camera_covariance([cam], reassemble=False)[1]
    print(f"\n{route} k = {k}: delta {case['delta']:.4g}, tol {case['tol']:.3e}, iterations {info['iters'].tolist()}")
    assert info["status"] == PSBA_OK and info["iters"][0] == k and info["relres"][0] <= case["tol"]
    c.h.set_solver(2, tol=case["tol"], max_iter=k - 1)
    info = c.h.sparse_camera_covariance([cam], reassemble=False)[1]
    assert info["status"] == PSBA_PCG_MAXIT and info["iters"][0] == k - 1 and info["relres"][0] > case["tol"]
    c.h.set_solver(2, tol=fp.TOL, max_iter=fp.MAXIT)


# ---- h. the failure protocol ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", C_ROUTES)
def test_failure_protocol(route):
    c = constructed("band43", route)
    sy = fp.quality_system("band43", *fp.QUALITY[0], c.c)
    c.h.set_solver(2, tol=fp.TOL, max_iter=fp.MAXIT)
    sel = [21, 3]

    def call(S=None, val=None):
        c.load(S, np.zeros(c.nA), val=val)
        return c.h.sparse_camera_covariance(sel, reassemble=False)[1]

    def good(what):
        info = call(sy["S"])
        assert info["status"] == PSBA_OK and np.all(info["relres"] <= fp.TOL), f"{route} after {what}: {info}"

    good("nothing")
    assert call(fp.bad_diag(c.n_cams, c.blocks, 21, c.c // 2, c.c))["status"] == PSBA_NOT_SPD
    good("a bad pivot")
    blocks = sorted(c.blocks)
    j, k = next(b for b in blocks if b[0] == 21)
    S = fp.dominant(c.n_cams, c.blocks, 1.0, c.c, 0.0, 0)
    I = np.eye(c.c)
    for (r, s), B in (((j, j), I), ((k, k), I), ((j, k), 2 * I), ((k, j), 2 * I)):   # freepcg_ref.indefinite_pd_diag on a pair of camera 21
        S[c.c * r:c.c * r + c.c, c.c * s:c.c * s + c.c] = B
    info = call(S)
    assert info["status"] == PSBA_NOT_SPD and info["iters"].max() < fp.MAXIT
    good("an indefinite S")
    val = fp.blocks_of(sy["S"], c.jk, c.c)
    at = next(i for i, (r, s) in enumerate(c.jk) if r == 21 and s != 21)
    val[at, 2, c.c - 1] = np.nan
    assert call(val=val)["status"] == PSBA_NOT_SPD
    good("a NaN block")
    c.h.set_solver(2, tol=fp.TOL, max_iter=3)
    info = call(sy["S"])
    assert info["status"] == PSBA_PCG_MAXIT and np.all(info["iters"][info["relres"] > fp.TOL] == 3) and np.any(info["relres"] > fp.TOL)
    c.h.set_solver(2, tol=fp.TOL, max_iter=fp.MAXIT)
    good("a budget of 3")
    c.good("after the failures")


# ---- i. state rules -----------------------------------------------------------------------------------------------------------

def try_bits(h, mu):
    h.schur_assemble(mu)
    rc = h.schur_solve()
    it = h.pcg_info()[:2]
    s = h.backsub(mu)
    return rc, it, h.get_dp(), np.array([s.status, s.dp_l2, s.gain_den, s.new_cost, s.newp_l2])


@pytest.mark.parametrize("route", ["fk", "kd-all"])
def test_refusals_change_nothing(route):
    import psba_amd
    from psba_amd.capi import PsbaError, lib
    cnp = ROUTES[route][0]
    p = fe.prob("tiny")

    def refused(h, code, *words, **kw):
        with pytest.raises(PsbaError) as e:
            h.sparse_camera_covariance(kw.pop("sel", [0]), **kw)
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), f"{w!r} not in {e.value}"

    h = psba_amd.Psba(0)                                               # before an upload
    h.set_camera_model(psba_amd.CAMERA_FREE_KD if cnp == 16 else psba_amd.CAMERA_FREE_K)
    h.set_solver(psba_amd.SOLVER_SPARSE)
    refused(h, PSBA_E_STATE, "psba_sparse_camera_covariance")
    h.close()
    h = open_handle(p, route, 0)                                       # a dense free-intrinsics handle
    refused(h, PSBA_E_STATE, "PSBA_SOLVER_SPARSE", "psba_free_covariance_compute")
    with pytest.raises(PsbaError) as e:
        h.sparse_S_times_many(np.zeros((1, cnp * p["nC"], 16)))
    assert e.value.code == PSBA_E_STATE and "PSBA_SOLVER_SPARSE" in str(e.value)
    h.close()
    six = psba_amd.Psba(0)                                             # six-parameter blocks
    six.set_solver(psba_amd.SOLVER_SPARSE)
    six.upload_problem(p)
    refused(six, PSBA_E_STATE, "PSBA_SOLVER_SPARSE", "psba_covariance_compute")
    six.close()
    fresh = open_handle(p, route, 2)
    h = open_handle(p, route, 2)
    try:
        for g in (fresh, h):
            g.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        h.schur_assemble(mu)
        h.schur_solve()
        h.backsub_async(mu)
        refused(h, PSBA_E_STATE, "in flight")                          # a try in flight
        h.backsub_wait()
        for bad in (np.nan, np.inf, -1.0):
            refused(h, PSBA_E_INVALID, "mu", mu=bad)
        for bad in (np.nan, np.inf, 0.0, -2.0):
            refused(h, PSBA_E_INVALID, "scale", scale=bad)
        refused(h, PSBA_E_INVALID, "n_sel", sel=[])
        refused(h, PSBA_E_INVALID, "sel[1] = 2", sel=[0, p["nC"]])
        refused(h, PSBA_E_INVALID, "sel[1] = -1", sel=[0, -1])
        refused(h, PSBA_E_INVALID, "camera 1 is listed twice", sel=[1, 0, 1])
        one = np.zeros(1, dtype=np.int32)
        rc = lib.psba_sparse_camera_covariance(h._h, 0.0, 1.0, 1, 1, one.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None,
                                               None, None)
        assert rc == PSBA_E_INVALID and "C is a null pointer" in lib.psba_last_error(h._h).decode()
        with pytest.raises(PsbaError) as e:                            # the solve above ended the assembled state
            h.sparse_camera_covariance([0], reassemble=False)
        assert e.value.code == PSBA_E_STATE
        a, b = try_bits(fresh, mu), try_bits(h, mu)                    # the refusals changed nothing
        assert a[:2] == b[:2] and bits_equal(a[2], b[2]) and bits_equal(a[3], b[3])
    finally:
        h.close()
        fresh.close()


@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_a_solve_or_levmar_after_a_compute_is_that_of_a_fresh_handle(route):
    p = P54()
    out = []
    for compute in (True, False):
        h = open_handle(p, route, 2, tol=1e-10)
        try:
            h.linearize(1.0, 1.0)
            mu = 1e-3 * h.max_diag()
            if compute:
                _, info = h.sparse_camera_covariance([3, 40], mu=mu)
                assert info["status"] == PSBA_OK
                rc = h.schur_solve()                                   # the handle is left as after psba_schur_assemble(mu)
                it = h.pcg_info()[:2]
                s = h.backsub(mu)
                t = (rc, it, h.get_dp(), np.array([s.status, s.dp_l2, s.gain_den, s.new_cost, s.newp_l2]))
                h.sparse_camera_covariance([3], mu=mu)
            else:
                t = try_bits(h, mu)
            res, log = h.levmar(max_iter=5, tr_handoff=False, log_cap=64)
            out.append((t, res.final_err, res.iters, log, h.get_params(0)))
        finally:
            h.close()
    (ta, ea, ia, la, pa), (tb, eb, ib, lb, pb) = out
    assert ta[:2] == tb[:2] and bits_equal(ta[2], tb[2]) and bits_equal(ta[3], tb[3])
    assert ea == eb and ia == ib and bits_equal(la, lb) and bits_equal(pa[0], pb[0]) and bits_equal(pa[1], pb[1])
