"""psba_sparse_point_covariance on the GPU (kernels_free_pcg_points.hip): the joint covariance of chosen 3-D
points under PSBA_SOLVER_SPARSE on camera blocks of 11 (fk) and 16 (kd-all / kd-bal).  Needs an MI355X.
tests/sparseptcov_ref.py holds the reference and derives the bounds.

  a  every solved column by its true residual in long double from the device's own blocks and the device's own Y
  b  C per entry on the device's own inputs (cols, V, Y) within the contraction bound; the exact parts as bits
  c  against psba_free_covariance_compute + psba_get_free_point_covariance of a dense handle under composed settings
  d  independence of the chosen set, its order, the position in a panel and the batch; two calls; a poisoned child
     process; 513 cameras
  e  track lengths around the contract kernel's edges: 1, 2, 63, 64, 65 cameras and every camera of the scene (66).
     wide_problem(65) holds no track longer than 13, so the scene is drawn for this test with freekd_twin._scene
  f  per-column stops and the failure protocol through psba_set_sparse_S, and a good call after each failure
  g  state rules: every refusal by code and text, the handle unchanged; a solve after a compute
The module prints found / allowed per judge.

c's bound.  The gap of the diagonal 3 x 3 blocks to the dense route in sigma-units, max |dC_rc| / sqrt(C_rr C_cc), was
measured on an MI355X (DENSE_GAP below); the test allows four times the measurement and never more than 1e-6
(the LM_GAP precedent of test_gpu_free_sparse.py: the solve is deterministic, the margin is for another compiler)."""
import ctypes
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
import sparsecov_ref as sc
import sparseptcov_ref as sp
import test_gpu_free_entrywise as fe
import test_gpu_free_sparse as gs
from freekd_twin import _scene, wide_problem
from test_freekd_twin import P54
from test_gpu_free_sparse import ROUTES, bits_equal, open_handle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

PSBA_OK, PSBA_NOT_SPD, PSBA_SINGULAR_V, PSBA_PCG_MAXIT, PSBA_E_STATE, PSBA_E_INVALID = 0, 1, 2, 4, -6, -1
TOL = gs.TRY_TOL
ALL_ROUTES = ["fk", "kd-all", "kd-bal"]
# c: measured on an MI355X, (input, route, damping rule) -> the gap in sigma-units
DENSE_GAP = {("P54", "fk", "identity"): 3.345e-16, ("P54", "fk", "marquardt"): 3.197e-13,
             ("P54", "kd-bal", "identity"): 3.100e-16, ("P54", "kd-bal", "marquardt"): 2.394e-15,
             ("ring", "kd-bal", "identity"): 9.857e-15, ("ring", "kd-bal", "marquardt"): 9.577e-15}
_CONSTRUCTED = {}


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for c in _CONSTRUCTED.values():
        c.close()
    _CONSTRUCTED.clear()


def live_of(route, nC, poses=None):
    """[cnp nC] bool: neither masked by the route's mask nor a held pose coordinate"""
    cnp, free = ROUTES[route]
    ni = cnp - 6
    live = np.ones((nC, cnp), dtype=bool)
    if free is not None:
        live[:, :ni] &= np.asarray(free, dtype=bool)[None, :]
    if poses is not None:
        live[np.asarray(poses) != 0, ni:] = False
    return live.reshape(-1)


def judge_call(case, h, p, route, sel, mu, scale=1.0, held_pts=None, poses=None, rule=fr.NO_RULE):
    """a + b on one call: (C, info, V, Y)"""
    cnp = ROUTES[route][0]
    nC, nP = int(p["nC"]), int(p["nP"])
    C, info = h.sparse_point_covariance(sel, mu=mu, scale=scale, want_cols=True)
    assert info["status"] == PSBA_OK, f"{case}: status {info['status']}"
    jk, val, _ = h.get_sparse_S()
    op = fp.ListOp(nC, jk, val, cnp)
    V, Y = h.free_point_blocks()
    ptr, j = sp.tracks(p["iidx"], nP), np.asarray(p["jidx"])
    J = sp.column_judges(op, info["cols"], Y, ptr, j, sel, held_pts, info["iters"], TOL, cnp)
    solved = J[:, 2] > 0
    if solved.any():
        print(f"{case}: worst true residual / allowed {np.max(J[solved, 0] / J[solved, 1]):.3e} "
              f"(iterations {info['iters'][solved].min()} .. {info['iters'][solved].max()})")
    assert np.all(info["relres"][solved] <= TOL) and np.all(info["iters"][solved] > 0) and np.all(J[:, 0] <= J[:, 1]), case
    assert np.all(info["iters"][~solved] == 0) and sc.plus_zero(info["relres"][~solved]) and sc.plus_zero(info["cols"][~solved])
    want, bound = sp.contract(info["cols"], V, Y, ptr, j, sel, held_pts, mu, rule, scale, cnp)
    ratio = sp.contract_ratio(C, want, bound)
    print(f"{case}: C found / allowed {ratio:.3e} per entry")
    assert ratio <= 1.0, case
    assert sp.exact_parts(C, info, sel, held_pts) == [], case
    assert sc.plus_zero(info["cols"][:, ~live_of(route, nC, poses)]), f"{case}: a masked or held coordinate of a column is not +0.0"
    return C, info, V, Y


# ---- a, b. columns by their true residual; C per entry ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "P54", "wide65"])
@pytest.mark.parametrize("route", ALL_ROUTES)
def test_columns_and_entries_on_an_assembled_try(route, name):
    p = {"tiny": lambda: fe.prob("tiny"), "P54": P54, "wide65": lambda: wide_problem(65)}[name]()
    nP = int(p["nP"])
    sel = {"tiny": [2, 0, 1], "P54": [449, 3, 100, 17, 250, 8, 301], "wide65": [nP - 1, 0, 200, 31, 77, 150]}[name]
    h = open_handle(p, route, 2)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        C, info, V, Y = judge_call(f"{route} {name}", h, p, route, sel, mu, 2.0)
        if name == "wide65":                                        # the point without observations: scale V*^-1 alone
            assert np.all(info["iters"][:3] == 0) and sc.plus_zero(C[:3, 3:])
            assert bits_equal(C[:3, :3], 2.0 * h.sparse_point_covariance([nP - 1], mu=mu)[0])
            np.testing.assert_allclose(C[:3, :3], 2.0 * np.linalg.inv(V[nP - 1] + mu * np.eye(3)), rtol=1e-12)
    finally:
        h.close()


@pytest.mark.parametrize("marquardt", [False, True])
@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_exact_parts_with_held_poses_and_points(route, marquardt):
    """a held point's zeros, zero rows of cols on masked and held coordinates, scale = 4 is 4 x scale = 1; the point
    without observations gives the bits of the dense route's kernel (scale V*^-1 by the same closed form)"""
    p = wide_problem(65)
    nC, nP = int(p["nC"]), int(p["nP"])
    rule = fe.MQ["default"] if marquardt else fr.NO_RULE
    poses, pts = hr.flags(nC, [0, 7]), hr.flags(nP, [200, 40])
    # (Marquardt: the point without observations has V* = mu dmin I, |det| = 1e-27 < 1e-16 -- PSBA_SINGULAR_V by the
    # definition, on the dense route as well; a point seen once takes its place and nothing is compared as bits)
    sel = [40, 0 if marquardt else nP - 1, 31, 200, 150, 77]
    out = {}
    for solver in (2,) if marquardt else (2, 0):
        h = open_handle(p, route, solver, rule=rule)
        try:
            h.set_held(poses, pts)
            h.linearize(1.0, 1.0)
            mu = out.setdefault("mu", 1e-3 if marquardt else 1e-3 * h.max_diag())       # the sparse handle's, for both
            if solver:
                C1, i1, _, _ = judge_call(f"{route} wide65 held" + (" marquardt" if marquardt else ""), h, p, route, sel, mu, 1.0,
                                          pts, poses, rule)
                C4, i4 = h.sparse_point_covariance(sel, mu=mu, scale=4.0, want_cols=True)
                assert bits_equal(C4, 4.0 * C1) and bits_equal(i4["cols"], i1["cols"])
                out["C4"] = C4
            else:
                assert h.free_covariance(mu=mu, scale=4.0) == PSBA_OK
                out["dense"] = h.free_point_covariance()
        finally:
            h.close()
    if not marquardt:
        assert bits_equal(out["C4"][3:6, 3:6], out["dense"][nP - 1]) and np.all(np.diag(out["dense"][nP - 1]) > 0.0)


# ---- c. against the dense route -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("marquardt", [False, True])
@pytest.mark.parametrize("name,route", [("P54", "fk"), ("P54", "kd-bal"), ("ring", "kd-bal")])
def test_against_the_dense_route_under_composed_settings(name, route, marquardt):
    """held poses and a held point, priors, Huber with sigmas, both damping rules.  The ring with two poses held runs
    at mu = 0 under the identity rule (kd-bal only: blocks of 11 are singular to rounding there)"""
    import psba_amd
    cnp = ROUTES[route][0]
    if name == "ring":
        p, kc0, poses = hr.held_ring()
    else:
        p, kc0, poses = P54(), None, hr.flags(54, [0, 1])
    nC, nP = int(p["nC"]), int(p["nP"])
    rng = np.random.default_rng(5)
    pts = hr.flags(nP, [5])
    sigma = rng.uniform(0.5, 2.0, int(p["nO"]))
    sel, scale = [9, 5, 0, 33, 71, 118, 64], 3.0
    out = {}
    for solver in (2, 0):
        h = open_handle(p, route, solver, kc=kc0, rule=fe.MQ["default"] if marquardt else fr.NO_RULE, max_iter=2000)
        try:
            cams, pts0 = h.get_params(0)
            h.set_held(poses, pts)
            h.set_priors(cams * (1.0 + 1e-3), np.full((nC, cnp), 1e-2), pts0 + 1e-3, np.full((nP, 3), 1e-1))
            h.set_obs_weighting(psba_amd.LOSS_HUBER, 2.0, sigma)
            h.linearize(1.0, 1.0)
            mu = out.setdefault("mu", 1e-4 if marquardt else (0.0 if name == "ring" else 1e-3 * h.max_diag()))
            if solver:
                out["C"] = judge_call(f"{route} {name} composed" + (" marquardt" if marquardt else ""), h, p, route, sel, mu,
                                      scale, pts, poses, fe.MQ["default"] if marquardt else fr.NO_RULE)[0]
            else:
                assert h.free_covariance(mu=mu, scale=scale) == PSBA_OK
                out["dense"] = h.free_point_covariance()
        finally:
            h.close()
    gap = 0.0
    for a, i in enumerate(sel):
        got, want = out["C"][3 * a:3 * a + 3, 3 * a:3 * a + 3], out["dense"][i]
        if pts[i]:
            assert sc.plus_zero(got) and sc.plus_zero(want)
            continue
        sd = np.sqrt(np.diag(want))
        assert np.all(sd > 0.0)
        gap = max(gap, float((np.abs(got - want) / np.outer(sd, sd)).max()))
    key = (name, route, "marquardt" if marquardt else "identity")
    allowed = min(4.0 * DENSE_GAP[key], 1e-6)
    print(f"{key}: sparse against dense {gap:.3e} sigma-units, allowed {allowed:.3e}")
    assert gap <= allowed


# ---- d. independence ------------------------------------------------------------------------------------------------------

def per_point(C, info, sel):
    return {s: (info["cols"][3 * a:3 * a + 3].copy(), info["iters"][3 * a:3 * a + 3].copy(),
                info["relres"][3 * a:3 * a + 3].copy(), C[3 * a:3 * a + 3, 3 * a:3 * a + 3].copy()) for a, s in enumerate(sel)}


def same_columns(x, y):
    return bits_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and bits_equal(x[2], y[2]) and bits_equal(x[3], y[3])


Q, Q2 = 17, 250
OTHERS = list(range(55, 445, 10))      # 39 other points
D_SELS = [[Q], [Q, 61, 62, 63, 64], [61, 62, 63, 64, 65, Q], OTHERS + [Q, Q2], (OTHERS + [Q, Q2])[::-1], [Q2], [Q, Q2]]


def p54_run(route, sels):
    h = open_handle(P54(), route, 2)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        return [h.sparse_point_covariance(s, mu=mu, want_cols=True) for s in sels]
    finally:
        h.close()


@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_columns_do_not_depend_on_the_chosen_set(route):
    """alone; first of 5; last of 6 (second panel); positions 39 and 40 of 41 (the batch boundary at 8 panels x 5
    points); reversed; the same call twice"""
    assert len(OTHERS) == 39
    runs = p54_run(route, D_SELS + [D_SELS[3]])
    assert all(info["status"] == PSBA_OK for _, info in runs)
    pp = [per_point(C, info, s) for (C, info), s in zip(runs, D_SELS + [D_SELS[3]])]
    alone, first5, last6, b41, rev, alone2, pair, again = pp
    assert np.all(alone[Q][1] > 1)
    for other in (first5, last6, b41, rev, pair, again):
        assert same_columns(alone[Q], other[Q])
    for other in (b41, rev, pair, again):
        assert same_columns(alone2[Q2], other[Q2])
    for s in OTHERS:
        assert same_columns(b41[s], rev[s]), f"point {s}"
    assert bits_equal(runs[3][0], runs[7][0]) and bits_equal(runs[3][1]["cols"], runs[7][1]["cols"])


def poison_worker(out):
    """(in a process of its own, started with PSBA_DEBUG_POISON=1)"""
    res = {}
    for route in ("fk", "kd-bal"):
        (C, info), = p54_run(route, [[Q, 61, 62, 63, 64, Q2]])
        res[f"{route}|C"], res[f"{route}|cols"], res[f"{route}|iters"], res[f"{route}|relres"] = C, info["cols"], info["iters"], info["relres"]
    np.savez(out, **res)


def test_poisoned_allocations_give_the_same_bits(tmp_path):
    """The handle reads PSBA_DEBUG_POISON once per process, so the poisoned run is a child process: that is what this
    test is about."""
    out = str(tmp_path / "poisoned.npz")
    env = dict(os.environ, PSBA_DEBUG_POISON="1")
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; " \
           f"import test_gpu_sparse_point_covariance as t; t.poison_worker({out!r})"
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    got = np.load(out)
    for route in ("fk", "kd-bal"):
        (C, info), = p54_run(route, [[Q, 61, 62, 63, 64, Q2]])
        assert bits_equal(got[f"{route}|C"], C) and bits_equal(got[f"{route}|cols"], info["cols"])
        assert np.array_equal(got[f"{route}|iters"], info["iters"]) and bits_equal(got[f"{route}|relres"], info["relres"])


def test_513_cameras_where_the_product_grid_takes_its_second_trip():
    nC = 513
    assert (nC + 3) // 4 > 128
    p = gs.big_problem("band", nC)
    h = open_handle(p, "kd-bal", 2)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        sel = [1000, 100, 7]
        C1, i1, _, _ = judge_call("kd-bal band513", h, p, "kd-bal", sel, mu)
        C2, i2 = h.sparse_point_covariance(sel, mu=mu, want_cols=True)
        Ca, ia = h.sparse_point_covariance([100], mu=mu, want_cols=True)
        assert np.all(i1["iters"] > 1)
        assert bits_equal(C1, C2) and bits_equal(i1["cols"], i2["cols"]) and np.array_equal(i1["iters"], i2["iters"])
        assert same_columns(per_point(C1, i1, sel)[100], per_point(Ca, ia, [100])[100])
    finally:
        h.close()


# ---- e. track lengths -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def track_scene():
    rng = np.random.default_rng(43)
    nC, nP = 66, 60
    lens = np.r_[[1, 2, 63, 64, 65, 66, 3], rng.integers(3, 9, nP - 7)]
    keep = np.zeros((nP, nC), dtype=bool)
    for i, n in enumerate(lens):
        keep[i, rng.choice(nC, size=n, replace=False)] = True
    return _scene(rng, nC, rng.uniform(-1.0, 1.0, (nP, 3)), keep), lens


@pytest.mark.parametrize("route", ALL_ROUTES)
def test_track_lengths_around_the_contract_kernels_edges(route):
    p, lens = track_scene()
    assert np.array_equal(np.bincount(p["iidx"], minlength=60), lens) and lens[5] == p["nC"]
    h = open_handle(p, route, 2)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        judge_call(f"{route} tracks 1, 2, 63 .. 66", h, p, route, [5, 0, 4, 1, 3, 2, 6], mu, 1.5)
    finally:
        h.close()


# ---- f. per-column stops and the failure protocol ----------------------------------------------------------------------------

def constructed(name, route):
    if (name, route) not in _CONSTRUCTED:
        _CONSTRUCTED[(name, route)] = gs.Constructed(name, route)
    return _CONSTRUCTED[(name, route)]


@pytest.mark.parametrize("route", ["fk", "kd-all"])
def test_failure_protocol(route):
    """error returns of a healthy kernel on chosen data: the right-hand sides are the pattern problem's own Y"""
    c = constructed("band43", route)
    sy = fp.quality_system("band43", *fp.QUALITY[0], c.c)
    prob = fp.pattern_problem(c.n_cams, c.blocks)
    iidx, jidx = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    sel = [int(iidx[jidx == 21][0]), int(iidx[jidx == 3][0])]
    assert sel[0] != sel[1]
    c.h.set_solver(2, tol=fp.TOL, max_iter=fp.MAXIT)

    def call(S=None, val=None):
        c.load(S, np.zeros(c.nA), val=val)
        return c.h.sparse_point_covariance(sel, mu=gs.MU, reassemble=False)

    def good(what):
        C, info = call(sy["S"])
        assert info["status"] == PSBA_OK and np.all(info["relres"] <= fp.TOL) and np.all(info["iters"] > 0), f"{route} after {what}: {info}"
        return C

    C0 = good("nothing")
    assert call(fp.bad_diag(c.n_cams, c.blocks, 21, c.c // 2, c.c))[1]["status"] == PSBA_NOT_SPD
    good("a bad pivot")
    j, k = next(b for b in sorted(c.blocks) if b[0] == 21)
    S = fp.dominant(c.n_cams, c.blocks, 1.0, c.c, 0.0, 0)
    I = np.eye(c.c)
    for (r, s), B in (((j, j), I), ((k, k), I), ((j, k), 2 * I), ((k, j), 2 * I)):
        S[c.c * r:c.c * r + c.c, c.c * s:c.c * s + c.c] = B
    info = call(S)[1]
    assert info["status"] == PSBA_NOT_SPD and info["iters"].max() < fp.MAXIT
    good("an indefinite S")
    val = fp.blocks_of(sy["S"], c.jk, c.c)
    at = next(i for i, (r, s) in enumerate(c.jk) if r == 21 and s != 21)
    val[at, 2, c.c - 1] = np.nan
    assert call(val=val)[1]["status"] == PSBA_NOT_SPD
    good("a NaN block")
    c.h.set_solver(2, tol=fp.TOL, max_iter=3)
    C3, info = call(sy["S"])
    late = info["relres"] > fp.TOL
    assert info["status"] == PSBA_PCG_MAXIT and late.any() and np.all(info["iters"][late] == 3)
    assert np.all(np.isfinite(C3)) and np.all(np.diag(C3) > 0.0) and bits_equal(C3, C3.T)        # C is still written
    c.h.set_solver(2, tol=fp.TOL, max_iter=fp.MAXIT)
    assert bits_equal(good("a budget of 3"), C0)
    c.good("after the failures")


def test_a_singular_point_block_is_reported():
    """priors on every camera and on every point but the one without observations: S is positive definite at mu = 0,
    and that point's V* = 0"""
    route, cnp = "kd-bal", 16
    p = wide_problem(65)
    nC, nP = int(p["nC"]), int(p["nP"])
    h = open_handle(p, route, 2)
    try:
        cams, pts0 = h.get_params(0)
        info_b = np.full((nP, 3), 1e-1)
        info_b[nP - 1] = 0.0
        h.set_priors(cams, np.full((nC, cnp), 1.0), pts0, info_b)
        _, info = h.sparse_point_covariance([31, nP - 1], mu=0.0)
        assert info["status"] == PSBA_SINGULAR_V and np.all(info["iters"][3:] == 0)
        C, info = h.sparse_point_covariance([31, 77], mu=0.0)
        assert info["status"] == PSBA_OK and np.all(np.diag(C) > 0.0)
    finally:
        h.close()


# ---- g. state rules -------------------------------------------------------------------------------------------------------------

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
            h.sparse_point_covariance(kw.pop("sel", [0]), **kw)
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), f"{w!r} not in {e.value}"

    h = psba_amd.Psba(0)                                               # before an upload
    h.set_camera_model(psba_amd.CAMERA_FREE_KD if cnp == 16 else psba_amd.CAMERA_FREE_K)
    h.set_solver(psba_amd.SOLVER_SPARSE)
    refused(h, PSBA_E_STATE, "psba_sparse_point_covariance")
    h.close()
    h = open_handle(p, route, 0)                                       # a dense free-intrinsics handle
    refused(h, PSBA_E_STATE, "psba_sparse_point_covariance", "PSBA_SOLVER_SPARSE", "psba_free_covariance_compute")
    h.close()
    six = psba_amd.Psba(0)                                             # six-parameter blocks
    six.set_solver(psba_amd.SOLVER_SPARSE)
    six.upload_problem(p)
    refused(six, PSBA_E_STATE, "psba_sparse_point_covariance", "PSBA_SOLVER_SPARSE", "psba_covariance_compute")
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
        refused(h, PSBA_E_INVALID, "sel_pts[1] = 3", sel=[0, p["nP"]])
        refused(h, PSBA_E_INVALID, "sel_pts[1] = -1", sel=[0, -1])
        refused(h, PSBA_E_INVALID, "point 1 is listed twice", sel=[1, 0, 1])
        one = np.zeros(1, dtype=np.int32)
        rc = lib.psba_sparse_point_covariance(h._h, 0.0, 1.0, 1, 1, one.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None,
                                              None, None)
        assert rc == PSBA_E_INVALID and "C is a null pointer" in lib.psba_last_error(h._h).decode()
        with pytest.raises(PsbaError) as e:                            # the solve above ended the assembled state
            h.sparse_point_covariance([0], reassemble=False)
        assert e.value.code == PSBA_E_STATE
        a, b = try_bits(fresh, mu), try_bits(h, mu)                    # the refusals changed nothing
        assert a[:2] == b[:2] and bits_equal(a[2], b[2]) and bits_equal(a[3], b[3])
    finally:
        h.close()
        fresh.close()


@pytest.mark.parametrize("route", ["fk", "kd-bal"])
def test_a_solve_after_a_compute_is_that_of_a_fresh_handle(route):
    p = P54()
    out = []
    for compute in (True, False):
        h = open_handle(p, route, 2, tol=1e-10)
        try:
            h.linearize(1.0, 1.0)
            mu = 1e-3 * h.max_diag()
            if compute:
                C, info = h.sparse_point_covariance([3, 40, 449, 7, 8, 9], mu=mu)
                assert info["status"] == PSBA_OK
                Cr, ir = h.sparse_point_covariance([3, 40, 449, 7, 8, 9], mu=mu, reassemble=False)   # the blocks as they stand
                assert ir["status"] == PSBA_OK and bits_equal(C, Cr)
                rc = h.schur_solve()                                   # the handle is left as after psba_schur_assemble(mu)
                it = h.pcg_info()[:2]
                s = h.backsub(mu)
                t = (rc, it, h.get_dp(), np.array([s.status, s.dp_l2, s.gain_den, s.new_cost, s.newp_l2]))
                h.sparse_point_covariance([3], mu=mu)
            else:
                t = try_bits(h, mu)
            res, log = h.levmar(max_iter=5, tr_handoff=False, log_cap=64)
            out.append((t, res.final_err, res.iters, log, h.get_params(0)))
        finally:
            h.close()
    (ta, ea, ia, la, pa), (tb, eb, ib, lb, pb) = out
    assert ta[:2] == tb[:2] and bits_equal(ta[2], tb[2]) and bits_equal(ta[3], tb[3])
    assert ea == eb and ia == ib and bits_equal(la, lb) and bits_equal(pa[0], pb[0]) and bits_equal(pa[1], pb[1])
