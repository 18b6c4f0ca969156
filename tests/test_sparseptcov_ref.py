"""The host reference of psba_sparse_point_covariance (tests/sparseptcov_ref.py) against itself, without a GPU: the two
statements of the model agree on tiny_problem (mu > 0), 7camsvarK with poses 0 and 1 held at mu = 0 under kd-bal and the
ring with priors; each injected fault fails the agreement; the float64 twin of the solve and a plain float64
contraction meet the bounds the device is held to; the twin's residual gap on Y right-hand sides is within C_GAP; the
entry points exist."""
import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import freecov_ref as fc
import freepcg_ref as fp
import held_ref as hr
import sparseptcov_ref as sp
from freekd_twin import tiny_problem
from test_freecov_ref import AGREE, MQ, ROUTES, p7, plain_route, ring

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

TOL = 1e-12


def agree(rt, sel, mu, rule=fr.NO_RULE, scale=1.0, fault=None):
    want, kappa = sp.dense_points(rt, sel, mu, rule, scale)
    got, kS = sp.schur_points(rt, sel, mu, rule, scale, fault)
    return sp.sigma_error(got, want), max(kappa, kS) * AGREE, want


def test_the_two_statements_agree_on_tiny_problem():
    """mu > 0 only: the problem is singular at 0"""
    for which in ROUTES:
        rt = plain_route(tiny_problem(), which, [1], [1])
        sel = list(range(rt.nP))[::-1]
        for rule, mu in ((fr.NO_RULE, 1.0), (MQ, 1e-3)):
            e, tol, want = agree(rt, sel, mu, rule, 2.5)
            print(f"tiny {which} {rule}: {e:.3e} (allowed {tol:.3e})")
            assert e <= tol
            held = np.repeat(rt.held_pts[sel], 3)
            assert np.all(want[held] == 0.0) and np.all(want[:, held] == 0.0)


def test_the_two_statements_agree_on_7camsvarK_with_two_poses_held_at_mu_0():
    rt = p7("kd-bal")
    held = int(np.flatnonzero(rt.held_pts)[0])
    free = np.flatnonzero(~rt.held_pts.astype(bool))
    sel = [int(free[5]), held, int(free[0]), int(free[11]), int(free[3])]
    e, tol, want = agree(rt, sel, 0.0)
    print(f"7camsvarK kd-bal mu = 0: {e:.3e} (allowed {tol:.3e})")
    assert e <= tol and np.all(want[3:6] == 0.0) and np.all(np.diag(want)[[0, 6, 9, 12]] > 0.0)


def test_the_two_statements_agree_on_the_ring_with_priors():
    rt = ring()
    sel = [7, 2, 9, 0]
    for rule, mu in ((fr.NO_RULE, 0.0), (MQ, 1e-6)):
        e, tol, _ = agree(rt, sel, mu, rule, 3.0)
        print(f"ring {rule} mu = {mu}: {e:.3e} (allowed {tol:.3e})")
        assert e <= tol


@pytest.mark.parametrize("fault", sp.FAULTS)
def test_each_injected_fault_fails_the_agreement(fault):
    rt = p7("kd-bal")
    held = int(np.flatnonzero(rt.held_pts)[0])
    free = np.flatnonzero(~rt.held_pts.astype(bool))
    sel, rule, mu, scale = [int(free[5]), held, int(free[0]), int(free[11])], MQ, 1e-3, 2.5
    e, tol, _ = agree(rt, sel, mu, rule, scale)
    assert e <= tol
    e, tol, _ = agree(rt, sel, mu, rule, scale, fault)
    print(f"{fault}: {e:.3e} (allowed {tol:.3e})")
    assert e > tol


# ---- the device's judges on a float64 twin ------------------------------------------------------------------------------

def synthetic(name, c, seed=3):
    """a dominant system on a pattern, points with drawn tracks (1 camera, 2, all of them, none), Y and V drawn"""
    n_cams, blocks = fp.fpattern(name)
    rng = np.random.default_rng([seed, c, n_cams])
    S = fp.dominant(n_cams, blocks, 1e-2, c, 2.0, 5)
    lens = [1, 2, n_cams, 0, 3, min(4, n_cams), 2]
    cams = [np.sort(rng.choice(n_cams, size=m, replace=False)) for m in lens]
    ptr = np.r_[0, np.cumsum(lens)]
    j_of_obs = np.concatenate(cams).astype(np.int64)
    Y = rng.standard_normal((ptr[-1], c, 3)) * 10.0 ** rng.uniform(-3, 1, (ptr[-1], 1, 1))
    G = rng.standard_normal((len(lens), 3, 3))
    V = G @ np.transpose(G, (0, 2, 1)) + 0.1 * np.eye(3)
    held = np.zeros(len(lens), dtype=np.uint8)
    held[4] = 1
    jk = np.array(sorted([(j, j) for j in range(n_cams)] + list(blocks)))
    return dict(n_cams=n_cams, blocks=blocks, S=S, ptr=ptr, j=j_of_obs, Y=Y, V=V, held=held, jk=jk, c=c)


def plain_contraction(s, cols, sel, mu, rule, scale):
    """float64, the verb's rule: what a device does, in numpy's order"""
    n = len(sel)
    Vs = fc.damped_V(s["V"], mu, rule)
    C = np.zeros((3 * n, 3 * n))
    for b in range(n):
        for a in range(b, n):
            ia, ib = sel[a], sel[b]
            if s["held"][ia] or s["held"][ib]:
                continue
            T = np.zeros((3, 3))
            for o in range(s["ptr"][ia], s["ptr"][ia + 1]):
                r = slice(s["c"] * s["j"][o], s["c"] * s["j"][o] + s["c"])
                T = T + s["Y"][o].T @ cols[3 * b:3 * b + 3, r].T
            if a == b:
                T = T + np.linalg.inv(Vs[ia])
                T = np.tril(T) + np.tril(T, -1).T
            C[3 * a:3 * a + 3, 3 * b:3 * b + 3] = scale * T
            C[3 * b:3 * b + 3, 3 * a:3 * a + 3] = scale * T.T
    return C


@pytest.mark.parametrize("name,c", [("five", 11), ("five", 16), ("trip", 16)])
def test_twin_and_plain_contraction_meet_the_bounds(name, c):
    s = synthetic(name, c)
    sel, mu, scale = [2, 4, 0, 3, 6, 1, 5], 0.25, 4.0
    cols, iters, relres = sp.solve_columns(s["S"], s["n_cams"], s["blocks"], s["Y"], s["ptr"], s["j"], sel, s["held"], TOL,
                                           fp.MAXIT, c)
    op = fp.ListOp(s["n_cams"], s["jk"], fp.blocks_of(s["S"], s["jk"], c), c)
    J = sp.column_judges(op, cols, s["Y"], s["ptr"], s["j"], sel, s["held"], iters, TOL, c)
    solved = J[:, 2] > 0
    assert np.array_equal(solved, np.repeat([True, False, True, False, True, True, True], 3))   # held 4, empty 3
    assert np.all(iters[~solved] == 0) and np.all(relres[~solved] == 0.0) and np.all(iters[solved] > 0)
    assert np.all(relres[solved] <= TOL) and np.all(J[solved, 0] <= J[solved, 1])
    gap = np.abs(J[solved, 0] - relres[solved]) / ((J[solved, 1] - TOL) / sp.C_GAP)
    print(f"{name} c = {c}: worst residual / allowed {np.max(J[solved, 0] / J[solved, 1]):.3e}, "
          f"twin's gap on Y right-hand sides {gap.max():.3f} of a unit (C_GAP = {sp.C_GAP})")
    assert gap.max() <= sp.C_GAP
    want, bound = sp.contract(cols, s["V"], s["Y"], s["ptr"], s["j"], sel, s["held"], mu, MQ, scale, c)
    C = plain_contraction(s, cols, sel, mu, MQ, scale)
    ratio = sp.contract_ratio(C, want, bound)
    print(f"{name} c = {c}: plain float64 contraction / bound {ratio:.3e}")
    assert ratio <= 1.0
    info = dict(cols=cols, iters=iters, relres=relres)
    assert sp.exact_parts(C, info, sel, s["held"]) == []
    k = sel.index(3)                                                         # the point without observations: scale V*^-1
    assert np.all(want[3 * k:3 * k + 3, :3 * k] == 0) and np.all(bound[3 * k:3 * k + 3, :3 * k] == 0)
    for fault in ("no-vinv", "vinv-off-diagonal", "scale-twice", "held-vinv", "mu-identity"):
        bad, bb = sp.contract(cols, s["V"], s["Y"], s["ptr"], s["j"], sel, s["held"], mu, MQ, scale, c, fault=fault)
        assert sp.contract_ratio(C, bad, bb) > 1.0, fault
    skew = C.copy()
    skew[0, 1] = np.nextafter(skew[0, 1], np.inf)
    assert "C is not bit-symmetric" in sp.exact_parts(skew, info, sel, s["held"])


def test_the_entry_point_exists():
    from psba_amd import capi
    assert capi.lib.psba_sparse_point_covariance(None, 0.0, 1.0, 1, 0, None, None, None, None, None) == -1
    assert hasattr(capi.Psba, "sparse_point_covariance")
