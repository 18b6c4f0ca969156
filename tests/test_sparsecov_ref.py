"""The host reference of psba_sparse_camera_covariance (tests/sparsecov_ref.py) against itself, without a GPU: the float64
twin of the multi-column solve meets the bounds the device is held to (b: the true residual of every column, c: C
against the refined inverse in sigma-units, e: the exact parts), and each of the three injected faults of the assembly
rule fails a judge."""
import numpy as np
import pytest

import freepcg_ref as fp
import sparsecov_ref as sc

TOL = 1e-12
CASES = [("five", 11, [3, 0]), ("five", 16, [1, 4, 2]), ("trip", 11, [12, 2, 16]), ("trip", 16, [16, 0])]


def system(name, c, dead_of):
    n_cams, blocks = fp.fpattern(name)
    S = fp.dominant(n_cams, blocks, 1e-2, c, 2.0, 5)
    live = np.ones(c * n_cams, dtype=bool)
    live[dead_of] = False
    return n_cams, blocks, sc.with_dead(S, np.flatnonzero(~live), S[dead_of[0], dead_of[0]]), live


def solved(name, c, sel):
    dead = [c * sel[0] + 1, c * sel[0] + c - 1, c * sel[-1] + 2, 0]
    n_cams, blocks, S, live = system(name, c, dead)
    cols, iters, relres = sc.solve_columns(S, n_cams, blocks, sel, live, TOL, fp.MAXIT, c)
    return S, live, cols, iters, relres


@pytest.mark.parametrize("name,c,sel", CASES)
def test_twin_meets_the_bounds(name, c, sel):
    S, live, cols, iters, relres = solved(name, c, sel)
    lv = live[sc.chosen_coords(sel, c)]
    assert np.all(relres[lv] <= TOL) and np.all(iters[lv] > 0) and np.all(iters[~lv] == 0)
    C, out = sc.assemble(cols, sel, live, 4.0, c)
    assert sc.exact_parts(C, out, sel, live, c) == []
    found, allowed = sc.column_residuals(S, out, sel, live, iters, TOL, c)
    print(f"{name} c = {c}: worst residual / allowed {np.max(found[lv] / allowed[lv]):.3e}")
    assert np.all(found <= allowed)
    j = sc.c_error_and_bound(S, C, sel, live, allowed, 4.0, c)
    print(f"{name} c = {c}: C found {j['found']:.3e}, allowed {j['allowed']:.3e}, kappa {j['kappa']:.3e}")
    assert j["ratio"] <= 1.0
    C1, _ = sc.assemble(cols, sel, live, 1.0, c)
    assert np.array_equal(C, 4.0 * C1)


@pytest.mark.parametrize("fault", sc.FAULTS)
def test_faults_fail_the_judges(fault):
    name, c, sel = CASES[1]
    S, live, cols, iters, relres = solved(name, c, sel)
    placeholder = S[0, 0]
    C, out = sc.assemble(cols, sel, live, 4.0, c, fault=fault, placeholder=placeholder)
    exact = sc.exact_parts(C, out, sel, live, c)
    found, allowed = sc.column_residuals(S, out, sel, live, iters, TOL, c)
    if fault == "dead-placeholder":
        assert "a dead coordinate's row or column of C is not +0.0" in exact
    elif fault == "no-mirror":
        assert "C is not bit-symmetric" in exact
    else:
        assert exact == [] and np.any(found > allowed)
