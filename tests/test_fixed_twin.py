"""Fixed parameter blocks without a GPU: the twin (tests/fixed_twin.py) with the oracle's own sums against a dense
solve of the reduced system, its gradient against central differences of its own cost, the C entry point's refusal of
a null handle (the library only, as tests/test_host.py) and the sharding of the point mask."""
import os

import numpy as np
import pytest

import psba_amd
from psba_amd import capi, synth
from conftest import DATA
from fixed_twin import FixedTwin, fixed_pieces, masks
from robust_twin import KINDS
from sba_text import KK


def _mask(prob, seed=3, frac=0.1):
    """cameras 0 and 1 and a seeded tenth of the points"""
    rng = np.random.default_rng(seed)
    fp = np.zeros(prob["nP"], dtype=bool)
    fp[rng.choice(prob["nP"], max(1, round(frac * prob["nP"])), replace=False)] = True
    fc = np.zeros(prob["nC"], dtype=bool)
    fc[[0, 1]] = True
    return fc, fp


@pytest.mark.parametrize("n", [7, 9])
def test_twin_and_oracle_sums_match_reduced_dense_solve(n):
    """Two statements of the model: the embedded one (masked blocks through the oracle's own U, V, W, g, S and solve)
    and the reduced one (columns deleted, numpy.linalg.solve)."""
    prob = psba_amd.read_problem(os.path.join(DATA, f"{n}cams.txt"), os.path.join(DATA, f"{n}pts.txt"), KK)
    fc, fp = _mask(prob)
    t, _, lin = fixed_pieces(prob, fc, fp)
    fx = t.fixed_entries()
    assert np.all(lin["g"][fx] == 0.0)
    assert lin["maxdiag"] > 0
    mu = 1e-3 * lin["maxdiag"]
    ref = fixed_pieces(prob, fc, fp, mu=mu)[2]
    assert ref["ret"] == 0.0
    dp = ref["dp"]
    assert np.all(dp[fx] == 0.0)
    want = t.reduced_step(mu)
    err = np.abs(dp - want).max() / np.abs(want).max()
    print(f"{n} cameras: oracle step on masked blocks vs reduced dense solve: {err:.3e}")
    assert err <= 1e-12, err
    # the twin's own dense embedded system says the same
    own = t.step(mu)
    assert np.abs(own[fx]).max() == 0.0
    assert np.abs(own - want).max() <= 1e-12 * np.abs(want).max()
    # S: rows and columns of fixed cameras are zero off the diagonal, mu I on it; e_a zero there
    S, ea = ref["S"], ref["ea"]
    fa = fx[:t.nA]
    off = S[fa][:, ~fa]
    assert np.all(off == 0.0) and np.all(S[~fa][:, fa] == 0.0) and np.all(ea[fa] == 0.0)
    assert np.array_equal(S[fa][:, fa], mu * np.eye(int(fa.sum())))


def _lens_problem(seed=3):
    rng = np.random.default_rng(seed)
    base = synth.make_problem(6, 40, 4, seed=seed)
    prob, _ = synth.add_outliers(base, 0.1, 20.0, 80.0, seed)
    kc = np.column_stack([0.3 * np.ones(6), -0.2 * np.ones(6), 1e-3 * rng.normal(size=6),
                          1e-3 * rng.normal(size=6), 0.1 * rng.normal(size=6)])
    G = rng.normal(size=(prob["nO"], 2, 2))
    cov = G @ np.transpose(G, (0, 2, 1)) + 0.5 * np.eye(2)[None]
    return prob, kc, cov


@pytest.mark.parametrize("model", ["plain", "lens_cauchy"])
def test_gradient_against_central_differences(model):
    prob, kc, cov = _lens_problem()
    fc, fp = _mask(prob, frac=0.2)
    t = FixedTwin(prob, fc, fp) if model == "plain" else FixedTwin(prob, fc, fp, KINDS["cauchy"], 2.0, kc, cov)
    g = t.gradient()
    fx = t.fixed_entries()
    assert fx.sum() == 12 + 3 * fp.sum() and np.all(g[fx] == 0.0)
    p0 = np.r_[t.cams.reshape(-1), t.pts.reshape(-1)]
    nA = t.nA
    free = np.flatnonzero(~fx)
    fd = np.empty(free.size)
    for n, k in enumerate(free):
        h = 1e-6 * max(abs(p0[k]), 1e-2)
        pp, pm = p0.copy(), p0.copy()
        pp[k] += h
        pm[k] -= h
        fd[n] = (t.cost(pp[:nA], pp[nA:]) - t.cost(pm[:nA], pm[nA:])) / (2.0 * h)
    err = np.abs(-2.0 * g[free] - fd).max() / np.abs(fd).max()
    assert err <= 1e-6, err


def test_solve_lm_keeps_fixed_blocks():
    prob = synth.make_problem(6, 40, 4, seed=3, noise_px=1.0)
    fc, fp = _mask(prob, frac=0.2)
    t = FixedTwin(prob, fc, fp)
    F0 = t.cost()
    cams, pts, F = t.solve_lm(30)
    assert F < F0
    assert np.array_equal(cams[fc], t.cams[fc]) and np.array_equal(pts[fp], t.pts[fp])
    assert not np.array_equal(cams[~fc], t.cams[~fc])


def test_set_fixed_refuses_a_null_handle():
    """loads the library only: the symbol exists and checks its handle before anything else"""
    assert capi.lib.psba_set_fixed(None, None, None) == -1
    assert capi.lib.psba_fixed_counts(None, None, None) == -1
    assert hasattr(capi.Psba, "set_fixed") and hasattr(capi.Psba, "fixed_counts")


def test_shard_problem_slices_the_point_mask():
    prob = synth.make_problem(8, 120, 4, seed=9)
    fc, fp = _mask(prob)
    full = capi.Problem(prob, fixed_cams=fc, fixed_pts=fp)
    bounds = capi.partition_points(prob["nP"], prob["iidx"], 3)
    got = []
    for r in range(3):
        s = capi.shard_problem(full, 3, r)
        assert np.array_equal(s["fixed_cams"], fc)
        assert len(s["fixed_pts"]) == s["nP"] == bounds[r + 1] - bounds[r]
        assert np.array_equal(s["fixed_pts"], fp[bounds[r]:bounds[r + 1]])
        got.append(s["fixed_pts"])
    assert np.array_equal(np.concatenate(got), fp)
    # absent keys stay absent, a None mask stays None
    assert "fixed_pts" not in capi.shard_problem(prob, 3, 0)
    s = capi.shard_problem(capi.Problem(prob, fixed_cams=None, fixed_pts=None), 3, 1)
    assert s["fixed_cams"] is None and s["fixed_pts"] is None
    fcm, fpm = masks(prob, [0, 1], np.flatnonzero(fp))
    assert np.array_equal(fcm, fc) and np.array_equal(fpm, fp)
