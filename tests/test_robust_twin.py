"""The robust-loss twin (tests/robust_twin.py) against its own definition, without a GPU: rho' against central
differences of rho, the IRLS gradient against central differences of F (distortion and non-diagonal covariances
on), and the lens twin as the limit of a huge scale."""
import numpy as np
import pytest

from psba_amd import synth
from lens_twin import Twin
from robust_twin import KINDS, RobustTwin, drho, rho

C = 2.0


@pytest.mark.parametrize("name", sorted(KINDS))
def test_drho_is_derivative_of_rho(name):
    kind = KINDS[name]
    # both sides of Huber's knee at s = c2 = 4 (not on it), from tiny to far-out residuals
    s = np.r_[np.geomspace(1e-4, 3.5, 20), np.geomspace(4.5, 1e4, 20)]
    h = 1e-6 * np.maximum(s, 1.0)
    fd = (rho(kind, C, s + h) - rho(kind, C, s - h)) / (2.0 * h)
    assert np.abs(fd - drho(kind, C, s)).max() <= 1e-7
    assert rho(kind, C, 0.0) == 0.0 and drho(kind, C, 0.0) == 1.0
    assert np.all(np.diff(rho(kind, C, s)) > 0) and np.all(drho(kind, C, s) <= 1.0)


def _lens_outlier_problem(seed=3):
    rng = np.random.default_rng(seed)
    base = synth.make_problem(6, 40, 4, seed=seed)
    prob, idx = synth.add_outliers(base, 0.1, 20.0, 80.0, seed)
    kc = np.column_stack([0.3 * np.ones(6), -0.2 * np.ones(6), 1e-3 * rng.normal(size=6),
                          1e-3 * rng.normal(size=6), 0.1 * rng.normal(size=6)])
    G = rng.normal(size=(prob["nO"], 2, 2))
    cov = G @ np.transpose(G, (0, 2, 1)) + 0.5 * np.eye(2)[None]
    return prob, idx, kc, cov


def test_add_outliers():
    base = synth.make_problem(6, 40, 4, seed=3)
    prob, idx = synth.add_outliers(base, 0.1, 20.0, 80.0, 3)
    assert idx.size == round(0.1 * base["nO"]) and np.all(np.diff(idx) > 0)
    d = np.linalg.norm(prob["impts"] - base["impts"], axis=1)
    assert np.all(d[idx] >= 20.0 - 1e-9) and np.all(d[idx] <= 80.0 + 1e-9)
    assert np.all(np.delete(d, idx) == 0.0)
    assert prob["impts"] is not base["impts"] and prob["nO"] == base["nO"]


@pytest.mark.parametrize("name", sorted(KINDS))
def test_gradient_is_half_minus_dF(name):
    prob, idx, kc, cov = _lens_outlier_problem()
    t = RobustTwin(prob, KINDS[name], C, kc, cov)
    s = t.sq_residuals()
    assert (s > C * C).sum() >= idx.size  # the outliers are in the down-weighted region
    g = t.gradient()
    p0 = np.r_[t.cams.reshape(-1), t.pts.reshape(-1)]
    nA = t.nA
    fd = np.empty_like(p0)
    for k in range(p0.size):
        h = 1e-6 * max(abs(p0[k]), 1e-2)
        pp, pm = p0.copy(), p0.copy()
        pp[k] += h
        pm[k] -= h
        fd[k] = (t.cost(pp[:nA], pp[nA:]) - t.cost(pm[:nA], pm[nA:])) / (2.0 * h)
    err = np.abs(-2.0 * g - fd).max() / np.abs(fd).max()
    assert err <= 1e-6, err


def test_huge_scale_is_the_lens_twin():
    prob, _, kc, cov = _lens_outlier_problem()
    lens = Twin(prob, kc, cov)
    e0, A0, B0 = lens.linearize()
    for kind in KINDS.values():
        t = RobustTwin(prob, kind, 1e12, kc, cov)
        e, A, B = t.linearize()
        for x, y in ((e, e0), (A, A0), (B, B0)):
            assert np.abs(x - y).max() <= 1e-13 * np.abs(y).max()
        assert abs(t.cost() - lens.cost()) <= 1e-12 * lens.cost()
