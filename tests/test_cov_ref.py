"""The covariance of the estimate without a GPU (tests/cov_ref.py): the two statements of the model -- the
reduced dense inverse and the Schur formulas -- against each other, the extended-precision inverse that judges the
device, the per-entry judge of the point formula, and the new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

import psba_amd
from psba_amd import capi, synth
from conftest import DATA, ROOT
import cov_ref as cr
from fixed_twin import random_kc, random_spd
from robust_twin import KINDS
from sba_text import KK

EPS = cr.EPS


def _golden(n):
    return psba_amd.read_problem(os.path.join(DATA, f"{n}cams.txt"), os.path.join(DATA, f"{n}pts.txt"), KK)


def _mask(prob, seed=17, frac=0.1):
    fc = np.zeros(prob["nC"], dtype=bool)
    fc[[0, 1]] = True
    fp = np.zeros(prob["nP"], dtype=bool)
    fp[np.random.default_rng(seed).choice(prob["nP"], max(1, round(frac * prob["nP"])), replace=False)] = True
    return fc, fp


def _agree(t, mu, scale=1.0):
    """both statements, and the bound they must agree to: each is an fp64 inverse of a matrix of condition kappa (the
    Schur route's S and V are no worse conditioned than N), forward error c kappa eps each with c = 32 for the sizes here"""
    C, kappa = cr.dense_covariance(t, mu, scale)
    Caa, Cbb = cr.schur_covariance(t, mu, scale)
    tol = 64 * kappa * EPS
    assert tol < 1e-3, f"kappa = {kappa:.3e}: the bound would mean nothing"
    nA = t.nA
    ea = np.abs(Caa - C[:nA, :nA]).max() / np.abs(C[:nA, :nA]).max()
    blocks = np.stack([C[nA + 3 * i:nA + 3 * i + 3, nA + 3 * i:nA + 3 * i + 3] for i in range(t.nP)])
    eb = np.abs(Cbb - blocks).max() / np.abs(blocks).max()
    print(f"kappa {kappa:.2e}: cameras {ea:.2e}, points {eb:.2e} (bound {tol:.2e})")
    assert ea <= tol and eb <= tol
    return C, Caa, Cbb


@pytest.mark.parametrize("n", [7, 9])
@pytest.mark.parametrize("damped", [False, True])
def test_dense_and_schur_statements_agree(n, damped):
    prob = _golden(n)
    fc, fp = _mask(prob)
    t = cr.twin(prob, fc, fp)
    U, _, _ = cr.schur_pieces(t, 0.0)
    mu = 1e-6 * max(np.einsum("jkk->jk", U).max(), 0.0) if damped else 0.0
    C, Caa, Cbb = _agree(t, mu, scale=2.5)
    fx = t.fixed_entries()
    assert np.all(C[fx] == 0.0) and np.all(C[:, fx] == 0.0)
    assert np.all(Caa[:12] == 0.0) and np.all(Caa[:, :12] == 0.0) and np.all(Cbb[fp] == 0.0)
    assert np.all(np.linalg.eigvalsh(Caa[12:, 12:]) > 0.0)


def test_lens_covariance_huber_fixed_point_and_point_of_fixed_cameras():
    rng = np.random.default_rng(5)
    base = synth.make_problem(6, 40, 4, seed=5)
    prob, _ = synth.add_outliers(base, 0.1, 20.0, 80.0, 5)
    kc, cov = random_kc(rng, 6, k1=0.3), random_spd(rng, prob["nO"])
    p0 = 7  # the point whose cameras are all fixed
    fc = np.zeros(6, dtype=bool)
    fc[np.asarray(prob["jidx"])[np.asarray(prob["iidx"]) == p0]] = True
    assert 2 <= fc.sum() < 6
    fp = np.zeros(prob["nP"], dtype=bool)
    fp[[3, 11]] = True
    t = cr.twin(prob, fc, fp, kind=KINDS["huber"], c=2.0, kc=kc, cov=cov)
    scale = 1.7
    C, Caa, Cbb = _agree(t, 0.0, scale)
    assert np.all(Cbb[[3, 11]] == 0.0)
    _, Vs, _ = cr.schur_pieces(t, 0.0)
    want = scale * np.linalg.inv(Vs[p0])
    assert np.abs(Cbb[p0] - want).max() <= 8 * EPS * np.abs(want).max()
    nA = t.nA
    got = C[nA + 3 * p0:nA + 3 * p0 + 3, nA + 3 * p0:nA + 3 * p0 + 3]
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # the weights matter: the plain model gives another covariance
    plain = cr.schur_covariance(cr.twin(prob, fc, fp), 0.0, scale)[0]
    assert np.abs(plain - Caa).max() > 1e-3 * np.abs(Caa).max()


@pytest.mark.parametrize("n", [7, 9])
def test_refined_inverse_is_an_inverse_to_extended_precision(n):
    prob = _golden(n)
    fc, fp = _mask(prob)
    t = cr.twin(prob, fc, fp)
    U, Vs, W = cr.schur_pieces(t, 0.0)
    Vinv = np.zeros_like(Vs)
    Vinv[~fp] = np.linalg.inv(Vs[~fp])
    S = np.zeros((t.nA, t.nA))
    for j in range(t.nC):
        S[6 * j:6 * j + 6, 6 * j:6 * j + 6] = U[j]
    Y = W @ Vinv[t.i]
    for i in range(t.nP):
        obs = np.flatnonzero(t.i == i)
        for a in obs:
            for b in obs:
                S[6 * t.j[a]:6 * t.j[a] + 6, 6 * t.j[b]:6 * t.j[b] + 6] -= Y[a] @ W[b].T
    S = 0.5 * (S + S.T)
    free = np.repeat(~fc, 6)
    X, it = cr.embedded_inverse(S, free)
    kappa = np.linalg.cond(S[np.ix_(free, free)])
    print(f"{n} cameras: kappa(S) {kappa:.2e}, {it} iterations")
    assert it <= 8
    idx = np.flatnonzero(free)
    R = np.eye(idx.size, dtype=cr.LD) - S[np.ix_(idx, idx)].astype(cr.LD) @ X[np.ix_(idx, idx)]
    assert float(np.abs(R).max()) <= 1e-17 * kappa  # an fp64 inverse leaves about kappa eps = 2e-16 kappa
    assert np.all(X[~free] == 0) and np.all(X[:, ~free] == 0)
    lap = np.linalg.inv(S[np.ix_(idx, idx)])
    err = float(np.abs(lap - X[np.ix_(idx, idx)]).max() / np.abs(lap).max())
    assert err <= 64 * kappa * EPS  # ... and LAPACK's own inverse is within its forward bound of it


def test_point_judges_envelope_and_sum():
    rng = np.random.default_rng(2)
    iidx = np.array([0, 0, 0, 1, 2, 2])
    jidx = np.array([0, 1, 3, 2, 0, 2])
    Y = rng.normal(size=(6, 6, 3))
    G = rng.normal(size=(24, 24))
    Caa = G @ G.T
    Vinv = np.stack([np.eye(3) * (k + 1) for k in range(3)])
    J = cr.point_judges(iidx, jidx, Vinv, Y, Caa, 2.0, [0, 1, 2])
    for i in range(3):
        obs = np.flatnonzero(iidx == i)
        want = 2.0 * Vinv[i]
        for a in obs:
            for b in obs:
                want = want + Y[a].T @ Caa[6 * jidx[a]:6 * jidx[a] + 6, 6 * jidx[b]:6 * jidx[b] + 6] @ Y[b]
        got, bound, _ = J[i]
        assert np.all(np.abs(got - want) <= bound), i
        assert np.all(bound > 0) and np.all(bound <= 2 * (36 * obs.size ** 2 + 5) * EPS * 1e6)
        assert np.allclose(got, got.T, rtol=1e-13)


def test_every_covariance_symbol_of_the_header_is_exported():
    with open(os.path.join(ROOT, "include", "psba_hip.h")) as f:
        text = f.read()
    start = text.index("covariance of the refined cameras and points")
    end = text.index("which S-assembly route", start)
    names = re.findall(r"^int (psba_\w+)\(", text[start:end], flags=re.M)
    assert {"psba_covariance_compute", "psba_get_camera_covariance", "psba_get_covariance_matrix",
            "psba_get_point_covariance"} <= set(names)
    bound = {s[0] for s in capi.SIGNATURES}
    for name in names:
        assert hasattr(capi.lib, name), name
        assert name in bound, name
    # a null handle is refused, not dereferenced
    assert capi.lib.psba_covariance_compute(None, 0.0, 1.0, 1) == -1
    assert capi.lib.psba_get_point_covariance(None, None) == -1
