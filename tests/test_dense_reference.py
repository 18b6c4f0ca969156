"""The host reference of the dense-solve tests (tests/dense_ref.py) checked against exact arithmetic and its own
claims, so that the GPU sweep (tests/test_gpu_dense_solve.py) judges the kernels with a yardstick that is itself
tested.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import dense_ref as dr


def _exact_residual(A, x, b):
    n = A.shape[0]
    return [Fraction(b[i]) - sum((Fraction(A[i, j]) * Fraction(x[j]) for j in range(n)), Fraction(0)) for i in range(n)]


@pytest.mark.parametrize("use_ld", [True, False] if dr.LD_OK else [False])
def test_extended_residual_is_exact_on_a_12x12_case(use_ld):
    """Entries of 20 significant bits: every product and partial sum fits the 64-bit significand of a long double
    (and a double-double), so the residual is the exact one rounded once -- bit for bit."""
    rng = np.random.default_rng(12)
    n = 12
    A = np.ldexp(rng.integers(-2**19, 2**19, size=(n, n)).astype(np.float64), -10)
    A = np.tril(A) + np.tril(A, -1).T
    x = np.ldexp(rng.integers(-2**19, 2**19, size=n).astype(np.float64), -12)
    # b = A x rounded, so the residual is all cancellation: the case where a double evaluation is worst
    b = np.array([float(v) for v in (sum(Fraction(A[i, j]) * Fraction(x[j]) for j in range(n)) for i in range(n))])
    b = np.nextafter(b, np.inf)
    want = np.array([float(v) for v in _exact_residual(A, x, b)])
    got = dr.residual(A, x, b, use_ld=use_ld)
    assert np.array_equal(got, want)
    assert np.any(got != 0)


@pytest.mark.parametrize("use_ld", [True, False] if dr.LD_OK else [False])
def test_extended_residual_on_full_precision_entries(use_ld):
    """Full 53-bit entries: within the error bound of the extended format (n eps_ext of the absolute terms; 2^-64 for
    the long double, ~2^-100 for the double-double)."""
    rng = np.random.default_rng(13)
    n = 12
    A = rng.standard_normal((n, n))
    x = rng.standard_normal(n)
    b = A @ x
    exact = _exact_residual(A, x, b)
    want = np.array([float(v) for v in exact])
    got = dr.residual(A, x, b, use_ld=use_ld)
    scale = np.abs(A) @ np.abs(x) + np.abs(b)
    eps_ext = 2.0**-63 if use_ld else 2.0**-100
    assert np.all(np.abs(got - want) <= n * eps_ext * scale + 1e-300)
    # and far better than a double evaluation could promise for this cancellation
    assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max()


def test_extended_residual_with_a_two_term_solution():
    rng = np.random.default_rng(14)
    n = 12
    A = rng.standard_normal((n, n))
    hi, lo = rng.standard_normal(n), 1e-17 * rng.standard_normal(n)
    b = rng.standard_normal(n)
    exact = [Fraction(b[i]) - sum((Fraction(A[i, j]) * (Fraction(hi[j]) + Fraction(lo[j])) for j in range(n)), Fraction(0))
             for i in range(n)]
    want = np.array([float(v) for v in exact])
    for use_ld in ([True, False] if dr.LD_OK else [False]):
        got = dr.residual(A, (hi, lo), b, use_ld=use_ld)
        assert np.abs(got - want).max() <= 1e-17 * np.abs(want).max()


def test_buffer_layout():
    n = 42
    buf = dr.lowrank_shift(n, 1e3, 1)
    n32 = dr.n32_of(n)
    assert buf.shape == (n32 + 1, n32)
    assert np.array_equal(buf[n:n32, n:], np.eye(n32 - n))
    assert not buf[n:n32, :n].any() and not buf[:n, n:].any()
    A = dr.matrix(buf, n)
    assert np.array_equal(A, A.T)
    b = np.arange(n, dtype=np.float64)
    dr.set_rhs(buf, n, b)
    assert np.array_equal(buf[-1, :n], b) and not buf[-1, n:].any()


@pytest.mark.parametrize("n,kappa", [(200, 1e2), (200, 1e6), (500, 1e10), (1000, 1e3)])
def test_lowrank_family_reaches_its_condition_number(n, kappa):
    A = dr.matrix(dr.lowrank_shift(n, kappa, 7), n)
    assert np.array_equal(A, A.T)
    k = dr.cond2(A)
    assert kappa / 2 <= k <= 2 * kappa
    assert np.all(A != 0)  # every tile dense


@pytest.mark.parametrize("n,kappa", [(96, 1e2), (300, 1e6), (300, 1e10)])
def test_spectrum_family_reaches_its_condition_number(n, kappa):
    A = dr.matrix(dr.spectrum(n, kappa, 8), n)
    assert np.array_equal(A, A.T)
    assert kappa / 2 <= dr.cond2(A) <= 2 * kappa


def test_graded_family_is_an_exact_scaling():
    n = 300
    buf, cbuf, d = dr.graded(n, 9)
    A, C = dr.matrix(buf, n), dr.matrix(cbuf, n)
    assert np.array_equal(A, A.T)
    assert np.array_equal(A / d[None, :] / d[:, None], C)
    e = np.log2(d)
    assert np.array_equal(e, np.round(e)) and e.min() >= -20 and e.max() <= 20 and e.max() - e.min() >= 30
    assert dr.cond2(C) <= 200
    dg = np.abs(np.diag(A))
    assert dg.max() / dg.min() > 1e16  # the spread shows in A (kappa(A) beyond what eigvalsh resolves), not in C


@pytest.mark.parametrize("n,k,pivot", [(100, 0, -1.0), (100, 31, 0.0), (100, 32, -1.0), (300, 257, 0.0),
                                       (300, 299, -1.0)])
def test_indefinite_family_fails_first_at_its_pivot(n, k, pivot):
    A = dr.matrix(dr.indefinite(n, k, 10, pivot), n)
    assert np.array_equal(A, A.T)
    assert dr.first_bad_pivot(A) == k
    if k > 0:
        np.linalg.cholesky(A[:k, :k])  # the leading block is SPD


@pytest.mark.parametrize("family,n,kappa", [("lowrank", 300, 1e3), ("lowrank", 1000, 1e6), ("spectrum", 300, 1e2),
                                            ("spectrum", 300, 1e6), ("spectrum", 300, 1e10), ("graded", 300, None)])
def test_refined_solution_has_a_tiny_backward_error(family, n, kappa):
    if family == "lowrank":
        buf = dr.lowrank_shift(n, kappa, 11)
    elif family == "spectrum":
        buf = dr.spectrum(n, kappa, 11)
    else:
        buf = dr.graded(n, 11)[0]
    A = dr.matrix(buf, n)
    b, xs = dr.rhs_for(A, 11)
    ref = dr.refined_solution(A, b)
    assert dr.backward_error(A, ref, b) < 1e-18
    # a plain double solve is not that good: the check measures something
    assert dr.backward_error(A, np.linalg.solve(A, b), b) > 1e-18
    if family != "graded":
        assert dr.forward_error(xs, ref) <= 2 * kappa * dr.EPS  # b = A x* rounded once: x* is that close


def test_right_hand_side_with_one_entry():
    b = dr.rhs_last(30, 2.5)
    assert b[-1] == 2.5 and np.count_nonzero(b) == 1
