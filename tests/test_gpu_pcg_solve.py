"""The block-sparse route (psba_set_solver PSBA_SOLVER_PCG, kernels_pcg.hip) on constructed systems, judged against
the extended-precision host reference tests/pcg_ref.py (which tests/test_pcg_ref.py judges on the CPU).

One handle per named block pattern on a problem that produces exactly that pattern; psba_linearize once, then per
matrix psba_schur_assemble (any mu: it opens the try) -> psba_set_sparse_S -> the verb under test:
  a. psba_sparse_S_times, the solve's product kernel, entry by entry within the summation bound, and with the same
     bits when the strict upper triangles of the diagonal blocks hold NaN;
  b. the block inverse: block-diagonal systems take one iteration and every camera's part of the solution lies within
     C_inv kappa_2(B_j) eps of the long-double block solve, in the norm of the grading (pcg_ref.C_INV says why);
  c. the stop rule at iterations 1, 7, 8, 9, 16, 17 -- both sides of a burst of eight and of the four-slot rotation;
  d. solve quality on graded diagonally dominant systems: reported against true residual, forward error, iterations;
  e. failures (a bad pivot of a chosen diagonal block, an indefinite S with positive definite diagonal blocks, NaN and
     Inf in S and e_a) are reported as PSBA_NOT_SPD and forgotten by the next solve;
  f. the upper triangle of a diagonal block is never read, and repeats give the same bits where one workgroup owns
     every sum;
  g. the Gershgorin margins of psba_cholmod_lambda, with the smallest planted in every lane;
  h. the verbs of the dense buffer and the Cholesky chain refuse the mode.
The worst ratios per pattern are printed at the end of the module."""
import numpy as np
import pytest

import dense_ref as dr
import pcg_ref as pr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pr.LD_OK, reason="np.longdouble has no 64-bit significand here")]

PSBA_OK, PSBA_NOT_SPD, PSBA_PCG_MAXIT, PSBA_E_STATE = 0, 1, 4, -6
NAMES = list(pr.PATTERNS)
FAIL_AT = ("five", "band43", "arrow257")
MU = 1.0  # of psba_schur_assemble and psba_backsub: plays no part, the blocks are overwritten


class Handle:
    """A PCG handle on the pattern problem of a named pattern, linearized once."""

    def __init__(self, name):
        import psba_amd
        from psba_amd import capi
        self.name = name
        self.n_cams, self.blocks = pr.pattern(name)
        self.nA = 6 * self.n_cams
        prob = pr.pattern_problem(self.n_cams, self.blocks)
        assert np.array_equal(capi.sparse_pattern(prob), pr.pattern_flags(self.n_cams, self.blocks))
        self.h = psba_amd.Psba(0)
        self.h.set_solver(1, tol=pr.TOL, max_iter=pr.MAXIT)
        self.h.upload_problem(prob)
        self.h.linearize(1.0, 1.0)
        self.h.schur_assemble(MU)
        self.jk = self.h.get_sparse_S()[0]
        want = sorted([(j, j) for j in range(self.n_cams)] + list(self.blocks))
        assert sorted(map(tuple, self.jk.tolist())) == want, f"{name}: the handle's block list is not the pattern"
        self.m = pr.entry_row_lengths(self.n_cams, self.blocks)

    def load(self, S, b, poison=False, val=None):
        """A fresh try holding S (or the block values val) and b."""
        self.h.schur_assemble(MU)
        if val is None:
            val = pr.blocks_of(S, self.jk)
        if poison:
            val = pr.poison_upper(val, self.jk)
        self.h.set_sparse_S(val, b)

    def solve(self, S, b, tol=pr.TOL, max_iter=pr.MAXIT, poison=False, val=None):
        """-> (rc of psba_schur_solve, x, iters, relres, PSBA_NOT_SPD bit of the try)"""
        self.h.set_solver(1, tol=tol, max_iter=max_iter)
        self.load(S, b, poison, val)
        rc = self.h.schur_solve()
        x = self.h.get_dp()[:self.nA].copy()
        iters, relres, _, _ = self.h.pcg_info()
        status = self.h.backsub(MU).status
        return rc, x, iters, relres, status & PSBA_NOT_SPD

    def good(self, what, sweep=0):
        """The first system of the solve-quality sweep on this handle, through all of its checks."""
        delta, grade = pr.QUALITY[sweep]
        sy = pr.system(self.name, delta, grade)
        rc, x, iters, relres, bad = self.solve(sy["S"], sy["b"])
        assert not bad, f"{self.name} {what}: PSBA_NOT_SPD on a good system"
        r = pr.judge_solve(sy, rc, x, iters, relres, what)
        note(self.name, "residual gap / allowed", r["gap"])
        note(self.name, "forward error / allowed", r["fwd"])
        note(self.name, "iterations - twin's", r["iters"])
        return x

    def close(self):
        self.h.close()


WORST = {}
_HANDLES = {}


def note(name, what, value):
    row = WORST.setdefault(name, {})
    row[what] = max(row.get(what, -np.inf), float(value))


def handle(name):
    if name not in _HANDLES:
        _HANDLES[name] = Handle(name)
    return _HANDLES[name]


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for c in _HANDLES.values():
        c.close()
    _HANDLES.clear()
    if WORST:
        print("\nworst ratios per pattern (1 = the bound):")
        for name, row in WORST.items():
            print(f"  {name:9s} " + ", ".join(f"{k} {v:.3g}" for k, v in row.items()))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- a. the product, entry by entry ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_product_entry_by_entry(name):
    c = handle(name)
    S = pr.dominant(c.n_cams, c.blocks, 1e-2, 2.0, 2)
    b = np.zeros(c.nA)
    c.load(S, b)
    ys = []
    for what, x in pr.product_vectors(c.n_cams):
        y = c.h.sparse_S_times(x)
        err = np.abs(y.astype(pr.LD) - pr.spmv_exact(S, x)).astype(np.float64)
        bound = pr.spmv_bound(S, x, c.m)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        note(name, "product / bound", ratio.max())
        i = int(np.argmax(ratio))
        assert ratio[i] <= 1.0, (f"{name}, x = {what}: y[{i}] (camera {i // 6}, lane {i % 6}, {c.m[i]} blocks in its row)"
                                 f" = {y[i]:.17e}, off by {err[i]:.3e}, bound {bound[i]:.3e}")
        ys.append(y)
    c.load(S, b, poison=True)  # NaN in the strict upper triangle of every diagonal block: never read
    for (what, x), y in zip(pr.product_vectors(c.n_cams), ys):
        assert bits_equal(c.h.sparse_S_times(x), y), f"{name}, x = {what}: the poisoned product differs"
    # the verb leaves a later solve alone
    c.good("after psba_sparse_S_times")


# ---- b. the block inverse ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAIL_AT)
@pytest.mark.parametrize("grade", [0.0, 5.0])
def test_block_inverse_solves_block_diagonal_systems_in_one_iteration(name, grade):
    c = handle(name)
    case = pr.blockdiag_case(name, grade)
    rc, x, iters, relres, bad = c.solve(case["S"], case["b"], tol=1e-10)
    assert rc == PSBA_OK and not bad and np.all(np.isfinite(x))
    assert iters == 1, f"{name} grade {grade}: {iters} iterations on a block-diagonal system (relres {relres:.3e})"
    ratio = pr.blockdiag_ratios(case, x) / pr.C_INV
    note(name, "block inverse / bound", ratio.max())
    j = int(np.argmax(ratio))
    assert ratio[j] <= 1.0, (f"{name} grade {grade}: camera {j} (kappa {case['kap'][j]:.1f}) is {ratio[j]:.2f} x "
                             f"C_inv kappa eps = {pr.C_INV * case['kap'][j] * pr.EPS:.2e} away from the block solve")


# ---- c. the stop at chosen iterations ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["band43", "arrow257"])
@pytest.mark.parametrize("k", pr.BURST_EDGES)
def test_stop_at_chosen_iteration(name, k):
    c = handle(name)
    case = pr.burst_case(name, k)
    assert case is not None
    tol = case["tol"]
    kappa, ref = pr.burst_reference(case)
    rc, x, iters, relres, bad = c.solve(case["S"], case["b"], tol=tol)
    print(f"\n{name} k = {k}: delta {case['delta']:.4g}, tol {tol:.3e}, twin {case['hist'][k - 1]:.3e} -> "
          f"{case['hist'][k]:.3e}; iters {iters}, relres {relres:.3e}")
    assert rc == PSBA_OK and not bad
    assert iters == k, f"{name}: stopped after {iters} iterations, the twin after {k}"
    assert relres <= tol
    fe = dr.forward_error(x, ref)
    note(name, "stop: forward error / allowed", fe / (2 * kappa * (tol + 1e-14)))
    assert fe <= 2 * kappa * (tol + 1e-14), f"{name} k = {k}: forward error {fe:.3e}, kappa {kappa:.2f}"
    rc2, x2, iters2, relres2, _ = c.solve(case["S"], case["b"], tol=tol, max_iter=k)
    assert rc2 == PSBA_OK and iters2 == k and relres2 <= tol, f"max_iter = {k}: rc {rc2}, {iters2}, {relres2:.3e}"
    assert dr.forward_error(x2, ref) <= 2 * kappa * (tol + 1e-14)
    if k > 1:  # (max_iter = 0 keeps the handle's value: a budget of zero cannot be asked for)
        rc3, x3, iters3, relres3, bad3 = c.solve(case["S"], case["b"], tol=tol, max_iter=k - 1)
        assert rc3 == PSBA_PCG_MAXIT and not bad3, f"max_iter = {k - 1}: rc {rc3}"
        assert iters3 == k - 1 and relres3 > tol
        assert abs(relres3 - case["hist"][k - 1]) <= 1e-3 * case["hist"][k - 1] + 1e-15


# ---- d. solve quality ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_solve_quality(name):
    c = handle(name)
    for sweep in range(len(pr.QUALITY)):
        c.good(f"(delta, grade) = {pr.QUALITY[sweep]}", sweep)


# ---- e. failures are reported and forgotten --------------------------------------------------------------------------------

def expect_failure(c, what, S, b, val=None, max_iter=pr.MAXIT):
    rc, x, iters, relres, bad = c.solve(S, b, val=val, max_iter=max_iter)
    assert rc != PSBA_PCG_MAXIT and iters < pr.MAXIT, f"{c.name} {what}: ran its budget out ({iters} iterations)"
    assert bad, f"{c.name} {what}: passed for a solve (rc {rc}, {iters} iterations, relres {relres})"
    c.good(f"after {what}")


@pytest.mark.parametrize("name", FAIL_AT)
def test_bad_diagonal_block_is_reported(name):
    c = handle(name)
    b = pr.system(name, *pr.QUALITY[0])["b"]
    for j in (0, c.n_cams // 2, c.n_cams - 1):
        for col in (0, 5):
            expect_failure(c, f"bad pivot {col} of diagonal block {j}", pr.bad_diag(c.n_cams, c.blocks, j, col), b)


@pytest.mark.parametrize("name", FAIL_AT)
def test_indefinite_with_positive_definite_diagonal_blocks_is_reported(name):
    c = handle(name)
    b = pr.system(name, *pr.QUALITY[0])["b"]
    for which in ("first", "middle", "last"):
        S, pair = pr.indefinite_pd_diag(c.n_cams, c.blocks, which)
        expect_failure(c, f"indefinite on the {which} pair {pair}", S, b)


@pytest.mark.parametrize("name", FAIL_AT)
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_input_is_reported(name, value):
    c = handle(name)
    sy = pr.system(name, *pr.QUALITY[0])
    val = pr.blocks_of(sy["S"], c.jk)
    off = [i for i, (j, k) in enumerate(c.jk) if j != k]
    diag = [i for i, (j, k) in enumerate(c.jk) if j == k]
    v = val.copy()
    v[off[len(off) // 2], 2, 3] = value
    expect_failure(c, f"{value} in an off-diagonal block", None, sy["b"], val=v)
    v = val.copy()
    v[diag[len(diag) // 2], 4, 1] = value
    expect_failure(c, f"{value} in the lower triangle of a diagonal block", None, sy["b"], val=v)
    b = sy["b"].copy()
    b[c.nA // 2] = value
    expect_failure(c, f"{value} in e_a", None, b, val=val)
    if np.isinf(value):
        # p.Sp = +Inf passes the curvature test (alpha = 0, r = NaN) and is met one iteration later -- unless the budget
        # ends there: a NaN residual at the end of the budget is a failure too, not an exhausted budget.  One of the two
        # signs gives +Inf.
        for sign in (1.0, -1.0):
            v = val.copy()
            v[off[len(off) // 2], 2, 3] = sign * value
            expect_failure(c, f"{sign * value} in an off-diagonal block, max_iter = 1", None, sy["b"], val=v, max_iter=1)


# ---- f. the upper triangle is not read; repeats ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_upper_triangle_is_not_read_and_repeats_agree(name):
    c = handle(name)
    sy = pr.system(name, *pr.QUALITY[1])
    first = c.solve(sy["S"], sy["b"])
    again = c.solve(sy["S"], sy["b"])
    poisoned = c.solve(sy["S"], sy["b"], poison=True)
    for what, (rc, x, iters, relres, bad) in (("first", first), ("repeat", again), ("poisoned", poisoned)):
        assert not bad, f"{name} {what}: PSBA_NOT_SPD"
        pr.judge_solve(sy, rc, x, iters, relres, what)
    if name in pr.SMALL:  # one workgroup owns every sum: the order is fixed
        assert bits_equal(again[1], first[1]) and again[2:4] == first[2:4], f"{name}: a repeat differs"
        assert bits_equal(poisoned[1], first[1]) and poisoned[2:4] == first[2:4], f"{name}: the poisoned solve differs"
    # the Gershgorin walk reads the same half
    c.load(sy["S"], sy["b"])
    lam, info = c.h.cholmod_lambda(reassemble=False)
    c.load(sy["S"], sy["b"], poison=True)
    lam_p, info_p = c.h.cholmod_lambda(reassemble=False)
    assert bits_equal(np.array([lam]), np.array([lam_p])) and bits_equal(info, info_p), f"{name}: {info} vs {info_p}"


# ---- g. Gershgorin, row by row ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["five", "rows", "hubs", "arrow257"])
def test_gershgorin_margin_in_every_lane(name):
    c = handle(name)
    base = pr.dominant(c.n_cams, c.blocks, 1.0, 0.0, 3)
    b = np.zeros(c.nA)
    # diagonally dominant: the documented fallback, 1e-6 of the largest margin
    d, bound = pr.gershgorin_exact(base, c.m)
    c.load(base, b)
    lam, info = c.h.cholmod_lambda(reassemble=False)
    assert info[0] > 0 and abs(np.float64(info[0] - d.min())) <= bound[int(np.argmin(d))]
    assert d.max() - bound[int(np.argmax(d))] <= info[1] <= (d + bound).max()
    assert lam == 1e-6 * info[1] and info[2] == 0.0
    for cam in (0, c.n_cams - 1):  # camera 0 of the arrow is the row of 257 blocks, most of them read transposed
        for lane in range(6):
            row = 6 * cam + lane
            S = pr.plant_margin(base, row)
            d, bound = pr.gershgorin_exact(S, c.m)
            assert int(np.argmin(d)) == row and d[row] < 0
            c.load(S, b)
            lam, info = c.h.cholmod_lambda(reassemble=False)
            err = abs(np.float64(info[0] - d[row]))
            note(name, "margin / bound", err / bound[row])
            assert err <= bound[row], (f"{name}: smallest margin planted in camera {cam} lane {lane}: {info[0]:.17e}, "
                                       f"exact {float(d[row]):.17e}, bound {bound[row]:.3e}")
            assert lam == -info[0]
            assert d.max() - bound[int(np.argmax(d))] <= info[1] <= (d + bound).max()
    c.good("after psba_cholmod_lambda")


# ---- h. the dense verbs refuse the mode --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["five", "band43"])
def test_dense_verbs_refuse_the_block_sparse_mode(name):
    from psba_amd.capi import PsbaError
    c = handle(name)
    sy = pr.system(name, *pr.QUALITY[0])
    c.load(sy["S"], sy["b"])
    h = c.h
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
        "psba_covariance_compute": lambda: h.covariance(reassemble=False),
    }
    for verb, call in verbs.items():
        with pytest.raises(PsbaError) as e:
            call()
        assert e.value.code == PSBA_E_STATE, f"{verb}: {e.value}"
        assert "PSBA_SOLVER_PCG" in str(e.value), f"{verb} refused without naming the mode: {e.value}"
    # the refusals changed nothing: the try that was open still solves its system
    rc = h.schur_solve()
    x = h.get_dp()[:c.nA].copy()
    iters, relres, _, _ = h.pcg_info()
    assert not (h.backsub(MU).status & PSBA_NOT_SPD)
    pr.judge_solve(sy, rc, x, iters, relres, "after the refusals")
    c.good("after the refusals, a new try")
