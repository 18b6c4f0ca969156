"""tests/pcg_ref.py judged on the CPU: every condition tests/test_gpu_pcg_solve.py relies on is shown here to hold for
the reference alone -- the pattern problems have the named patterns and row lengths, numpy's own float64 product
satisfies the product bound, the families are what they say, the twin converges, stops and fails where the GPU tests
expect the kernels to, and the two measured constants are the ones on record."""
import numpy as np
import pytest

import dense_ref as dr
import pcg_ref as pr

needs_ld = pytest.mark.skipif(not pr.LD_OK, reason="np.longdouble has no 64-bit significand here")
NAMES = list(pr.PATTERNS)
FAIL_AT = ("five", "band43", "arrow257")


# ---- patterns and containers ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_pattern_problem_has_the_named_pattern(name):
    from psba_amd import capi
    n, blocks = pr.pattern(name)
    prob = pr.pattern_problem(n, blocks)
    assert np.array_equal(capi.sparse_pattern(prob), pr.pattern_flags(n, blocks))
    assert prob["nO"] == len(prob["iidx"]) == len(prob["jidx"]) and prob["nC"] == n


def test_named_row_lengths():
    full = lambda name: pr.row_lengths(*pr.pattern(name))  # noqa: E731
    for name, n in (("one", 1), ("two", 2), ("three", 3), ("five", 5)):
        assert full(name).tolist() == [n] * n  # fewer rows than a workgroup's four waves; 5 % 4 != 0
    assert 6 * pr.PATTERNS["band43"][0] == 258  # the second workgroup of the vector kernels holds two threads
    assert set(full("band43").tolist()) == {4, 5, 6, 7}
    # `rows`: camera j shares with its j % 20 predecessors -- 1..20 stored blocks per row, 20 walked ones everywhere
    assert pr.stored_row_lengths(*pr.pattern("rows")).tolist() == [1 + j % 20 for j in range(40)]
    assert set(full("rows").tolist()) == {20}
    # `hubs`: the walked rows on both sides of the stride of eight
    h = full("hubs")
    assert h[16] == 1 and h[17:].tolist() == [7, 8, 9, 16, 17] and set(h.tolist()) >= {1, 2, 3, 7, 8, 9, 16, 17}
    assert 6 * max(pr.PATTERNS[s][0] for s in pr.SMALL) <= 256
    for name, n in (("arrow257", 257), ("arrow260", 260)):
        m = full(name)
        assert m[0] == n and set(m[1:].tolist()) == {3, 4}
        assert (n + 3) // 4 == 65  # 65 workgroups of the product: slot 0 of p.Sp gets two adds
    assert 260 % 4 == 0 and 257 % 4 == 1


@pytest.mark.parametrize("name", ["three", "hubs", "band43"])
def test_containers_round_trip(name):
    n, blocks = pr.pattern(name)
    S = pr.dominant(n, blocks, 1.0, 2.0, 1)
    jk = pr.lower_jk(n, blocks)[::-1]  # any order of the list
    val = pr.blocks_of(S, jk)
    assert np.array_equal(pr.dense_of(n, jk, val), S)
    assert np.array_equal(pr.dense_of(n, jk, pr.poison_upper(val, jk)), S)  # the upper triangles are not read
    off = [b for b, (j, k) in enumerate(jk) if j != k]
    assert all(not np.array_equal(val[b], val[b].T) for b in off)  # a transposed read shows


# ---- bounds ---------------------------------------------------------------------------------------------------------

@needs_ld
@pytest.mark.parametrize("name", NAMES)
def test_float64_product_is_within_the_product_bound(name):
    n, blocks = pr.pattern(name)
    S = pr.dominant(n, blocks, 1e-2, 2.0, 2)
    m = pr.entry_row_lengths(n, blocks)
    for what, x in pr.product_vectors(n):
        err = np.abs((S @ x).astype(pr.LD) - pr.spmv_exact(S, x)).astype(np.float64)
        assert np.all(err <= pr.spmv_bound(S, x, m)), f"{name}, x = {what}"


@needs_ld
@pytest.mark.parametrize("name", ["five", "hubs", "arrow257"])
def test_float64_margins_are_within_the_gershgorin_bound(name):
    n, blocks = pr.pattern(name)
    S = pr.plant_margin(pr.dominant(n, blocks, 1.0, 0.0, 3), 6 * n - 2)
    d, bound = pr.gershgorin_exact(S, pr.entry_row_lengths(n, blocks))
    assert int(np.argmin(d)) == 6 * n - 2 and d.min() < 0
    d64 = np.diag(S) - (np.abs(S).sum(axis=1) - np.abs(np.diag(S)))
    assert np.all(np.abs(d64.astype(pr.LD) - d).astype(np.float64) <= bound)


# ---- families -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_dominant_is_positive_definite(name):
    n, blocks = pr.pattern(name)
    for delta, grade in pr.QUALITY:
        S = pr.dominant(n, blocks, delta, 0.0, 0)
        assert np.array_equal(S, S.T) and np.linalg.eigvalsh(S)[0] > 0  # before the grading, by Gershgorin
        G = pr.dominant(n, blocks, delta, grade, 0)
        assert np.array_equal(G, G.T)
        for j in range(n):
            assert dr.first_bad_pivot(G[6 * j:6 * j + 6, 6 * j:6 * j + 6]) is None


@pytest.mark.parametrize("name", FAIL_AT)
def test_blockdiag_is_positive_definite_with_modest_blocks(name):
    n, _ = pr.pattern(name)
    for grade in (0.0, 5.0):
        S, kap, d = pr.blockdiag(n, grade, 3)
        assert kap.max() <= 100.0 * (1 + 1e-12) and np.array_equal(S, S.T)
        for j in range(n):
            s = slice(6 * j, 6 * j + 6)
            B = S[s, s] / np.outer(d[s], d[s])
            assert np.linalg.eigvalsh(B)[0] > 0
            S[s, s] = 0.0
        assert not S.any()  # off-diagonal blocks exactly zero


@pytest.mark.parametrize("name", FAIL_AT)
def test_failing_families_fail_where_they_say(name):
    n, blocks = pr.pattern(name)
    for which in ("first", "middle", "last"):
        S, (j, k) = pr.indefinite_pd_diag(n, blocks, which)
        assert (j, k) in blocks and np.linalg.eigvalsh(S)[0] < 0
        for c in range(n):
            assert dr.first_bad_pivot(S[6 * c:6 * c + 6, 6 * c:6 * c + 6]) is None
        t = pr.twin_pcg(S, n, blocks, pr.rhs(pr.dominant(n, blocks, 1.0, 0.0, 0), 1), pr.TOL, pr.MAXIT)
        assert t["failed"] and t["iters"] < pr.MAXIT
    for j in (0, n // 2, n - 1):
        for c in (0, 5):
            S = pr.bad_diag(n, blocks, j, c)
            for cam in range(n):
                want = c if cam == j else None
                assert dr.first_bad_pivot(S[6 * cam:6 * cam + 6, 6 * cam:6 * cam + 6]) == want
            _, bad = pr.block_inverse(np.stack([S[6 * q:6 * q + 6, 6 * q:6 * q + 6] for q in range(n)]))
            assert bad.tolist() == [q == j for q in range(n)]


# ---- the twin -------------------------------------------------------------------------------------------------------

@needs_ld
@pytest.mark.parametrize("name", NAMES)
def test_twin_passes_the_solve_checks_itself(name):
    for delta, grade in pr.QUALITY:
        sy = pr.system(name, delta, grade)
        t = sy["t64"]
        assert t["converged"] and not t["failed"] and t["iters"] < pr.MAXIT
        assert sy["t80"]["converged"]
        pr.judge_solve(sy, 0, t["x"], t["iters"], t["relres"], f"twin ({delta}, {grade})")


def test_twin_stop_rule():
    n, blocks = pr.pattern("band43")
    S = pr.dominant(n, blocks, 1.0, 0.0, 0)
    b = pr.rhs(S, 1)
    z = pr.twin_pcg(S, n, blocks, np.zeros(6 * n), 1e-10, 50)
    assert z["converged"] and z["iters"] == 0 and z["relres"] == 0.0 and not z["x"].any()  # r.z == 0: solved
    full = pr.twin_pcg(S, n, blocks, b, 1e-10, 50, keep_iterates=True)
    k = full["iters"]
    assert full["converged"] and full["hist"][k] <= 1e-10 < full["hist"][k - 1] and len(full["iterates"]) == k
    assert np.array_equal(full["iterates"][-1], full["x"])
    at = pr.twin_pcg(S, n, blocks, b, 1e-10, k)
    assert at["converged"] and at["iters"] == k and np.array_equal(at["x"], full["x"])
    short = pr.twin_pcg(S, n, blocks, b, 1e-10, k - 1)
    assert short["exhausted"] and short["iters"] == k - 1 and short["relres"] > 1e-10
    assert np.array_equal(short["x"], full["iterates"][k - 2])


@needs_ld
@pytest.mark.parametrize("name", FAIL_AT)
def test_blockdiag_takes_one_iteration(name):
    for grade in (0.0, 5.0):
        c = pr.blockdiag_case(name, grade)
        for dtype in (np.float64, pr.LD):
            t = pr.twin_pcg(c["S"], c["n_cams"], c["blocks"], c["b"], 1e-10, 50, dtype)
            assert t["converged"] and t["iters"] == 1, f"{name} grade {grade} {dtype}: {t['iters']}"


@needs_ld
@pytest.mark.parametrize("name", ["band43", "arrow257"])
def test_burst_edge_cases_exist_and_both_twins_stop_there(name):
    for k in pr.BURST_EDGES:
        c = pr.burst_case(name, k)
        assert c is not None, f"{name}: no dominant system whose residual drops 4x at iteration {k}"
        h = c["hist"]
        assert h[k - 1] >= 4.0 * h[k] and h[k] < c["tol"] < h[k - 1]
        assert pr.precond_cond(c["S"], c["n_cams"]) <= 100.0
        for dtype in (np.float64, pr.LD):
            t = pr.twin_pcg(c["S"], c["n_cams"], c["blocks"], c["b"], c["tol"], pr.MAXIT, dtype)
            assert t["converged"] and t["iters"] == k, f"{name} k = {k} {dtype}: {t['iters']}"
        assert pr.twin_pcg(c["S"], c["n_cams"], c["blocks"], c["b"], c["tol"], k - 1)["exhausted"]


# ---- the measured constants ----------------------------------------------------------------------------------------

@needs_ld
def test_c_inv_is_the_measured_one():
    worst = 0.0
    for name in FAIL_AT:
        for grade in (0.0, 5.0):
            c = pr.blockdiag_case(name, grade)
            t = pr.twin_pcg(c["S"], c["n_cams"], c["blocks"], c["b"], 1e-10, 50)
            worst = max(worst, float(pr.blockdiag_ratios(c, t["x"]).max()))
    print(f"\nblock inverse, float64 transcription: worst ratio {worst:.3f}, C_inv {pr.C_INV}")
    assert abs(worst - pr.INV_RATIO) <= 0.01 * pr.INV_RATIO
    assert pr.next_pow2_above(4.0 * worst) == pr.C_INV


@needs_ld
def test_c_gap_is_the_measured_one():
    worst = 0.0
    for name in NAMES:
        for delta, grade in pr.QUALITY:
            sy = pr.system(name, delta, grade)
            t = sy["t64"]
            gap = abs(pr.true_relres(sy["S"], t["x"], sy["b"]) - t["relres"])
            worst = max(worst, gap / pr.gap_unit(sy["S"], t["x"], sy["b"], t["iters"]))
    print(f"\nresidual gap, float64 twin: worst ratio {worst:.3f}, C_gap {pr.C_GAP}")
    assert abs(worst - pr.GAP_RATIO) <= 0.01 * pr.GAP_RATIO
    assert pr.next_pow2_above(4.0 * worst) == pr.C_GAP
