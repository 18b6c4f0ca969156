"""tests/freepcg_ref.py judged on the CPU, and the host-only plan hook of the block-sparse free-intrinsics route
(psba_blockprod_plan_rows_info / psba_blockprod_plan_rows): the stored blocks and the row walk the library derives from
the product plan, slot by slot against a numpy enumeration; the containers; numpy's own float64 product inside the
product bound; the families; the twin's stop rule; and the measured constants C_inv(11), C_inv(16) and C_gap."""
import functools

import numpy as np
import pytest

import dense_ref as dr
import freepcg_ref as fp
from freekd_twin import tiny_problem, wide_problem
from test_freekd_twin import P54

needs_ld = pytest.mark.skipif(not fp.LD_OK, reason="np.longdouble has no 64-bit significand here")
FAIL_AT = ("five", "band43", "arrow257")


# ---- the plan hook --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plan_input(name):
    if name in fp.PATTERNS_F:
        return fp.pattern_problem(*fp.fpattern(name))
    return {"tiny": tiny_problem, "P54": P54, "wide65": lambda: wide_problem(65)}[name]()


@pytest.mark.parametrize("name", ["tiny", "P54", "wide65", "hubs", "trip"])
def test_plan_rows_slot_by_slot(name):
    """The stored list is the plan's blocks plus a diagonal block for every camera without a product (28 on P54, one on
    wide_problem(65), camera 16 of `hubs` has products of its own), ascending in (j, k); diag_slot, rowptr and every row
    entry equal the enumeration; every stored off-diagonal block is walked once as stored and once transposed."""
    from psba_amd import capi
    p = plan_input(name)
    nC = p["nC"]
    got = capi.blockprod_plan(nC, p["nP"], p["iidx"], p["jidx"], 64)
    want = fp.rows_enumeration(nC, p["iidx"], p["jidx"])
    jk = got["jk"]
    assert np.array_equal(jk, want["jk"])
    assert got["diag_added"] == len(want["added"]) == {"P54": 28, "wide65": 1}.get(name, 0)
    key = jk[:, 0].astype(np.int64) * nC + jk[:, 1]
    assert np.all(np.diff(key) > 0) and np.all(jk[:, 1] <= jk[:, 0])              # ascending in (j, k), lower triangle
    assert np.array_equal(jk[got["diag_slot"]], np.stack([np.arange(nC)] * 2, 1))  # every diagonal is present
    have = {tuple(b) for b in got["blocks"]}
    assert have | {(j, j) for j in want["added"]} == {tuple(b) for b in jk} and len(have) + len(want["added"]) == len(jk)
    assert np.array_equal(got["diag_slot"], want["diag_slot"])
    assert np.array_equal(got["rowptr"], want["rowptr"])
    assert np.array_equal(got["rowent"], want["rowent"])
    slot, other, how = got["rowent"][:, 0], got["rowent"][:, 1] & 0x0fffffff, got["rowent"][:, 1] >> 28
    row = np.repeat(np.arange(nC), np.diff(got["rowptr"]))
    off = np.flatnonzero(jk[:, 0] != jk[:, 1])
    for h, (a, b) in ((0, (0, 1)), (1, (1, 0))):                                  # as stored: row j, other k; transposed: swapped
        sel = how == h
        assert np.array_equal(np.sort(slot[sel]), off)
        assert np.array_equal(row[sel], jk[slot[sel], a]) and np.array_equal(other[sel], jk[slot[sel], b])
    sel = how == 2
    assert np.array_equal(slot[sel], got["diag_slot"]) and np.array_equal(row[sel], other[sel])
    blocks = [(j, k) for j, k in jk if j != k]
    assert np.array_equal(np.diff(got["rowptr"]), fp.row_lengths(nC, blocks))


def test_trip_pattern_row_lengths():
    """`trip`: the walked rows of the hubs have 3 .. 9 entries -- both sides of one and of two trips of TRIP blocks"""
    n, blocks = fp.fpattern("trip")
    m = fp.row_lengths(n, blocks)
    assert fp.TRIP == 4 and m[10:].tolist() == [3, 4, 5, 6, 7, 8, 9]
    assert {fp.TRIP - 1, fp.TRIP, fp.TRIP + 1, 2 * fp.TRIP - 1, 2 * fp.TRIP, 2 * fp.TRIP + 1} <= set(m.tolist())


# ---- containers and bounds ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", fp.BLOCKS)
@pytest.mark.parametrize("name", ["three", "hubs", "trip"])
def test_containers_round_trip(name, c):
    n, blocks = fp.fpattern(name)
    S = fp.dominant(n, blocks, 1.0, c, 2.0, 1)
    jk = fp.lower_jk(n, blocks)[::-1]
    val = fp.blocks_of(S, jk, c)
    assert np.array_equal(fp.dense_of(n, jk, val, c), S)
    assert np.array_equal(fp.dense_of(n, jk, fp.poison_upper(val, jk, c), c), S)   # the upper triangles are not read
    assert all(not np.array_equal(val[b], val[b].T) for b, (j, k) in enumerate(jk) if j != k)


@needs_ld
@pytest.mark.parametrize("c", fp.BLOCKS)
@pytest.mark.parametrize("name", ["one", "five", "hubs", "trip", "band43", "arrow257"])
def test_float64_product_is_within_the_product_bound(name, c):
    n, blocks = fp.fpattern(name)
    S = fp.dominant(n, blocks, 1e-2, c, 2.0, 2)
    m = fp.entry_row_lengths(n, blocks, c)
    op = fp.BlockOp(S, n, blocks, c)
    for what, x in fp.product_vectors(n, c):
        exact = fp.spmv_exact(S, x)
        for y in (S @ x, op.times(x)):
            err = np.abs(y.astype(fp.LD) - exact).astype(np.float64)
            assert np.all(err <= fp.spmv_bound(S, x, m, c)), f"{name}, x = {what}"


@pytest.mark.parametrize("c", fp.BLOCKS)
def test_block_inverse_transcription(c):
    """M B = I to rounding on modest blocks; a masked coordinate (row and column zero off the diagonal) comes out with
    exact zeros in its row and column of M; a planted pivot is found in its block only."""
    n, blocks = fp.fpattern("five")
    S, kap, _ = fp.blockdiag(n, c, 0.0, 3)
    D = np.stack([S[c * j:c * j + c, c * j:c * j + c] for j in range(n)])
    for r in (0, c // 2, c - 1):
        D[1, r, :] = 0.0
        D[1, :, r] = 0.0
        D[1, r, r] = 1.0
    M, bad = fp.block_inverse(fp.poison_upper(D, [(j, j) for j in range(n)], c))
    assert not bad.any()
    for j in range(n):
        assert np.abs(M[j] @ D[j] - np.eye(c)).max() <= 64 * c * kap[j] * fp.EPS
    for r in (0, c // 2, c - 1):
        row = M[1, r].copy()
        row[r] = 0.0
        assert np.all(row == 0.0) and np.all(np.delete(M[1, :, r], r) == 0.0) and M[1, r, r] == 1.0
    S = fp.bad_diag(n, blocks, 3, c - 1, c)
    _, bad = fp.block_inverse(np.stack([S[c * j:c * j + c, c * j:c * j + c] for j in range(n)]))
    assert bad.tolist() == [j == 3 for j in range(n)]
    assert dr.first_bad_pivot(S[c * 3:c * 4, c * 3:c * 4]) == c - 1


# ---- families and the twin ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", fp.BLOCKS)
@pytest.mark.parametrize("name", FAIL_AT)
def test_failing_families_fail_where_they_say(name, c):
    n, blocks = fp.fpattern(name)
    b = fp.rhs(fp.dominant(n, blocks, 1.0, c, 0.0, 0), 1)
    for which in ("first", "last"):
        S, (j, k) = fp.indefinite_pd_diag(n, blocks, which, c)
        v = np.zeros(c * n)
        v[c * j], v[c * k] = 1.0, -1.0
        assert (j, k) in blocks and v @ S @ v == -2.0
        M, bad = fp.block_inverse(np.stack([S[c * q:c * q + c, c * q:c * q + c] for q in range(n)]))
        assert not bad.any()
        t = fp.twin_pcg(S, n, blocks, b, fp.TOL, fp.MAXIT, c)
        assert t["failed"] and t["iters"] < fp.MAXIT


@pytest.mark.parametrize("c", fp.BLOCKS)
def test_twin_stop_rule(c):
    n, blocks = fp.fpattern("band43")
    S = fp.dominant(n, blocks, 1.0, c, 0.0, 0)
    b = fp.rhs(S, 1)
    z = fp.twin_pcg(S, n, blocks, np.zeros(c * n), 1e-10, 50, c)
    assert z["converged"] and z["iters"] == 0 and z["relres"] == 0.0 and not z["x"].any()
    full = fp.twin_pcg(S, n, blocks, b, 1e-10, 50, c, keep_iterates=True)
    k = full["iters"]
    assert full["converged"] and full["hist"][k] <= 1e-10 < full["hist"][k - 1]
    at = fp.twin_pcg(S, n, blocks, b, 1e-10, k, c)
    assert at["converged"] and at["iters"] == k and np.array_equal(at["x"], full["x"])
    short = fp.twin_pcg(S, n, blocks, b, 1e-10, k - 1, c)
    assert short["exhausted"] and short["iters"] == k - 1 and np.array_equal(short["x"], full["iterates"][k - 2])
    assert fp.twin_pcg(S, n, blocks, b, 1e-10, 3, c)["exhausted"]                  # the GPU module's budget of 3


@needs_ld
@pytest.mark.parametrize("c", fp.BLOCKS)
def test_blockdiag_takes_one_iteration(c):
    for name in FAIL_AT:
        for grade in (0.0, 5.0):
            case = fp.blockdiag_case(name, grade, c)
            for dtype in (np.float64, fp.LD):
                t = fp.twin_pcg(case["S"], case["n_cams"], case["blocks"], case["b"], 1e-10, 50, c, dtype)
                assert t["converged"] and t["iters"] == 1, f"{name} grade {grade} {dtype}: {t['iters']}"


@needs_ld
@pytest.mark.parametrize("c", fp.BLOCKS)
def test_burst_edge_cases_exist_and_both_twins_stop_there(c):
    for k in fp.BURST_EDGES:
        case = fp.burst_case("band43", k, c)
        assert case is not None, f"blocks of {c}: no dominant system whose residual drops 4x at iteration {k}"
        h = case["hist"]
        assert h[k - 1] >= 4.0 * h[k] and h[k] < case["tol"] < h[k - 1]
        for dtype in (np.float64, fp.LD):
            t = fp.twin_pcg(case["S"], case["n_cams"], case["blocks"], case["b"], case["tol"], fp.MAXIT, c, dtype)
            assert t["converged"] and t["iters"] == k, f"blocks of {c}, k = {k} {dtype}: {t['iters']}"


# ---- the measured constants -----------------------------------------------------------------------------------------

@needs_ld
@pytest.mark.parametrize("c", fp.BLOCKS)
def test_c_inv_is_the_measured_one(c):
    worst = 0.0
    for name in FAIL_AT:
        for grade in (0.0, 5.0):
            case = fp.blockdiag_case(name, grade, c)
            t = fp.twin_pcg(case["S"], case["n_cams"], case["blocks"], case["b"], 1e-10, 50, c)
            worst = max(worst, float(fp.blockdiag_ratios(case, t["x"]).max()))
    print(f"\nblock inverse of {c}, float64 transcription: worst ratio {worst:.3f}, C_inv {fp.C_INV[c]}")
    assert abs(worst - fp.INV_RATIO[c]) <= 0.01 * fp.INV_RATIO[c]
    assert fp.next_pow2_above(4.0 * worst) == fp.C_INV[c]


@needs_ld
def test_c_gap_is_the_measured_one():
    for c in fp.BLOCKS:
        worst = 0.0
        for name in fp.GAP_PATTERNS:
            for delta, grade in fp.QUALITY:
                sy = fp.quality_system(name, delta, grade, c)
                t = sy["t64"]
                assert t["converged"]
                gap = abs(fp.true_relres(sy["S"], t["x"], sy["b"]) - t["relres"])
                worst = max(worst, gap / fp.gap_unit(sy["S"], t["x"], sy["b"], t["iters"]))
        print(f"\nresidual gap, float64 twin, blocks of {c}: worst ratio {worst:.3f}, C_gap {fp.C_GAP}")
        assert abs(worst - fp.GAP_RATIO[c]) <= 0.01 * fp.GAP_RATIO[c]
        assert fp.next_pow2_above(4.0 * worst) <= fp.C_GAP
    assert max(fp.next_pow2_above(4.0 * fp.GAP_RATIO[c]) for c in fp.BLOCKS) == fp.C_GAP
