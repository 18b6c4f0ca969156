"""The judges of tests/tr_ref.py on the host (no GPU): they pass the fp64 oracle twin's modified Cholesky
(oracle_lib.cholmod) on every matrix the GPU tests use, with no undecided comparison and the intended branches taken;
and they catch injected faults that the comparison of lambda with the twin (tests/test_gpu_trust_region.py) and the
1e-11-of-the-largest-magnitude rule for J x pass."""
import numpy as np
import pytest

import tr_ref as tr
from oracle_lib import cholmod

pytestmark = pytest.mark.skipif(not tr.LD_OK, reason="needs an 80-bit long double")

CASES = [(n, name) for n in tr.SIZES.values() for name in tr.matrices(n)]


def _twin(A):
    L, E, delta, beta = cholmod(A)
    return L, abs(E.sum()) / A.shape[0], delta, beta


def _judge(A, L, lam, delta, beta):
    """(worst ratios of (a) and (b), mirror result)"""
    r = tr.apost(A, L, lam, delta, beta)
    m = tr.mirror(A, L, delta, beta)
    r["diag"] = m["ratio"]
    return r, m


@pytest.mark.parametrize("n,name", CASES)
def test_twin_passes_the_judges(n, name):
    make, expect = tr.matrices(n)[name]
    A = make()
    assert np.array_equal(A, A.T)
    L, lam, delta, beta = _twin(A)
    r, m = _judge(A, L, lam, delta, beta)
    print(n, name, {k: f"{v:.2e}" for k, v in r.items()}, "one-column block columns", m["single"])
    assert all(v <= 1.0 for v in r.values()), r
    assert m["undecided"] == [], "change the seed of this matrix, not the threshold"
    log = m["log"]
    if expect == "none":
        assert m["single"] == 0
    elif expect == "some":
        assert m["single"] > 0
    elif expect[0] == "over":  # the first block column to leave the block route is Js, by the restore from the backup
        assert log[0][0] == expect[1] and log[0][1] == "over" and log[0][2]
    else:  # theta: the 3 x 3 factor fails at column js and that column takes theta / beta
        js = expect[1]
        assert log[0][0] == js - js % 3 and log[0][1] == "fail" and js in log[0][2]
    # the fp64 numpy form of k_cholmod (the carrier of the injected faults below) takes the same branches
    Lf, lamf, df, bf, single = tr.cholmod_f64(A)
    assert single == m["single"] and df == delta and bf == beta
    if n <= 324:
        rf, mf = _judge(A, Lf, lamf, df, bf)
        assert all(v <= 1.0 for v in rf.values()) and mf["single"] == single and mf["undecided"] == [], rf


# ---- faults -----------------------------------------------------------------------------------------------------------

def _old_rule(A, lam, delta, beta, single, indefinite):
    """what tests/test_gpu_trust_region.py asserts of a modified Cholesky"""
    _, want, d, b = _twin(A)
    ok = abs(delta - d) <= 1e-12 * d and abs(beta - b) <= 1e-12 * b
    ok = ok and abs(lam - want) <= 1e-9 * want + 1e-13 * np.abs(A).max()
    if indefinite:
        ok = ok and lam > 0 and single > 0
    return bool(ok)


def _old_matrices():
    """the matrices of tests/test_gpu_trust_region.py"""
    for n, seed0, shifts in ((42, 11, (-3.0, -40.0, 0.0)), (324, 5, (-3.0, -400.0, 0.0))):
        for s in shifts:
            B = np.random.default_rng(int(-s) + seed0).normal(size=(n, n))
            yield s, B @ B.T + s * np.eye(n)


def test_a_dropped_term_of_the_second_tile():
    """entry (1040, 1030) without its term k = 1024 (the first of k_cholmod_grid's second LDS tile): the row's later
    entries and its pivot absorb the error, E stays at rounding level and lambda with it"""
    A = tr.spd(1044, 3)
    L, lam, delta, beta, single = tr.cholmod_f64(A, ("drop", 1040, 1030, 1024))
    assert _old_rule(A, lam, delta, beta, single, False)
    assert tr.apost(A, L, lam, delta, beta)["LLt"] > 1e3


def test_a_block_column_not_restored():
    """the restore from the backup left out: the matrices of the lambda test never send a block column above beta
    after a successful 3 x 3 factor, so the faulty code returns what the correct one does there"""
    for s, A in _old_matrices():
        L, lam, delta, beta, single = tr.cholmod_f64(A, ("norestore", "all"))
        good = tr.cholmod_f64(A)
        assert np.array_equal(L, good[0])
        assert _old_rule(A, lam, delta, beta, single, s < 0)
        # why: no block column of these matrices leaves the block route by the comparison with beta
        m = tr.mirror(A, good[0], good[2], good[3])
        assert m["undecided"] == [] and m["single"] == good[4] and all(why == "fail" for _, why, _ in m["log"])
    # the fault is not inert: where a block column is restored, leaving every restore out changes the factor
    A = tr.matrices(42)["over21"][0]()
    assert not np.array_equal(tr.cholmod_f64(A, ("norestore", "all"))[0], tr.cholmod_f64(A)[0])
    A = tr.matrices(324)["over162"][0]()
    L, lam, delta, beta, single = tr.cholmod_f64(A, ("norestore", 162))
    r, m = _judge(A, L, lam, delta, beta)
    assert r["LLt"] > 1e3 and r["diag"] > 1e3


def test_a_nonzero_left_in_the_upper_triangle():
    A = tr.spd(42, 3)
    L, lam, delta, beta, single = tr.cholmod_f64(A, ("upper", 3, 17, 1e-300))
    assert _old_rule(A, lam, delta, beta, single, False)
    assert tr.apost(A, L, lam, delta, beta)["upper"] == np.inf


def test_fabs_in_the_beta_comparison():
    """|x| > beta instead of x > beta: the lambda test sees this one on two of its six matrices (a different damping),
    so it is not among the faults it misses; the mirror names the column: a diagonal entry theta / beta where the
    branch without fabs keeps sqrt(|d|)"""
    seen = [not _old_rule(A, *tr.cholmod_f64(A, ("fabs",))[1:], s < 0) for s, A in _old_matrices()]
    assert any(seen)
    A = tr.matrices(42)["shift3"][0]()
    L, lam, delta, beta, single = tr.cholmod_f64(A, ("fabs",))
    r, m = _judge(A, L, lam, delta, beta)
    assert r["LLt"] <= 1.0 and r["diag"] > 1e3  # (a).2 holds on either branch; the branch itself is wrong


def test_one_entry_of_jx_with_the_unwhitened_block(problems):
    """J x of the covariance-weighted model with one observation's B left unwhitened, in a vector whose entries for
    that camera and point are small (a step that barely moves them): 1e-11 of the largest magnitude passes it"""
    from lens_twin import Twin
    prob = problems["7cams"]
    nC, nP, nO = int(prob["nC"]), int(prob["nP"]), int(prob["nO"])
    rng = np.random.default_rng(6)
    G = rng.normal(size=(nO, 2, 2))
    cov = G @ np.transpose(G, (0, 2, 1)) + 0.5 * np.eye(2)[None]
    _, A, B = Twin(prob, None, cov).linearize()
    _, _, B0 = Twin(prob).linearize()
    iidx, jidx = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    nA = 6 * nC
    a = nO // 2
    x = rng.normal(size=nA + 3 * nP)
    x[6 * jidx[a]:6 * jidx[a] + 6] *= 1e-12
    x[nA + 3 * iidx[a]:nA + 3 * iidx[a] + 3] *= 1e-12

    def jx(Bm):
        return (np.einsum("akc,ac->ak", A, x[:nA].reshape(-1, 6)[jidx])
                + np.einsum("akc,ac->ak", Bm, x[nA:].reshape(-1, 3)[iidx])).reshape(-1)

    good = jx(B)
    Bf = B.copy()
    Bf[a] = B0[a]
    bad = jx(Bf)
    exact, bound = tr.jx_ref(A, B, x, iidx, jidx, nA)
    assert tr.ar.excess(good, exact, bound)[0] <= 1.0
    assert np.abs(bad - good).max() <= 1e-11 * np.abs(good).max()  # the rule of test_jmultiply_and_gradient
    assert tr.ar.excess(bad, exact, bound)[0] > 1e3


def test_dots_judge():
    rng = np.random.default_rng(8)
    r1, r2 = rng.normal(size=4001), rng.normal(size=4001)
    exact, bound = tr.dots_ref(r1, r2)
    got = np.array([r1 @ r1, r1 @ r2, r2 @ r2])
    assert tr.ar.excess(got, exact, bound)[0] <= 1.0
    got[1] += r1[17] * r2[17]  # one term twice
    assert tr.ar.excess(got, exact, bound)[0] > 1e3
