"""The trust-region operators of kernels_tr.hip entry by entry against the judges of tests/tr_ref.py.  Needs an MI355X.

Modified Cholesky: every matrix of tr_ref.matrices at 18, 42, 324 and 1044 columns (3, 7, 54 and 174 cameras of a
synthetic upload supply the sizes; 1044 gives k_cholmod_grid two LDS tiles and k_cholmod two passes of its row loops)
is put into the reduce buffer and factored by both routes (PSBA_CHOLMOD_GRID=0 / 1); the factor is read back with
psba_get_cholmod_factor.  Each route's factor is held to the a posteriori bounds (a) on its own and to the mirror (b), and the two routes must agree bit for bit in L,
delta, beta and the count of one-column block columns.  J x and its dot products: (d).  k_newp, k_newp_fixed and
k_pack_g: exact.  The module prints the worst bound ratio per route, size and quantity."""
import numpy as np
import pytest

import tr_ref as tr

ar = tr.ar
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not tr.LD_OK, reason="needs an 80-bit long double")]

WORST = {}  # (label, quantity) -> worst bound ratio
ROUTES = {"0": "one-wg", "1": "grid"}
CASES = [(nC, name) for nC, n in tr.SIZES.items() for name in tr.matrices(n)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        labels = sorted({r for r, _ in WORST})
        lines = [f"  {r}: " + ", ".join(f"{q} {v:.2e}" for (rr, q), v in WORST.items() if rr == r) for r in labels]
        print("\nworst bound ratio per route, size and quantity:\n" + "\n".join(lines))


def note(label, what, ratio):
    WORST[(label, what)] = max(WORST.get((label, what), 0.0), ratio)
    assert ratio <= 1.0, f"{label} {what}: bound ratio {ratio:.3e}"


def judge(label, what, got, exact, bound):
    r, k = ar.excess(np.asarray(got).reshape(np.shape(exact)), exact, bound)
    WORST[(label, what)] = max(WORST.get((label, what), 0.0), r)
    if not r <= 1.0:
        g, x, b = np.asarray(got).reshape(-1)[k], float(np.asarray(exact).reshape(-1)[k]), float(np.reshape(bound, -1)[k])
        raise AssertionError(f"{label} {what}: entry {k} = {g!r}, exact {x!r}, |diff| {abs(g - x):.3e} > bound {b:.3e} "
                             f"(ratio {r:.3e})")


# ---- modified Cholesky ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sized():
    """camera count -> (handle, n32): one upload per size"""
    import psba_amd
    from psba_amd import synth
    made = {}

    def get(nC):
        if nC not in made:
            h = psba_amd.Psba(0)
            h.upload_problem(synth.make_problem(nC, 4 * nC + 20, min(3.0, nC), seed=100 + nC))
            made[nC] = (h, h.chol_dist_shape()[0])
        return made[nC]
    yield get
    for h, _ in made.values():
        h.close()


def _factor(h, n32, A, route, monkeypatch):
    """(L, lambda, delta, beta, count) of A by the route ("0", "1", None = the library's choice)"""
    if route is None:
        monkeypatch.delenv("PSBA_CHOLMOD_GRID", raising=False)
    else:
        monkeypatch.setenv("PSBA_CHOLMOD_GRID", route)
    h.linearize(1.0, 1.0)
    h.schur_assemble(1.0)  # any assembly: makes the reduce buffer the current state
    h.set_reduce_buffer(tr.embed(A, n32))
    lam, info = h.cholmod_lambda(reassemble=False)
    return h.cholmod_factor(), lam, info[0], info[1], int(info[2])


def _judge_factor(label, A, got, with_mirror, same_as=None):
    """every ratio of one route's result, noted and asserted; same_as: (ratios, mirror) of a route that returned the
    same L, delta, beta and count bit for bit (only lambda, whose sum the routes order differently, is judged again)"""
    L, lam, delta, beta, count = got
    if same_as is not None:
        ratios, m = dict(same_as[0]), same_as[1]
        ratios["lambda"] = tr.lambda_ratio(A, L, lam)
    else:
        ratios, m = tr.apost(A, L, lam, delta, beta), None
        if with_mirror:
            m = tr.mirror(A, L, delta, beta)
            ratios["diag"] = m["ratio"]
    for what, r in ratios.items():
        note(label, what, r)
    if m is not None:
        assert m["undecided"] == [], f"{label}: undecided comparisons in the block columns {m['undecided']}"
        assert m["single"] == count, f"{label}: {count} one-column block columns, the mirror predicts {m['single']}"
    return ratios, m


@pytest.mark.parametrize("nC,name", CASES)
def test_modified_cholesky_entrywise(nC, name, sized, monkeypatch):
    n = tr.SIZES[nC]
    h, n32 = sized(nC)
    assert h.nA == n
    make, expect = tr.matrices(n)[name]
    A = make()
    with_mirror = True  # (both matrices at 1044 columns too: a few seconds of host time each)
    got = {r: _factor(h, n32, A, r, monkeypatch) for r in ROUTES}
    same = np.array_equal(got["0"][0], got["1"][0]) and got["0"][2:] == got["1"][2:]
    # each route is held to the bounds on its own
    first = _judge_factor(f"{ROUTES['0']} n={n}", A, got["0"], with_mirror)
    _judge_factor(f"{ROUTES['1']} n={n}", A, got["1"], with_mirror, same_as=first if same else None)
    # the header of kernels_tr.hip: every sum by one thread in the same order, the same factor bit for bit
    assert got["0"][2:] == got["1"][2:], (got["0"][2:], got["1"][2:])
    if not same:
        d = np.argwhere(got["0"][0] != got["1"][0])
        raise AssertionError(f"the routes differ in {len(d)} entries of L, the first at {tuple(d[0])}: "
                             f"{got['0'][0][tuple(d[0])]!r} / {got['1'][0][tuple(d[0])]!r}")
    count, m = got["0"][4], first[1]
    assert (count == 0) == (expect == "none"), count
    if m is not None and expect[0] == "over":
        assert m["log"][0][0] == expect[1] and m["log"][0][1] == "over" and m["log"][0][2]
    elif m is not None and expect[0] == "theta":
        js = expect[1]
        assert m["log"][0][0] == js - js % 3 and m["log"][0][1] == "fail" and js in m["log"][0][2]


@pytest.mark.parametrize("nC", [49, 50])
def test_default_route_at_the_threshold(nC, sized, monkeypatch):
    """launch_cholmod takes the grid from 50 cameras (300 columns) on: whichever it takes, the factor is the forced
    routes' bit for bit"""
    h, n32 = sized(nC)
    n = 6 * nC
    A = tr.shift(n, 3.0, 20 + nC)
    got = [_factor(h, n32, A, r, monkeypatch) for r in (None, "0", "1")]
    _judge_factor(f"default n={n}", A, got[0], True)
    for g in got[1:]:
        assert np.array_equal(g[0], got[0][0]) and g[2:] == got[0][2:]
    assert got[0][4] > 0


def test_factor_hook_refusals(problems):
    import psba_amd
    from psba_amd import capi
    prob = problems["7cams"]
    h = psba_amd.Psba(0)

    def refused(hh, word=None):
        with pytest.raises(capi.PsbaError) as ei:
            hh.cholmod_factor()
        assert ei.value.code == -6
        assert word is None or word in str(ei.value)

    with pytest.raises(capi.PsbaError) as ei:  # nothing uploaded
        h._ck(capi.lib.psba_get_cholmod_factor(h._h, None))
    assert ei.value.code == -6
    h.upload_problem(prob)
    refused(h, "psba_cholmod_lambda")  # before any psba_cholmod_lambda
    h.linearize(2.0, -2.0)
    h.cholmod_lambda()
    L = h.cholmod_factor()
    assert L.shape == (42, 42) and not np.triu(L, 1).any() and np.all(np.diag(L) > 0)
    assert np.array_equal(h.cholmod_factor(), L)  # reading it changes nothing
    h.linearize(2.0, -2.0)
    h.schur_assemble(1e-3 * h.max_diag())
    refused(h)  # the assembly may already factor the first diagonal block into the same buffer
    h.schur_reduce()
    h.schur_solve()
    refused(h, "psba_cholmod_lambda")  # after a psba_schur_solve
    h.cholmod_lambda()
    h.cholmod_factor()
    h.upload_problem(prob)
    refused(h)
    h.close()
    s = psba_amd.Psba(0)
    s.set_solver(1, 1e-12, 4000)
    s.upload_problem(prob)
    s.linearize(2.0, -2.0)
    s.cholmod_lambda()
    refused(s, "PSBA_SOLVER_PCG")
    s.close()


# ---- J x --------------------------------------------------------------------------------------------------------------

def _big_problem():
    from psba_amd import synth
    return synth.make_problem(40, 33000, 8.0, seed=31)


def _jx_case(case, problems):
    """(handle, problem, jac_slack, fixed entries of x or None)"""
    import psba_amd
    if case == "lens":  # distortion, covariances and Huber on 5 % outliers: the robust tests' default one-try case
        from test_gpu_assembly_entrywise import _handle, _jac_slack, _slack
        from test_gpu_robust import _one_try_case
        prob, kc, cov = _one_try_case("default")
        lens = (kc, cov, 2.0)
        h = _handle(prob, lens)
        return h, prob, _jac_slack(_slack(prob, h.compute_exQT(), lens), lens), None
    prob = _big_problem() if case == "big" else problems["54cams" if case == "fixed" else "trafalgar21"]
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    fixed = None
    if case == "fixed":
        from test_gpu_fixed import _mask
        fc, fp = _mask(prob)
        h.set_fixed(fc, fp)
        fixed = np.r_[np.repeat(fc != 0, 6), np.repeat(fp != 0, 3)]
    return h, prob, None, fixed


@pytest.mark.parametrize("case", ["plain", "lens", "fixed", "big"])
def test_jmultiply_entrywise(case, problems):
    h, prob, jac_slack, fixed = _jx_case(case, problems)
    nC, nP, nO = int(prob["nC"]), int(prob["nP"]), int(prob["nO"])
    if case == "big":  # past launch_jmul's 1024 workgroups of 256: the grid-stride loop, and a partly filled last turn
        assert nO > 262144 + 256 and nO % 256 != 0, nO
    nA = 6 * nC
    JA, JB = h.compute_jacobiQT()
    rng = np.random.default_rng(12)
    # entries of very different sizes, camera by camera and point by point: a bound from the largest magnitude of
    # the whole vector would say nothing about the small ones
    x = rng.normal(size=nA + 3 * nP) * np.r_[np.repeat(10.0 ** rng.uniform(-8, 2, nC), 6), np.repeat(10.0 ** rng.uniform(-8, 2, nP), 3)]
    y = rng.normal(size=x.size)
    label = f"jmul {case}"
    r1 = h.compute_Jmultiply(x)
    judge(label, "J x", r1, *tr.jx_ref(JA, JB, x, prob["iidx"], prob["jidx"], nA, jac_slack, fixed))
    r2 = h.compute_Jmultiply(y)
    judge(label, "J x", r2, *tr.jx_ref(JA, JB, y, prob["iidx"], prob["jidx"], nA, jac_slack, fixed))
    judge(label, "dots(x, y)", h.jmul_dots(x, y), *tr.dots_ref(r1, r2))
    judge(label, "dots(x)", h.jmul_dots(x), *tr.dots_ref(r1, r1))
    judge(label, "dots(x, x)", h.jmul_dots(x, x), *tr.dots_ref(r1, r1))
    h.close()


# ---- the exact kernels ------------------------------------------------------------------------------------------------

def test_newp_and_gradient_are_exact(problems):
    import psba_amd
    from psba_amd import capi
    prob = problems["54cams"]
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    cams, pts = h.get_params()
    p0 = np.r_[cams.reshape(-1), pts.reshape(-1)]
    rng = np.random.default_rng(3)
    dp = rng.normal(size=p0.size) * 10.0 ** rng.uniform(-12, 0, p0.size)
    h.set_step(dp)
    nc, npt = h.get_params(capi.PARAMS_NEW)
    assert np.array_equal(np.r_[nc.reshape(-1), npt.reshape(-1)], p0 + dp)  # k_newp: one IEEE add per entry
    assert np.array_equal(h.get_dp(), dp)
    # k_pack_g: a copy of g_a and of the tail of every point's record
    g = h.compute_g(-2.0)
    assert np.array_equal(h.get_gradient(), g)
    # k_newp_fixed: a fixed block's proposal is the current block, its entries of dp are zeroed whatever they held
    from test_gpu_fixed import _mask
    fc, fp = _mask(prob)
    h.set_fixed(fc, fp)
    fx = np.r_[np.repeat(fc != 0, 6), np.repeat(fp != 0, 3)]
    bad = dp.copy()
    bad[fx] = np.nan
    h.set_step(bad)
    nc, npt = h.get_params(capi.PARAMS_NEW)
    p1 = np.r_[nc.reshape(-1), npt.reshape(-1)]
    assert np.array_equal(p1[fx], p0[fx]) and np.array_equal(p1[~fx], (p0 + dp)[~fx])
    got = h.get_dp()
    assert np.all(got[fx] == 0.0) and not np.signbit(got[fx]).any() and np.array_equal(got[~fx], dp[~fx])
    h.close()
