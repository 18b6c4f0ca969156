"""CPU self-tests of tests/assembly_ref.py (no GPU): exactness on dyadic inputs, calibration against the fp64 oracle
(an independent code: its rounding must fit every envelope), and power (faults of 1e-6 in small entries, 1e-9 in U's
rotation rows, one product left out, one observation twice must all fail the entrywise check -- and the S faults pass
today's normwise close(..., 1e-11), the gap the entrywise check closes)."""
import numpy as np
import pytest

import assembly_ref as ar
from oracle_lib import Oracle

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

WORST = {}  # worst bound ratio per quantity over the calibration problems, printed at the end


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\noracle worst bound ratio per quantity: " + ", ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


def close_passes(got, want, tol):
    """today's check in test_gpu_parity.py: max|got - want| <= tol max|want|"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() <= tol * np.abs(want).max()


def ratio(got, exact, bound):
    return ar.excess(got, exact, bound)[0]


# ---- exactness ---------------------------------------------------------------------------------------------------

def test_dyadic_k1_and_schur_by_hand():
    """Two cameras, one point seen by both; every input a small dyadic number, so every sum is exact in fp64 too."""
    A = np.zeros((2, 2, 6))
    A[0, 0, :] = [1, 2, 0, 0, 0, 0.5]
    A[0, 1, :] = [0, 1, 1, 0, 0, 0]
    A[1, 0, :] = [0, 0, 0, 2, 0, 0]
    A[1, 1, :] = [1, 0, 0, 0, 0, 1]
    B = np.array([[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 0, 0]]], dtype=np.float64)
    e = np.array([[1.0, -2.0], [0.5, 0.25]])
    iidx, jidx = np.array([0, 0]), np.array([0, 1])
    k1 = ar.k1_sums(A, B, e, iidx, jidx, 2, 1, coeff=2.0, coeff_g=-2.0)
    for name, want in [("U", 2 * np.stack([A[0].T @ A[0], A[1].T @ A[1]])),
                       ("V", 2 * (B[0].T @ B[0] + B[1].T @ B[1])[None]),
                       ("W", 2 * np.stack([A[0].T @ B[0], A[1].T @ B[1]])),
                       ("g", -2 * np.r_[A[0].T @ e[0], A[1].T @ e[1], B[0].T @ e[0] + B[1].T @ e[1]])]:
        x, env = k1[name]
        assert np.array_equal(x.astype(np.float64), want), name
        assert np.all(env >= 0) and np.all(env <= 1e-13 * (1 + np.abs(want))), name
    V = k1["V"][0].astype(np.float64)  # [[4, 0, 0], [0, 2, 0], [0, 0, 2]]: inverse diag(1/4, 1/2, 1/2)
    X, envX = ar.vinv(V)
    assert np.array_equal(X.astype(np.float64)[0], np.diag([0.25, 0.5, 0.5]))
    U = k1["U"][0].astype(np.float64)
    W = k1["W"][0].astype(np.float64)
    g = k1["g"][0].astype(np.float64)
    ref = ar.schur(U, W, V, g, iidx, jidx, 2, 1)
    Y = W @ np.diag([0.25, 0.5, 0.5])
    S = np.zeros((12, 12))
    for ja in range(2):
        for jb in range(2):
            S[6 * ja:6 * ja + 6, 6 * jb:6 * jb + 6] = (U[ja] if ja == jb else 0) - Y[ja] @ W[jb].T
    blk, _ = ar.dense_to_blocks(S, ref["jk"])
    assert np.array_equal(ref["S"].astype(np.float64), blk)
    ea = g[:12] - np.concatenate([Y[0] @ g[12:], Y[1] @ g[12:]])
    assert np.array_equal(ref["ea"].astype(np.float64), ea)
    dpa = np.arange(12, dtype=np.float64) / 4
    eb, _ = ar.eb_ref(g, dpa, iidx, jidx, 2, 1, W=W)
    assert np.array_equal(eb.astype(np.float64), g[12:] - W[0].T @ dpa[:6] - W[1].T @ dpa[6:])


def test_cancellation_ea_matches_double_double():
    """e_a of a camera whose terms cancel to 1e-9 of their size, through ar.schur: one camera, 300 points seen once
    each, V_i = diag(2^k) (so V_i^-1 and Y_a = W_a V_i^-1 are exact in fp64) and g_a chosen so that g_a - sum Y_a g_b
    cancels.  The long-double e_a agrees with the error-free double-double evaluation of tests/dense_ref.py."""
    import dense_ref as dr
    rng = np.random.default_rng(5)
    n = 300
    iidx, jidx = np.arange(n), np.zeros(n, dtype=np.int64)
    W = rng.standard_normal((n, 6, 3)) * np.ldexp(1.0, rng.integers(-10, 10, size=(n, 1, 1)))
    d = np.ldexp(1.0, rng.integers(-4, 5, size=(n, 3)))
    V = np.zeros((n, 3, 3))
    V[:, np.arange(3), np.arange(3)] = d
    gb = rng.standard_normal((n, 3))
    Y = W / d[:, None, :]  # exact: division by powers of two
    t = np.einsum("art,at->r", ar.ld(Y), ar.ld(gb))
    ga = (t * ar.LD(1 + 1e-9)).astype(np.float64)
    g = np.r_[ga, gb.reshape(-1)]
    U = np.eye(6)[None] * 1e3
    ref = ar.schur(U, W, V, g, iidx, jidx, 1, n)
    M = Y.transpose(1, 0, 2).reshape(6, 3 * n)  # row r: Y_a[r, t] over (a, t)
    dd = dr.residual(M, gb.reshape(-1), ga, use_ld=False)
    got = ref["ea"].astype(np.float64)
    assert np.all(np.abs(got - dd) <= 1e-6 * np.abs(dd)), (got, dd)
    assert ar.excess(dd, ref["ea"], ref["ea_env"])[0] <= 1.0


# ---- calibration and power on the oracle's own fp64 intermediates ------------------------------------------------

def _synth_venice():
    import psba_amd.synth as synth
    return synth.venice_shaped(n_pts=12000, cluster=16)


class Walk:
    """One LM damping try of the oracle and the reference built from its inputs."""

    def __init__(self, prob):
        o = Oracle(prob)
        self.o, self.nC, self.nP, self.nA = o, o.nC, o.nP, o.nA
        self.iidx, self.jidx = o.iidx, o.jidx
        self.lin = lin = o.linearize()
        self.mu = 1e-3 * lin["maxdiag"]
        self.sch = sch = o.schur(lin, self.mu)
        ret, self.dp, self.eab = o.solve(lin, sch)
        assert ret == 0.0
        self.k1 = ar.k1_sums(lin["JA"], lin["JB"], lin["ex"], o.iidx, o.jidx, o.nC, o.nP)
        self.ref = ar.schur(sch["Ustar"], lin["W"], sch["Vstar"], lin["g"], o.iidx, o.jidx, o.nC, o.nP)
        self.S = sch["S"]
        self.eb = ar.eb_ref(lin["g"], self.dp[:o.nA], o.iidx, o.jidx, o.nC, o.nP, W=lin["W"])
        self.dpb = ar.dpb_ref(self.ref["Vinv"], self.ref["Vinv_env"], self.eab[o.nA:])

    def ratios(self, S=None, U=None, dpb=None):
        lin, sch, ref = self.lin, self.sch, self.ref
        out = {}
        for name in ("U", "V", "W", "g"):
            got = U if (name == "U" and U is not None) else lin[name]
            x, env = self.k1[name]
            out[name] = ratio(np.asarray(got).reshape(x.shape), x, env)
        out["Vinv"] = ratio(sch["Vinv"].reshape(-1, 3, 3), ref["Vinv"], ref["Vinv_env"])
        out["Y"] = ratio(sch["Y"].reshape(-1, 6, 3), ref["Y"], ref["Y_env"])
        blk, _ = ar.dense_to_blocks(self.S if S is None else S, ref["jk"])
        out["S"] = ratio(blk, ref["S"], ref["S_env"])
        rest = ar.outside_blocks(self.S if S is None else S, ref["jk"], self.nC)
        out["S zeros"] = 0.0 if not np.any(rest) else np.inf
        out["ea"] = ratio(sch["eab"][:self.nA], ref["ea"], ref["ea_env"])
        out["eb"] = ratio(self.eab[self.nA:], *self.eb)
        out["dpb"] = ratio(self.dp[self.nA:] if dpb is None else dpb, *self.dpb)
        return out


_WALKS = {}


def walk(name, problems):
    if name not in _WALKS:
        _WALKS[name] = Walk(_synth_venice() if name == "venice12000" else problems[name])
    return _WALKS[name]


CAL = ["7cams", "54cams", "trafalgar21", "venice12000"]


@pytest.mark.parametrize("name", CAL)
def test_oracle_fits_every_envelope(name, problems):
    w = walk(name, problems)
    r = w.ratios()
    for k, v in r.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(f"\n{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{name}: the oracle's fp64 rounding exceeds the envelope in {bad}"


def _fault_S_smallest_block_entry(w):
    S = w.S.copy()
    ref = w.ref
    mags = np.abs(ref["S"].astype(np.float64)).max(axis=(1, 2))
    b = int(np.argmin(np.where(mags > 0, mags, np.inf)))
    j, k = ref["jk"][b]
    blk = S[6 * j:6 * j + 6, 6 * k:6 * k + 6]
    r, c = np.unravel_index(int(np.argmax(np.abs(blk))), (6, 6))
    S[6 * j + r, 6 * k + c] *= 1 + 1e-6
    return S


def _fault_S_component01(w):
    S = w.S.copy()
    for j, k in w.ref["jk"]:
        S[6 * j, 6 * k + 1] *= 1 + 1e-6
    return S


def _fault_S_product_left_out(w):
    """The smallest of all products Y_a W_b^T (by its largest entry) added back: left out of its block's sum."""
    a, b = ar._pairs(w.iidx, w.nP)
    Y = w.sch["Y"].reshape(-1, 6, 3)
    W = w.lin["W"].reshape(-1, 6, 3)
    mags = np.einsum("prt,pct->prc", Y[a], W[b])
    m = np.abs(mags).max(axis=(1, 2))
    q = int(np.argmin(np.where(m > 0, m, np.inf)))
    S = w.S.copy()
    j, k = w.jidx[a[q]], w.jidx[b[q]]
    S[6 * j:6 * j + 6, 6 * k:6 * k + 6] += mags[q]
    return S


def _fault_U_observation_twice(w):
    A = w.lin["JA"].reshape(-1, 2, 6)
    U = w.lin["U"].reshape(-1, 6, 6).copy()
    a = w.o.nO // 2
    U[w.jidx[a]] += A[a].T @ A[a]
    return U


def _fault_U_rows(w):
    U = w.lin["U"].reshape(-1, 6, 6).copy()
    U[:, :3, :] *= 1 + 1e-9
    return U


def _fault_dpb_point(w):
    dpb = w.dp[w.nA:].copy()
    i = w.nP // 2
    dpb[3 * i:3 * i + 3] *= 1 + 1e-6
    return dpb


# fault -> (what it breaks, the problems on which today's close(..., 1e-11; dp 1e-9) passes it)
FAULTS = {
    "S smallest block entry 1e-6": ("S", _fault_S_smallest_block_entry, {"trafalgar21"}),
    "S (0,1) of every block 1e-6": ("S", _fault_S_component01, {"54cams"}),
    "S smallest product left out": ("S", _fault_S_product_left_out, set()),
    "U one observation twice": ("U", _fault_U_observation_twice, set()),
    "dp_b of one point 1e-6": ("dpb", _fault_dpb_point, set()),
    "U rows 0-2 1e-9": ("U", _fault_U_rows, set()),
}


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("name", CAL[1:3])
def test_injected_fault_fails_the_entrywise_check(name, fault, problems):
    w = walk(name, problems)
    what, inject, close_passes_on = FAULTS[fault]
    bad = inject(w)
    r = w.ratios(**{what: bad})
    key = what
    assert r[key] > 1.0, f"{name}: fault '{fault}' passes the entrywise check (ratio {r[key]:.2e})"
    want = {"S": w.S, "U": w.lin["U"].reshape(-1, 6, 6), "dpb": w.dp[w.nA:]}[what]
    tol = 1e-9 if what == "dpb" else 1e-11
    passes = close_passes(bad, want, tol)
    assert passes == (name in close_passes_on), \
        f"{name}: today's close(..., {tol:g}) {'passes' if passes else 'fails'} '{fault}'"
    print(f"\n{name} {fault}: entrywise ratio {r[key]:.2e}, today's close {'passes' if passes else 'fails'}")
