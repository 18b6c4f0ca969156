"""CPU self-tests of tests/fixed_ref.py (no GPU): calibration -- the oracle's fp64 sums on the masked blocks
(fixed_twin.fixed_pieces) must fit every envelope of the reference with the placeholder rule installed (the oracle
has 0 there, mu once damped) -- and power: faults a masked kernel could have must fail the entrywise or the exact
check.  For each fault the test records whether today's normwise check of tests/test_gpu_fixed.py lets it through."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import fixed_ref as fr
from fixed_twin import fixed_pieces
from lens_twin import Twin, oracle_pieces
from oracle_lib import Oracle
from robust_twin import RobustTwin

pytestmark = pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")

WORST = {}
PLACE = 0.0  # what the oracle's sums hold in the diagonal block of a fixed camera or point


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\noracle on masked blocks, worst bound ratio per quantity: "
              + ", ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


def close_passes(got, want, tol):
    """fixed_twin.close as a predicate: max|got - want| <= tol max|want|"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.abs(got - want).max() <= tol * np.abs(want).max())


def ratio(got, exact, bound):
    return ar.excess(np.asarray(got).reshape(np.shape(exact)), exact, bound)[0]


def cam_of_max(prob):
    """the camera that holds the largest diagonal entry of the unmasked U"""
    e, A, B = Twin(prob).linearize()
    U = oracle_pieces(prob, e, A, B)["U"].reshape(-1, 6, 6)
    return int(np.argmax(np.diagonal(U, axis1=1, axis2=2).max(axis=1)))


class MaskedWalk:
    """One damping try of the oracle on the masked blocks under the mixed mask, and the reference of its inputs."""

    def __init__(self, prob):
        self.prob = prob
        self.fc, self.fp, self.info = fr.mixed_mask(prob, cam_of_max(prob))
        fc, fp = self.fc, self.fp
        self.t, (e, A, B), lin = fixed_pieces(prob, fc, fp)
        self.e, self.A, self.B, self.lin = e, A, B, lin
        o = self.o = Oracle(prob)
        self.nC, self.nP, self.nA = o.nC, o.nP, o.nA
        self.iidx, self.jidx = np.asarray(o.iidx, dtype=np.int64), np.asarray(o.jidx, dtype=np.int64)
        self.fx = fr.fixed_entries(fc, fp)
        self.mu = 1e-3 * lin["maxdiag"]
        self.sch = sch = o.schur(lin, self.mu)
        ret, self.dp, self.eab = o.solve(lin, sch)
        assert ret == 0.0
        self.k1 = fr.install(ar.k1_sums(lin["JA"], lin["JB"], lin["ex"], o.iidx, o.jidx, o.nC, o.nP), fc, fp, PLACE)
        self.ref = ar.schur(sch["Ustar"], lin["W"], sch["Vstar"], lin["g"], o.iidx, o.jidx, o.nC, o.nP)
        self.eb = ar.eb_ref(lin["g"], self.dp[:o.nA], o.iidx, o.jidx, o.nC, o.nP, W=lin["W"])
        self.dpb = ar.dpb_ref(self.ref["Vinv"], self.ref["Vinv_env"], self.eab[o.nA:])
        self.newp = np.r_[self.t.cams.reshape(-1), self.t.pts.reshape(-1)] + self.dp
        e_new = o.exQT(self.newp[:o.nA], self.newp[o.nA:])
        self.s_new = (ar.ld(e_new).reshape(-1, 2) ** 2).sum(axis=1)
        self.scal = ar.try_scalars(self.dp, self.newp, self.mu, lin["g"], o.nA, self.s_new)

    def ratios(self, U=None, V=None, g=None, S=None, dpb=None):
        lin, sch, ref = self.lin, self.sch, self.ref
        out = {}
        for name, repl in (("U", U), ("V", V), ("W", None), ("g", g)):
            out[name] = ratio(lin[name] if repl is None else repl, *self.k1[name])
        for name, base, fixed in (("U*", "U", self.fc), ("V*", "V", self.fp)):
            x, env = fr.damped(*self.k1[base], self.mu, fixed, PLACE)
            out[name] = ratio(sch[name[0] + "star"], x, env)
        out["Vinv"] = ratio(sch["Vinv"], ref["Vinv"], ref["Vinv_env"])
        out["Y"] = ratio(sch["Y"], ref["Y"], ref["Y_env"])
        Sd = self.sch["S"] if S is None else S
        out["S"] = ratio(ar.dense_to_blocks(Sd, ref["jk"])[0], ref["S"], ref["S_env"])
        out["S zeros"] = np.inf if np.any(ar.outside_blocks(Sd, ref["jk"], self.nC)) else 0.0
        out["ea"] = ratio(sch["eab"][:self.nA], ref["ea"], ref["ea_env"])
        out["eb"] = ratio(self.eab[self.nA:], *self.eb)
        out["dpb"] = ratio(self.dp[self.nA:] if dpb is None else dpb, *self.dpb)
        return out


@functools.lru_cache(maxsize=None)
def _walk_of(name, loader):
    return MaskedWalk(loader(name))


def walk(name, problems):
    return _walk_of(name, problems.__getitem__)


# ---- the layer itself ------------------------------------------------------------------------------------------------

def test_placeholder_rule_by_hand():
    """two cameras, two points, camera 1 and point 0 fixed: the blocks, the zero envelopes and the once-rounded sum"""
    rng = np.random.default_rng(3)
    iidx, jidx = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])
    fc, fp = np.array([0, 1], dtype=np.uint8), np.array([1, 0], dtype=np.uint8)
    A = rng.normal(size=(4, 2, 6)) * (fc[jidx] == 0)[:, None, None]
    B = rng.normal(size=(4, 2, 3)) * (fp[iidx] == 0)[:, None, None]
    e = rng.normal(size=(4, 2))
    raw = ar.k1_sums(A, B, e, iidx, jidx, 2, 2, 2.0, -2.0)
    assert not np.any(raw["U"][0][1]) and not np.any(raw["U"][1][1]) and not np.any(raw["V"][1][0])
    assert not np.any(raw["W"][1][[0, 1, 3]]) and np.all(raw["W"][1][2] > 0)  # only (camera 0, point 1) is free-free
    for owner, want in ((True, 2.0), (False, 0.0)):
        k1 = fr.install(raw, fc, fp, 2.0, owner=owner)
        assert np.array_equal(k1["U"][0][1].astype(np.float64), want * np.eye(6)) and not np.any(k1["U"][1][1])
        assert np.array_equal(k1["V"][0][0].astype(np.float64), 2.0 * np.eye(3)) and not np.any(k1["V"][1][0])
        fx = fr.fixed_entries(fc, fp)
        assert not np.any(k1["g"][0][fx]) and not np.any(k1["g"][1][fx]) and np.all(k1["g"][1][~fx] > 0)
        assert np.array_equal(k1["U"][0][0], raw["U"][0][0]) and np.array_equal(k1["V"][1][1], raw["V"][1][1])
    assert np.array_equal(raw["U"][0][1], np.zeros((6, 6)))  # install copies
    mu = 0.1  # 2 + 0.1 is not a double: the block is the rounded sum, not the extended one
    X, env = fr.damped(*k1["V"], mu, fp, 2.0)
    assert np.array_equal(X[0], ar.LD(2.0 + 0.1) * np.eye(3)) and X[0, 0, 0] != ar.LD(2.0) + ar.LD(0.1)
    assert not np.any(env[0]) and np.all(np.diagonal(env[1]) > 0)
    assert X[1, 0, 0] == k1["V"][0][1, 0, 0] + ar.LD(0.1)
    U = np.stack([np.diag([5.0, 1, 1, 1, 1, 1]), 9.0 * np.eye(6)])
    V = np.stack([7.0 * np.eye(3), np.diag([1.0, 3.0, 2.0])])
    assert fr.free_max(U, V, fc, fp) == 5.0 and fr.all_max(U, V) == 9.0
    assert fr.free_max(U, V, [1, 0], [1, 0]) == 9.0 and fr.free_max(U, V, [1, 1], [0, 0]) == 7.0
    z = np.array([0.0, -0.0])
    assert np.array_equal(z, z[::-1]) and not fr.same_bits(z, z[::-1]) and fr.same_bits(z, z.copy())
    assert fr.plus_zero(z[:1]) and not fr.plus_zero(z)


def test_tiling_restated():
    """the greedy tiling on a hand-made point list: the observation limit, the point limit and a long point"""
    counts = [100, 100, 57, 300, 1] + [1] * 130 + [200, 56, 1]
    iidx = np.repeat(np.arange(len(counts)), counts)
    tl = fr.tiles(iidx, len(counts))
    assert tl == [(0, 2), (2, 3), (3, 4), (4, 132), (132, 136), (136, 138)]
    ptr = fr.point_ptr(iidx, len(counts))
    assert fr.crosses_wave(ptr, 0, 0) and fr.crosses_wave(ptr, 0, 1)  # 0..99 crosses 64, 100..199 crosses 128
    assert not fr.crosses_wave(ptr, 132, 134) and fr.crosses_wave(ptr, 132, 135)  # 2 alone, then 3..202
    assert not fr.crosses_wave(ptr, 136, 136) and not fr.crosses_wave(ptr, 136, 137)  # 0..55, then 56 alone


@pytest.mark.parametrize("name", ["7cams", "54cams"])
def test_masks_have_the_properties_they_claim(name, problems):
    prob = problems[name]
    nC, nP = int(prob["nC"]), int(prob["nP"])
    iidx, jidx = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    fc, fp, info = fr.mixed_mask(prob, cam_of_max(prob))
    print(f"\n{name} mixed: {info}")
    assert {0, 1, nC - 1, cam_of_max(prob)} == set(info["cams"]) and fp[0] and fp[nP - 1]
    assert info["wave_obs"][0] // 64 != info["wave_obs"][1] // 64 and fp[info["wave_point"]]
    assert 0 < fc.sum() < nC and 0.1 * nP <= fp.sum() < nP
    fc, fp, info = fr.island_mask(prob)
    print(f"{name} island: {info}")
    pt, cam = info["island_point"], info["island_cam"]
    assert not fp[pt] and np.all(fc[jidx[iidx == pt]]) and not fc[cam] and np.all(fp[iidx[jidx == cam]])
    assert 0 < fc.sum() < nC and 0 < fp.sum() < nP


# ---- calibration -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["7cams", "54cams"])
def test_oracle_on_masked_blocks_fits_every_envelope(name, problems):
    w = walk(name, problems)
    print(f"\n{name} mixed mask: {w.info}")
    r = w.ratios()
    for k, (x, b) in w.scal.items():
        got = {"dp_l2": w.dp @ w.dp, "gain_den": w.dp @ (w.mu * w.dp + w.lin["g"]), "newp_l2": w.newp @ w.newp,
               "new_cost": float(np.sum(w.o.exQT(w.newp[:w.nA], w.newp[w.nA:]) ** 2))}[k]
        r[k] = ratio(np.array([got]), np.array([x]), np.array([b]))
    for k, v in r.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{name}: the oracle's fp64 rounding on the masked blocks exceeds the envelope in {bad}"
    # the exact parts, as the oracle has them: zero blocks, mu I once damped, a zero step
    lin, sch = w.lin, w.sch
    fc, fp = fr.flags(w.fc, w.fp)
    assert fr.plus_zero(lin["U"].reshape(-1, 36)[fc]) and fr.plus_zero(lin["V"].reshape(-1, 9)[fp])
    assert not np.any(lin["W"].reshape(-1, 18)[fc[w.jidx] | fp[w.iidx]])  # (the oracle's 0 * x keeps x's sign)
    assert fr.plus_zero(lin["g"][w.fx]) and np.all(w.dp[w.fx] == 0.0)
    assert fr.same_bits(sch["Ustar"].reshape(-1, 6, 6)[fc], np.broadcast_to(w.mu * np.eye(6), (int(fc.sum()), 6, 6)))
    assert fr.free_max(lin["U"], lin["V"], fc, fp) == lin["maxdiag"]


# ---- power -------------------------------------------------------------------------------------------------------

def _unmasked(w):
    """A, B of the twin without the mask"""
    return RobustTwin.linearize(w.t)[1:]


def _fault_A_by_point_flag(w):
    """FIX_PT read where FIX_CAM is meant: A of an observation (free camera, fixed point) zeroed; the observation
    whose contribution to U_j is smallest"""
    fc, fp = fr.flags(w.fc, w.fp)
    cand = np.flatnonzero(fp[w.iidx] & ~fc[w.jidx])
    contrib = np.einsum("aki,akj->aij", w.A[cand], w.A[cand])
    a = cand[int(np.argmin(np.abs(contrib).max(axis=(1, 2))))]
    U = w.lin["U"].reshape(-1, 6, 6).copy()
    U[w.jidx[a]] -= w.A[a].T @ w.A[a]
    return dict(U=U), U, w.lin["U"].reshape(-1, 6, 6), 1e-11


def _fault_B_by_camera_flag(w):
    """the mirror image: B of an observation (fixed camera, free point) zeroed, the smallest contribution to V_i"""
    fc, fp = fr.flags(w.fc, w.fp)
    cand = np.flatnonzero(fc[w.jidx] & ~fp[w.iidx])
    contrib = np.einsum("aki,akj->aij", w.B[cand], w.B[cand])
    a = cand[int(np.argmin(np.abs(contrib).max(axis=(1, 2))))]
    V = w.lin["V"].reshape(-1, 3, 3).copy()
    V[w.iidx[a]] -= w.B[a].T @ w.B[a]
    return dict(V=V), V, w.lin["V"].reshape(-1, 3, 3), 1e-11


def _fault_W_of_fixed_point(w):
    """W of one observation of a fixed point (free camera) left at A^T B: it enters S_jj as -W W^T / (1 + mu), the
    library's placeholder 1 in V_i; the smallest such product"""
    fc, fp = fr.flags(w.fc, w.fp)
    _, B = _unmasked(w)
    cand = np.flatnonzero(fp[w.iidx] & ~fc[w.jidx])
    W = np.einsum("aki,akj->aij", w.A[cand], B[cand])
    prod = np.einsum("art,act->arc", W, W) / (1.0 + w.mu)
    q = int(np.argmin(np.abs(prod).max(axis=(1, 2))))
    j = w.jidx[cand[q]]
    S = w.sch["S"].copy()
    S[6 * j:6 * j + 6, 6 * j:6 * j + 6] -= prod[q]
    return dict(S=S), S, w.sch["S"], 1e-11


def _fault_gb_of_fixed_point(w):
    """g_b of one fixed point left at its sum (the sum of the unmasked B^T e)"""
    fp = np.flatnonzero(w.fp)
    _, B = _unmasked(w)
    i = int(fp[fp.size // 2])
    g = w.lin["g"].copy()
    sel = w.iidx == i
    g[w.nA + 3 * i:w.nA + 3 * i + 3] = np.einsum("aki,ak->i", B[sel], w.e.reshape(-1, 2)[sel])
    return dict(g=g), g, w.lin["g"], 1e-11


def _fault_dpb_one_ulp(w):
    """dp_b of a fixed point one ulp of its neighbour's instead of 0.0"""
    fp = np.flatnonzero(w.fp & np.r_[w.fp[1:] == 0, False])
    i = int(fp[fp.size // 2])
    dpb = w.dp[w.nA:].copy()
    dpb[3 * i:3 * i + 3] = np.spacing(np.abs(dpb[3 * i + 3:3 * i + 6]))
    assert np.all(dpb[3 * i:3 * i + 3] > 0)
    return dict(dpb=dpb), dpb, w.dp[w.nA:], 1e-9


# fault -> (the quantity whose check must fail, the injection)
FAULTS = {
    "A zeroed by the point's flag": ("U", _fault_A_by_point_flag),
    "B zeroed by the camera's flag": ("V", _fault_B_by_camera_flag),
    "W of a fixed point left non-zero": ("S", _fault_W_of_fixed_point),
    "g_b of a fixed point left at its sum": ("g", _fault_gb_of_fixed_point),
    "dp_b of a fixed point one ulp, not 0.0": ("dpb", _fault_dpb_one_ulp),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_fails_the_entrywise_check(fault, problems):
    w = walk("54cams", problems)
    what, inject = FAULTS[fault]
    kw, bad, good, tol = inject(w)
    r = w.ratios(**kw)[what]
    passes = close_passes(bad, good, tol)
    print(f"\n54cams '{fault}': entrywise ratio of {what} {r:.2e}; today's close(..., {tol:g}) "
          f"{'passes' if passes else 'fails'} it")
    assert r > 1.0, f"fault '{fault}' passes the entrywise check (ratio {r:.2e})"


def test_newp_l2_without_the_fixed_blocks_fails(problems):
    w = walk("54cams", problems)
    x, b = w.scal["newp_l2"]
    bad = float(w.newp[~w.fx] @ w.newp[~w.fx])
    r = ratio(np.array([bad]), np.array([x]), np.array([b]))
    good = float(w.newp @ w.newp)
    passes = abs(bad - good) <= 1e-8 * abs(good)
    print(f"\n54cams newp_l2 over the free blocks only: ratio {r:.2e}; today's relative 1e-8 "
          f"{'passes' if passes else 'fails'} it")
    assert r > 1.0


def test_signed_zero_of_a_fixed_block_is_seen_on_bit_patterns(problems):
    """camera 0's rotation set to -0.0 and a proposal that came back as cams + 0.0: array_equal passes it"""
    w = walk("54cams", problems)
    cur = np.r_[w.t.cams.reshape(-1), w.t.pts.reshape(-1)].copy()
    cur[:3] = -0.0
    bad = cur + np.where(w.fx, 0.0, w.dp)  # x + 0 instead of a select
    good = np.where(w.fx, cur, cur + w.dp)
    assert np.array_equal(bad[w.fx], cur[w.fx]), "today's check sees nothing"
    assert fr.same_bits(good[w.fx], cur[w.fx])
    assert not fr.same_bits(bad[w.fx], cur[w.fx])
    print("\n54cams proposal with -0.0 turned into +0.0: bit patterns differ; today's array_equal passes it")


@functools.lru_cache(maxsize=None)
def _scaled(loader):
    """54cams scaled by 2^-22 under the mixed mask of the unscaled problem: (problem, fc, fp, twin's U, V, e, A, B)"""
    base = loader("54cams")
    prob = fr.scaled_problem(base)
    fc, fp, _ = fr.mixed_mask(base, cam_of_max(base))
    _, (e, A, B), lin = fixed_pieces(prob, fc, fp)
    return base, prob, fc, fp, (e, A, B), lin


def test_scaled_problem_is_an_exact_scaling_below_the_placeholder(problems):
    base, prob, fc, fp, (e, A, B), lin = _scaled(problems.__getitem__)
    _, (e0, A0, B0), lin0 = fixed_pieces(base, fc, fp)
    s = 2.0 ** -22
    assert fr.same_bits(e, e0 * s) and fr.same_bits(A, A0 * s) and fr.same_bits(B, B0 * s)
    U, V = lin["U"].reshape(-1, 6, 6), lin["V"].reshape(-1, 3, 3)
    m = fr.free_max(U, V, fc, fp)
    assert m == lin["maxdiag"] and 0.5 < m < 0.75, m  # 0.570: below the placeholder 1 (and 1.140 below 2)
    mu = 1e-3 * m
    f = fp != 0
    det = np.linalg.det(V[~f] + mu * np.eye(3))
    print(f"\nscaled 54cams: largest free diagonal entry {m:.3f}, smallest det(V + mu I) {det.min():.2e}")
    assert det.min() > 1e-10  # 1.02e-9: far above sym3_inverse's absolute 1e-16 singular flag


def test_placeholder_in_the_maximum_shows_only_on_the_scaled_problem(problems):
    base, prob, fc, fp, _, lin = _scaled(problems.__getitem__)
    _, _, lin0 = fixed_pieces(base, fc, fp)
    for place in (1.0, 2.0):  # psba_linearize(1, 1) and (2, -2)
        out = {}
        for name, l in (("54cams", lin0), ("scaled", lin)):
            k1 = fr.install({"U": (place * ar.ld(l["U"]).reshape(-1, 6, 6), np.zeros((fc.size, 6, 6))),
                             "V": (place * ar.ld(l["V"]).reshape(-1, 3, 3), np.zeros((fp.size, 3, 3))),
                             "g": (ar.ld(l["g"]), np.zeros(l["g"].size))}, fc, fp, place)
            U, V = k1["U"][0].astype(np.float64), k1["V"][0].astype(np.float64)
            want, bad = fr.free_max(U, V, fc, fp), fr.all_max(U, V)
            out[name] = abs(bad - want) <= 1e-12 * want
            print(f"\n{name}, placeholder {place}: maximum over the free blocks {want:.6g}, with the placeholder "
                  f"{bad:.6g}: the relative 1e-12 {'passes' if out[name] else 'fails'} the fault")
        assert out["54cams"] and not out["scaled"]
