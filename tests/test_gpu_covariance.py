"""Covariance of the refined cameras and points on the GPU (psba_covariance_compute): the state and error
rules, the inverse judged entry by entry against an extended-precision inverse of the device's own S, chosen matrices
through reassemble = 0, the point formula per entry on the device's own V*^-1, Y and C_aa, the whole against the numpy
twin's reduced dense inverse, and structure-only / scale / determinism.  Needs an MI355X.

What judges the inverse (tests 2 and 3): LAPACK's fp64 inverse of the same matrix against the same reference is the
yardstick, and the device's normwise error may be at most MARGIN = 16 times max(that, n eps) -- the margin for another
block size and MFMA summation order in the same algorithm class, not a figure measured on the code under test."""
import functools
import os

import numpy as np
import pytest

import psba_amd
from psba_amd import capi, synth
import cov_ref as cr
import dense_ref as dr
from fixed_twin import random_kc, random_spd
from robust_twin import KINDS
from sba_text import KK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
EPS = cr.EPS
MARGIN = 16.0
LD = cr.LD


@functools.lru_cache(maxsize=None)
def _golden(n):
    return psba_amd.read_problem(os.path.join(DATA, f"{n}cams.txt"), os.path.join(DATA, f"{n}pts.txt"), KK)


def _mask(prob, frac=0.1, seed=17):
    """cameras 0 and 1 and a seeded fraction of the points"""
    fc = np.zeros(prob["nC"], dtype=np.uint8)
    fc[[0, 1]] = 1
    fp = np.zeros(prob["nP"], dtype=np.uint8)
    if frac > 0:
        fp[np.random.default_rng(seed).choice(prob["nP"], max(1, round(frac * prob["nP"])), replace=False)] = 1
    return fc, fp


def _handle(prob, fc=None, fp=None, kind=None, c=2.0, kc=None, cov=None):
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    if kc is not None:
        h.set_distortion(kc)
    if cov is not None:
        h.set_obs_covariance(cov)
    if kind is not None:
        h.set_robust_loss(kind, c)
    if fc is not None or fp is not None:
        h.set_fixed(fc, fp)
    return h


def _S(h):
    n32 = dr.n32_of(h.nA)
    return h.get_reduce_buffer().reshape(n32 + 1, n32)[:h.nA, :h.nA].copy()


def _refused(fn, code, *words):
    with pytest.raises(capi.PsbaError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def _getters_refuse(h):
    for fn in (h.camera_covariance, h.covariance_matrix, h.point_covariance):
        _refused(fn, -6)


def _judge_inverse(C, S, free, what):
    """C (device) against the extended-precision inverse of S[free, free] embedded with zeros; returns the ratio of the
    device's normwise error to the yardstick max(LAPACK's error, n eps).  (The reduce buffer is bit-symmetric, so the
    lower triangle the factorization reads and the matrix LAPACK takes are the same S.)"""
    assert np.array_equal(S, S.T), what
    ref, it = cr.embedded_inverse(S, free)
    idx = np.flatnonzero(free)
    lap = np.zeros(S.shape)
    lap[np.ix_(idx, idx)] = np.linalg.inv(S[np.ix_(idx, idx)])
    scale = float(np.abs(ref).max())
    yard = max(float(np.abs(lap.astype(LD) - ref).max()) / scale, S.shape[0] * EPS)
    dev = float(np.abs(C.astype(LD) - ref).max()) / scale
    print(f"{what}: refined in {it} iterations; LAPACK / n eps yardstick {yard:.2e}, device {dev:.2e}, ratio {dev / yard:.2f}")
    assert dev <= MARGIN * yard, (what, dev, yard)
    assert np.array_equal(C, C.T), what  # bit-symmetric
    assert np.all(C[~free] == 0.0) and np.all(C[:, ~free] == 0.0), what
    return dev / yard


# ---- 1. state and error rules ------------------------------------------------------------------------------------
def test_state_and_error_rules():
    prob = _golden(7)
    fc, fp = _mask(prob)
    h = psba_amd.Psba(0)
    _refused(lambda: h.covariance(), -6, "no problem uploaded")  # before an upload
    for name in ("psba_get_covariance_matrix", "psba_get_point_covariance"):
        assert getattr(capi.lib, name)(h._h, None) == -6
    h.upload_problem(prob)
    h.set_fixed(fc, fp)
    _getters_refuse(h)  # nothing computed yet
    for mu, scale in ((-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.0, 0.0), (0.0, -2.0),
                      (0.0, float("nan")), (0.0, float("inf"))):
        _refused(lambda: h.covariance(mu, scale), -1)
    _refused(lambda: h.covariance(scale="chi"), -1)
    _getters_refuse(h)
    _refused(lambda: h.covariance(reassemble=False), -6, "psba_schur_assemble")  # nothing in the reduce buffer
    assert h.covariance() == capi.PSBA_OK
    C, D, P = h.covariance_matrix(), h.camera_covariance(), h.point_covariance()
    assert D.shape == (7, 6, 6) and P.shape == (prob["nP"], 3, 3)
    # a refused call changes nothing
    _refused(lambda: h.covariance(-1.0), -1)
    _refused(lambda: h.camera_covariance([(0, 7)]), -1, "out of range")
    _refused(lambda: h.camera_covariance([(-1, 2)]), -1, "out of range")
    out = np.empty(36 * 3)
    assert capi.lib.psba_get_camera_covariance(h._h, 3, None, capi._d(out)) == -1  # no list: n_pairs must be nCams
    assert capi.lib.psba_get_camera_covariance(h._h, 7, None, None) == -1
    assert capi.lib.psba_covariance_times(h._h, None) == -1 and h.covariance_times().shape == (3,)
    assert np.array_equal(h.covariance_matrix(), C) and np.array_equal(h.point_covariance(), P)
    assert np.array_equal(h.camera_covariance(), D)
    # the handle is as after psba_schur_reduce: the buffer holds the S that was inverted, and a solve may follow
    S = _S(h)
    assert np.array_equal(S[:12, :12], np.eye(12)) and np.all(S[:12, 12:] == 0.0)
    h.schur_solve()
    sc = h.backsub(0.0)
    assert sc.status == 0
    assert np.array_equal(h.covariance_matrix(), C)  # a try does not touch the covariance's workspace ...
    h.accept()  # ... but accepting its step moves the parameters
    _getters_refuse(h)
    # everything that moves the parameters or the model invalidates the result
    cams, pts = h.get_params()
    rng = np.random.default_rng(1)
    movers = [lambda: h.set_params(cams, pts), h.reset_params, lambda: h.set_distortion(random_kc(rng, 7)),
              lambda: h.set_distortion(None), lambda: h.set_obs_covariance(random_spd(rng, prob["nO"])),
              lambda: h.set_obs_covariance(None), lambda: h.set_robust_loss(KINDS["huber"], 2.0),
              lambda: h.set_robust_loss(capi.LOSS_NONE, 1.0), lambda: h.set_fixed(fc, None), lambda: h.set_fixed(fc, fp),
              lambda: (h.upload_problem(prob), h.set_fixed(fc, fp))]
    for move in movers:
        assert h.covariance() == capi.PSBA_OK
        h.covariance_matrix()
        move()
        _getters_refuse(h)
    # a try in flight
    h.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h.schur_reduce()
    h.schur_solve()
    h.backsub_async(mu)
    _refused(lambda: h.covariance(), -6, "in flight")
    h.backsub_wait()
    assert h.covariance() == capi.PSBA_OK
    h.close()
    # the routes that are out of scope refuse with a text that names the reason
    for model, word in ((psba_amd.CAMERA_FREE_K, "PSBA_CAMERA_FREE_K"), (psba_amd.CAMERA_FREE_KD, "PSBA_CAMERA_FREE_KD")):
        fk = psba_amd.Psba(0)
        fk.set_camera_model(model)
        fk.upload_problem(psba_amd.read_problem(os.path.join(DATA, "7camsvarK.txt"), os.path.join(DATA, "7pts.txt")))
        _refused(lambda: fk.covariance(1.0), -6, word)
        if model == psba_amd.CAMERA_FREE_K:
            assert "PSBA_CAMERA_FREE_KD" not in str(capi.lib.psba_last_error(fk._h).decode())
        fk.close()
    pcg = psba_amd.Psba(0)
    pcg.set_solver(1, tol=1e-12, max_iter=100)
    pcg.upload_problem(prob)
    pcg.set_fixed(fc, fp)
    _refused(lambda: pcg.covariance(), -6, "PSBA_SOLVER_PCG")
    pcg.close()
    rk = psba_amd.Psba(0)
    rk.set_rank_layout(2, 0)
    rk.upload_problem(capi.shard_problem(prob, 2, 0))
    _refused(lambda: rk.covariance(1.0), -6, "rank layout")
    rk.close()


# ---- 2. the inverse, on its own input ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 7, 9, 54])
def test_inverse_against_extended_precision_inverse_of_the_devices_own_S(n):
    prob = _golden(n)
    fc, _ = _mask(prob, frac=0)
    h = _handle(prob, fc, None)
    free = np.repeat(fc == 0, 6)
    h.linearize(1.0, 1.0)
    for mu in (0.0, 1e-6 * h.max_diag()):
        st = h.covariance(mu)
        if n == 3 and mu == 0.0:
            # the free camera of this problem sees one point: S has rank 2 of 6 and no covariance exists.  Whether the
            # rounding leaves a pivot that is not positive decides the status; a judgement of accuracy has no meaning
            assert st in (capi.PSBA_OK, capi.PSBA_NOT_SPD)
            if st == capi.PSBA_NOT_SPD:
                _getters_refuse(h)
            else:
                C = h.covariance_matrix()
                assert np.array_equal(C, C.T) and np.all(C[:12] == 0.0)
            continue
        assert st == capi.PSBA_OK
        S = _S(h)  # the S that was inverted
        C = h.covariance_matrix()
        _judge_inverse(C, S, free, f"{n} cameras, mu = {mu:.3g}")
        # pairs in both orders are the blocks of the matrix and their transposes, bit for bit
        rng = np.random.default_rng(n)
        pairs = rng.integers(0, n, size=(40, 2))
        pairs[0] = (n - 1, 0)
        B = h.camera_covariance(pairs)
        Bt = h.camera_covariance(pairs[:, ::-1])
        for (j, k), b, bt in zip(pairs, B, Bt):
            assert np.array_equal(b, C[6 * j:6 * j + 6, 6 * k:6 * k + 6])
            assert np.array_equal(bt, b.T)
        D = h.camera_covariance()
        assert all(np.array_equal(D[j], C[6 * j:6 * j + 6, 6 * j:6 * j + 6]) for j in range(n))
        assert np.all(D[:2] == 0.0) and np.all(np.einsum("jkk->jk", D[2:]) > 0.0)
    h.close()


def test_fixed_cameras_away_from_the_leading_tile():
    """Every other test here fixes cameras 0 and 1, whose coordinates 0 .. 11 lie inside the first 16 x 16 tile.  With
    cameras 2 and 5 fixed the dead coordinates 12 .. 17 straddle the tile edge at 16 and 30 .. 35 the edge at 32, so a
    wrong index on a fixed camera in the compaction or the finish shows."""
    prob = _golden(7)
    fc = np.zeros(7, dtype=np.uint8)
    fc[[2, 5]] = 1
    h = _handle(prob, fc, None)
    free = np.repeat(fc == 0, 6)
    h.linearize(1.0, 1.0)
    for mu in (0.0, 1e-6 * h.max_diag()):
        assert h.covariance(mu) == capi.PSBA_OK
        _judge_inverse(h.covariance_matrix(), _S(h), free, f"cameras 2 and 5 fixed, mu = {mu:.3g}")
        D = h.camera_covariance()
        assert np.all(D[fc != 0] == 0.0) and np.all(np.einsum("jkk->jk", D[fc == 0]) > 0.0)
        P = h.point_covariance()
        assert np.array_equal(P, np.transpose(P, (0, 2, 1)))
    h.close()


# ---- 3. chosen matrices through reassemble = 0 -----------------------------------------------------------------------
def test_chosen_matrices_through_reassemble_0():
    prob = _golden(54)
    fc, _ = _mask(prob, frac=0)
    h = _handle(prob, fc, None)
    free = np.repeat(fc == 0, 6)
    nA = h.nA
    h.linearize(1.0, 1.0)
    h.schur_assemble(1e-3 * h.max_diag())
    for what, buf in (("well conditioned", dr.lowrank_shift(nA, 100.0, 11)), ("kappa 1e10", dr.spectrum(nA, 1e10, 12))):
        h.set_reduce_buffer(buf)
        assert h.covariance(reassemble=False) == capi.PSBA_OK
        A = dr.matrix(buf, nA)
        assert np.array_equal(_S(h), A)  # the buffer is untouched
        _judge_inverse(h.covariance_matrix(), A.copy(), free, what)
        _refused(h.point_covariance, -6, "reassemble = 0")  # only the camera part exists
    h.set_reduce_buffer(dr.indefinite(nA, 100, 13))
    assert h.covariance(reassemble=False) == capi.PSBA_NOT_SPD
    _getters_refuse(h)
    h.set_reduce_buffer(dr.lowrank_shift(nA, 100.0, 11))
    assert h.covariance(reassemble=False) == capi.PSBA_OK  # ... and the next one is good again
    h.close()


# ---- 4. points, on their own inputs ------------------------------------------------------------------------------------
def _edited(prob, fc):
    """the problem with one track cut to length 1 (its first free camera) and one cut to the fixed cameras alone;
    returns (problem, the two points)"""
    i, j = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    fixed = np.flatnonzero(fc)
    both = [q for q in range(prob["nP"]) if set(fixed) <= set(j[i == q])]
    p_fix = both[0]
    p_one = next(q for q in range(prob["nP"]) if q != p_fix and not set(j[i == q]) <= set(fixed))
    keep = np.ones(i.size, dtype=bool)
    keep[(i == p_fix) & ~np.isin(j, fixed)] = False
    first_free = np.flatnonzero((i == p_one) & ~np.isin(j, fixed))[0]
    keep[i == p_one] = False
    keep[first_free] = True
    out = psba_amd.Problem(prob)
    out["iidx"], out["jidx"] = i[keep].copy(), j[keep].copy()
    out["impts"] = np.asarray(prob["impts"]).reshape(-1, 2)[keep].copy()
    out["nO"] = int(keep.sum())
    return out, p_fix, p_one


def _judge_points(prob, fc, fp, kw, what):
    """every entry of every free point of a compute at mu = 1e-6 max diag, scale = 2.5 against the long-double sum of
    its terms on the device's own V*^-1, Y (mirror verbs of a second handle) and C_aa; returns (P, Vinv, bounds)"""
    h, m = _handle(prob, fc, fp, **kw), _handle(prob, fc, fp, **kw)
    h.linearize(1.0, 1.0)
    mu, scale = 1e-6 * h.max_diag(), 2.5
    assert h.covariance(mu, scale) == capi.PSBA_OK
    Caa, P = h.covariance_matrix(), h.point_covariance()
    m.linearize(1.0, 1.0)
    m.update_UV(mu)
    Vinv = m.compute_Vinv()[1].reshape(-1, 3, 3)
    Y = m.compute_Yblks().reshape(-1, 6, 3)
    m.restore_UVdiag()
    h.close()
    m.close()
    i, j = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    assert np.all(P[fp != 0] == 0.0)  # fixed points are exactly 0
    assert np.array_equal(P, np.transpose(P, (0, 2, 1)))  # symmetry is bit-exact
    cnt = np.bincount(i, minlength=prob["nP"])
    free_pts = np.flatnonzero(fp == 0)
    J = cr.point_judges(i, j, Vinv, Y, Caa, scale, free_pts)
    worst = 0.0
    for q, (want, bound, want_ld) in J.items():
        err = np.abs(P[q].astype(LD) - want_ld).astype(np.float64)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (q, int(cnt[q]), err, bound)
    print(f"{what}: {len(J)} points (tracks {cnt[free_pts].min()} .. {cnt[free_pts].max()}), worst error / bound {worst:.3f}")
    return P, scale * Vinv, J


@pytest.mark.parametrize("model", ["plain", "lens_cov_huber"])
@pytest.mark.parametrize("n", [9, 54])
def test_points_per_entry_on_the_devices_own_inputs(n, model):
    base = _golden(n)
    fc, fp = _mask(base)
    prob, p_fix, p_one = _edited(base, fc)
    fp[[p_fix, p_one]] = 0
    rng = np.random.default_rng(n)
    kw = {}
    if model != "plain":
        kw = dict(kind=KINDS["huber"], c=2.0, kc=random_kc(rng, n, k1=0.05), cov=random_spd(rng, prob["nO"]))
    i, j = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    assert np.count_nonzero(i == p_one) == 1 and set(j[i == p_fix]) == {0, 1}
    P, sVinv, J = _judge_points(prob, fc, fp, kw, f"{n} cameras, {model}")
    assert int(p_fix) in J and int(p_one) in J
    # the point of the fixed cameras alone is scale V*^-1 (its C_jk are zero), to the same bound
    assert np.all(np.abs(P[p_fix] - sVinv[p_fix]) <= J[int(p_fix)][1])


def test_points_with_tracks_longer_than_a_staging_chunk():
    """k_cov_points stages the rows Z_j of 32 cameras at a time: tracks of 33 .. 55 cameras take two chunks (the second
    one partial), 64 exactly two, 70 three, with the sum carried from chunk to chunk."""
    prob = synth.make_problem(70, 40, 48.0, 41, min_track=33, max_track=70)
    cnt = np.bincount(np.asarray(prob["iidx"]), minlength=prob["nP"])
    assert cnt.min() == 33 and cnt.max() == 70 and np.any(cnt == 64) and np.any((cnt > 32) & (cnt < 64) & (cnt % 32 != 0))
    fc = np.zeros(70, dtype=np.uint8)
    fc[[0, 1]] = 1
    fp = np.zeros(40, dtype=np.uint8)
    fp[[5, 17]] = 1
    _judge_points(prob, fc, fp, {}, "70 cameras, long tracks")


# ---- 5. end to end against the twin ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 9])
def test_end_to_end_against_the_twins_reduced_dense_inverse(n):
    prob = _golden(n)
    fc, fp = _mask(prob)
    h = _handle(prob, fc, fp)
    h.linearize(1.0, 1.0)
    mu = 1e-6 * h.max_diag()
    assert h.covariance(mu) == capi.PSBA_OK
    Caa, P = h.covariance_matrix(), h.point_covariance()
    h.close()
    C, kappa = cr.dense_covariance(cr.twin(prob, fc != 0, fp != 0), mu)
    assert kappa <= 1e7, kappa  # so that the bound means something
    tol = kappa * 1e-11  # 1e-11: the project's S parity tolerance
    nA = 6 * n
    want_a = C[:nA, :nA]
    want_b = np.stack([C[nA + 3 * q:nA + 3 * q + 3, nA + 3 * q:nA + 3 * q + 3] for q in range(prob["nP"])])
    ea = np.abs(Caa - want_a).max() / np.abs(want_a).max()
    eb = np.abs(P - want_b).max() / np.abs(want_b).max()
    print(f"{n} cameras: kappa {kappa:.2e}, cameras {ea:.2e}, points {eb:.2e} (bound {tol:.2e})")
    assert ea <= tol and eb <= tol


# ---- 6. structure-only, scale and determinism ------------------------------------------------------------------------
def test_structure_only_scale_and_determinism():
    prob = _golden(9)
    fc, fp = _mask(prob)
    # every camera fixed: no S, C_aa = 0, the points are V*^-1
    so = _handle(prob, np.ones(9, dtype=np.uint8), fp)
    so.linearize(1.0, 1.0)
    mu = 1e-6 * so.max_diag()
    assert so.covariance(mu) == capi.PSBA_OK
    assert np.all(so.covariance_matrix() == 0.0)
    P = so.point_covariance()
    so.update_UV(mu)
    Vinv = so.compute_Vinv()[1].reshape(-1, 3, 3)
    so.restore_UVdiag()
    assert np.array_equal(P[fp == 0], Vinv[fp == 0]) and np.all(P[fp != 0] == 0.0)
    so.close()

    h = _handle(prob, fc, fp)
    assert h.covariance(0.0, 1.0) == capi.PSBA_OK
    C1, P1, S1 = h.covariance_matrix(), h.point_covariance(), _S(h)
    # the same buffer inverted again: bit-identical
    assert h.covariance(0.0, 1.0, reassemble=False) == capi.PSBA_OK
    assert np.array_equal(h.covariance_matrix(), C1)
    # the whole again.  The new kernels have no atomics; the assembly in front of them sums with LDS atomics in an
    # order that may differ between launches, so bit-identity is asserted whenever S came out the same
    assert h.covariance(0.0, 1.0) == capi.PSBA_OK
    C2, P2, S2 = h.covariance_matrix(), h.point_covariance(), _S(h)
    same = np.array_equal(S1, S2)
    print(f"S of the two assemblies bit-identical: {same}")
    if same:
        assert np.array_equal(C2, C1) and np.array_equal(P2, P1)
    else:
        assert np.abs(C2 - C1).max() <= 1e-7 * np.abs(C1).max() and np.abs(P2 - P1).max() <= 1e-7 * np.abs(P1).max()
    # scale = 4 on the buffer as it stands (reassemble = 0: the same S): a power of two commutes with every rounding
    assert h.covariance(0.0, 4.0, reassemble=False) == capi.PSBA_OK
    C4 = h.covariance_matrix()
    assert np.all(np.abs(C4 - 4.0 * C2) <= EPS * np.abs(4.0 * C2))
    # ... and with the points, whenever the assembly gave the same S again
    assert h.covariance(0.0, 4.0) == capi.PSBA_OK
    C4, P4, S4 = h.covariance_matrix(), h.point_covariance(), _S(h)
    if np.array_equal(S4, S2):
        assert np.all(np.abs(C4 - 4.0 * C2) <= EPS * np.abs(4.0 * C2))
        assert np.all(np.abs(P4 - 4.0 * P2) <= EPS * np.abs(4.0 * P2))
    else:
        assert np.abs(P4 - 4.0 * P2).max() <= 1e-7 * np.abs(P4).max()
    # reduced chi-square: the scale is the cost over the degrees of freedom
    dof = 2 * prob["nO"] - (6 * 7 + 3 * int((fp == 0).sum()))
    s2 = h.residual() / dof
    assert h.covariance(0.0, "reduced_chi2") == capi.PSBA_OK
    Cr = h.covariance_matrix()
    assert np.abs(Cr - s2 * C2).max() <= 1e-7 * np.abs(Cr).max()
    # an LM run after a compute is the run of a fresh handle (two handles agree to rounding, not bit for bit: the
    # loop's sums depend on the order of its atomics, tests/test_gpu_robust.py)
    def same_log(a, b):
        return (a.shape == b.shape and np.array_equal(a[:, [0, 4]], b[:, [0, 4]])
                and np.abs(a[:, 1] - b[:, 1]).max() <= 1e-12 * np.abs(b[:, 1]).max())

    _, log = h.levmar(max_iter=5, log_cap=64)
    fresh = _handle(prob, fc, fp)
    _, log0 = fresh.levmar(max_iter=5, log_cap=64)
    _getters_refuse(h)  # the loop accepted steps
    h.close()
    fresh.close()
    if not same_log(log, log0):
        # DESIGN 5d, "LM runs that ended on another cost" (open): now and then one LM run of a handle takes another path
        # than every other run of the same problem, with or without a covariance before it.  Seen here once (the fourth
        # row of the run after the computes at 3235.71 where the fresh handle and sixteen replays of both sequences in
        # a process of their own have 3210.92).  As tests/test_gpu_parity.py does: the reference may be the odd one, so a
        # second fresh handle is asked; the log of the run after the computes is kept
        import warnings
        warnings.warn(f"an LM run after a compute and a fresh handle's disagree:\n{log}\n{log0}")
        fresh = _handle(prob, fc, fp)
        _, log0 = fresh.levmar(max_iter=5, log_cap=64)
        fresh.close()
        assert same_log(log, log0), (log, log0)


def test_two_computes_are_bit_identical_on_a_reproducible_S():
    """The unconditional form of the bit-identity above.  With two points every sum of the existing assembly has at
    most two addends besides zero, and a + b is b + a: S is the same bits whatever order its atomics take, so the whole
    of two computes -- linearization, assembly, factor, inverse and the point kernel on tracks of 70 cameras (three
    staging chunks) -- has to repeat bit for bit."""
    prob = synth.make_problem(70, 2, 70.0, 7, min_track=70, max_track=70)
    fc = np.zeros(70, dtype=np.uint8)
    fc[[0, 1]] = 1
    h = _handle(prob, fc, None)
    h.linearize(1.0, 1.0)
    mu = 1e-6 * h.max_diag()
    got = []
    for rep in range(3):
        if rep == 2:
            h.reset_params()  # the third compute linearizes again as well
        assert h.covariance(mu, 1.0) == capi.PSBA_OK
        got.append((_S(h), h.covariance_matrix(), h.point_covariance()))
    h.close()
    for S, C, P in got[1:]:
        assert np.array_equal(S, got[0][0])  # the premise
        assert np.array_equal(C, got[0][1]) and np.array_equal(P, got[0][2])
    assert np.all(np.einsum("ikk->ik", got[0][2]) > 0.0)
