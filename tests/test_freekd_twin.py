"""The numpy twin of PSBA_CAMERA_FREE_KD (tests/freekd_twin.py) against central differences, the oracle's 11-column
twin, lens_twin.Twin, its own sums in extended precision, and a synthetic scene it must recover (CPU only)."""
import os

import numpy as np
import pytest

from conftest import DATA
from freekd_twin import BAL, CNP, TwinKD, ring_problem, start_kc, tiny_problem
from sba_text import read_problem


def problem(cams, pts, max_pts=None):
    p = read_problem(os.path.join(DATA, cams), os.path.join(DATA, pts))
    if max_pts is not None and p["nP"] > max_pts:
        keep = np.asarray(p["iidx"]) < max_pts
        p = dict(p, pts=np.asarray(p["pts"])[:max_pts], impts=np.asarray(p["impts"])[keep],
                 iidx=np.asarray(p["iidx"])[keep], jidx=np.asarray(p["jidx"])[keep], nP=max_pts, nO=int(keep.sum()))
    return p


def P7():
    return problem("7camsvarK.txt", "7pts.txt")


def P54():
    return problem("54camsvarK.txt", "54pts.txt", 450)


def scaled_tol(p):
    """64 eps (largest observation count of one camera + 16): the bound of a sum of that length, safety 64"""
    return 64 * np.finfo(np.float64).eps * (np.bincount(np.asarray(p["jidx"])).max() + 16)


@pytest.mark.parametrize("make", [P7, P54])
def test_twin_jacobian_against_central_differences(make):
    p = make()
    t = TwinKD(p, start_kc(p["nC"]))
    _, A, B = t.linearize()
    for k in range(CNP):
        h = 1e-6 * max(1.0, np.abs(t.cams[:, k]).max())
        cp, cm = t.cams.copy(), t.cams.copy()
        cp[:, k] += h
        cm[:, k] -= h
        num = -(t.residual(cams=cp) - t.residual(cams=cm)) / (2 * h)
        err = np.abs(A[:, :, k] - num).max() / np.abs(num).max()
        print(f"column {k}: relative error {err:.2e}")
        assert err <= 1e-6
    for k in range(3):
        pp, pm = t.pts.copy(), t.pts.copy()
        pp[:, k] += 1e-6
        pm[:, k] -= 1e-6
        num = -(t.residual(pts=pp) - t.residual(pts=pm)) / 2e-6
        assert np.abs(B[:, :, k] - num).max() <= 1e-6 * np.abs(num).max()


def test_twin_reduces_to_the_eleven_column_oracle_at_zero_distortion():
    from oracle_lib import OracleFreeK
    p = P7()
    _, A, B = TwinKD(p).linearize()
    JA, JB = OracleFreeK(p).jacobi()
    cols = list(range(5)) + list(range(10, 16))
    np.testing.assert_allclose(A[:, :, cols], JA, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(B, JB, rtol=1e-12, atol=1e-12)
    assert np.all(A[:, 0, 1] == 1.0) and np.all(A[:, 1, 2] == 1.0)


def test_twin_extrinsic_columns_are_the_lens_twins():
    import lens_twin
    p = P7()
    kc = start_kc(p["nC"])
    e, A, B = TwinKD(p, kc).linearize()
    e6, A6, B6 = lens_twin.Twin(p, kc).linearize()
    assert np.array_equal(e, e6) and np.array_equal(A[:, :, 10:], A6) and np.array_equal(B, B6)


def test_twin_mask_zeroes_columns_and_keeps_the_rest():
    p = P7()
    kc = start_kc(p["nC"])
    _, Af, _ = TwinKD(p, kc).linearize()
    _, Am, _ = TwinKD(p, kc, BAL).linearize()
    held = [k for k in range(10) if not BAL[k]]
    kept = [k for k in range(16) if k not in held]
    assert np.all(Am[:, :, held] == 0.0) and np.array_equal(Am[:, :, kept], Af[:, :, kept])


@pytest.mark.parametrize("make", [tiny_problem, P7, P54])
def test_twin_sums_against_extended_precision(make):
    """The fp64 twin's own S and e_a against the same Jacobian blocks summed in 80-bit block by block, in the scaled
    measure the GPU tests use: it must sit well inside the tolerance it judges with (DESIGN 7d records the figures)."""
    p = make()
    t = TwinKD(p, start_kc(p["nC"]), BAL)
    cost, N, g = t.normal()
    worst = 0.0
    for mu in (1e-3 * t.max_diag(N), 1e-6 * np.median(np.diag(N))):
        S, ea = t.schur(N, g, mu)
        Sx, eax = t.schur_blocks(mu)
        d = np.sqrt(np.diag(N)[:t.nA] + mu)
        eS = (np.abs(S - Sx.astype(np.float64)) / np.outer(d, d)).max()
        ee = (np.abs(ea - eax.astype(np.float64)) / (d * np.sqrt(cost))).max()
        print(f"mu {mu:.3e}: twin S {eS:.2e}, e_a {ee:.2e} (tol {scaled_tol(p):.2e})")
        worst = max(worst, eS, ee)
    assert worst <= 0.25 * scaled_tol(p)


def test_twin_recovers_the_ring_scene():
    """Exact projections, the mask of Bundle Adjustment in the Large: the model and its Jacobian recover f, k1, k2 to
    fp64.  Without the loop's absolute stop (cost <= 1e-12 ends psba_levmar near 1e-17 of the initial cost here, with
    f at a few 1e-9: see test_gpu_freekd.py) so that the damping rules are followed to the end."""
    start, kc0, K_true, kc_true = ring_problem()
    t = TwinKD(start, kc0, BAL)
    res, log = t.levmar(max_iter=30, stop_small=False)
    f = np.abs(t.cams[:, 0] / K_true[:, 0] - 1).max()
    k1 = np.abs(t.cams[:, 5] - kc_true[:, 0]).max()
    k2 = np.abs(t.cams[:, 6] - kc_true[:, 1]).max()
    print(f"iterations {res.iters}, cost {res.final_err:.2e} of {res.init_err:.2e}, f {f:.1e}, k1 {k1:.1e}, k2 {k2:.1e}")
    assert res.final_err <= 1e-20 * res.init_err
    assert f <= 1e-12
