"""A second psba_upload_problem on a used handle: include/psba_hip.h promises that a new upload resets the lens model,
the loss and the fixed-block mask, and everything else an upload creates (buffers, K2's schedule, the state of the try
in flight) has to be that of the new problem alone.  One handle is driven through a sequence of uploads -- smaller
problem, forced owner route, back to the LDS route, a rejected upload -- and after each one compared with a fresh
handle given the same calls under the same environment.  Needs an MI355X.

psba_set_solver refuses to change the solver while a problem is uploaded (PSBA_E_STATE: the buffers depend on it) and
there is no verb that drops a problem, so a handle cannot go from the dense solver to PSBA_SOLVER_PCG and back: the
sequence has no such leg."""
import os

import numpy as np
import pytest

import psba_amd
from psba_amd import capi
from fixed_twin import close, random_kc, random_spd
from sba_text import KK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
E_INVALID, E_STATE, SOLVER_PCG = -1, -6, 1  # include/psba_hip.h


def _prob(name):
    return psba_amd.read_problem(os.path.join(DATA, f"{name}cams.txt"), os.path.join(DATA, f"{name}pts.txt"), KK)


def _same_as_fresh(H, prob, path, what):
    """H, which has just uploaded prob, against a handle that never held anything else: the tolerances of two handles
    on one problem (test_gpu_lens.py::test_neutral_settings_equal_plain; the LDS atomics rule out bit equality)"""
    F = psba_amd.Psba(0)
    F.upload_problem(prob)
    assert H.schur_path() == F.schur_path() == path, what
    for h in (H, F):
        assert h.lens_model() == (False, False), what
        assert h.robust_loss() == (capi.LOSS_NONE, 1.0), what
        assert h.fixed_counts() == (0, 0), what
    for verb in ("compute_exQT", "compute_jacobiQT"):
        a, b = getattr(F, verb)(), getattr(H, verb)()
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            close(y, x, 1e-13, f"{what}: {verb}")
    for verb in ("compute_U", "compute_V", "compute_Wblks", "compute_g"):
        close(getattr(H, verb)(1.0), getattr(F, verb)(1.0), 1e-13, f"{what}: {verb}")
    mu = 1e-3 * F.maxElmOfUV()
    assert abs(H.maxElmOfUV() - F.maxElmOfUV()) <= 1e-13 * F.maxElmOfUV(), what
    H.update_UV(mu)
    F.update_UV(mu)
    close(H.compute_S(), F.compute_S(), 1e-13, f"{what}: S")
    close(H.compute_ea(), F.compute_ea(), 1e-13, f"{what}: ea")
    for h in (H, F):
        h.restore_UVdiag()
        h.reset_params()
    rf, _ = F.levmar(max_iter=10)
    rh, _ = H.levmar(max_iter=10)
    print(f"{what}: path {path}, final_err {rh.final_err:.17g} (fresh {rf.final_err:.17g}), iters {rh.iters} ({rf.iters}), "
          f"flag {rh.flag} ({rf.flag})")
    assert (rh.iters, rh.flag) == (rf.iters, rf.flag), what
    assert abs(rh.final_err - rf.final_err) <= 1e-10 * rf.final_err, what
    for x, y in zip(F.get_params(), H.get_params()):
        close(y, x, 1e-10, f"{what}: parameters after 10 LM iterations")
    F.close()


def test_reupload_equals_fresh_handle(monkeypatch):
    monkeypatch.delenv("PSBA_SCHUR_OWNER", raising=False)
    p54, p7 = _prob("54"), _prob("7")
    rng = np.random.default_rng(5)
    H = psba_amd.Psba(0)

    # 1: every kind of per-problem state gets dirty, the linearization queued ahead by the LM loop included
    H.upload_problem(p54)
    _same_as_fresh(H, p54, 0, "first upload")
    H.reset_params()
    H.set_distortion(random_kc(rng, p54["nC"]))
    H.set_obs_covariance(random_spd(rng, p54["nO"]))
    H.set_robust_loss(capi.LOSS_HUBER, 2.0)
    fc = np.zeros(p54["nC"], dtype=np.uint8)
    fc[:2] = 1
    H.set_fixed(cams=fc)
    H.levmar(max_iter=3)
    assert H.lens_model() == (True, True) and H.robust_loss() == (capi.LOSS_HUBER, 2.0) and H.fixed_counts() == (2, 0)

    # 2: every dimension shrinks, n32 changes
    H.upload_problem(p7)
    _same_as_fresh(H, p7, 0, "54 -> 7 cameras")

    # 3: the owner route, forced
    monkeypatch.setenv("PSBA_SCHUR_OWNER", "1")
    H.upload_problem(p54)
    _same_as_fresh(H, p54, 1, "7 -> 54 cameras, owner route")

    # 4: the LDS route again: a stale owner plan must not be taken
    monkeypatch.delenv("PSBA_SCHUR_OWNER")
    H.upload_problem(p54)
    _same_as_fresh(H, p54, 0, "owner route -> LDS route")

    # (5, dense -> PSBA_SOLVER_PCG -> dense: psba_set_solver refuses the switch on a handle that holds a problem)
    with pytest.raises(capi.PsbaError) as exc:
        H.set_solver(SOLVER_PCG)
    assert exc.value.code == E_STATE

    # 6: a rejected upload (observations not point-major) leaves the old problem usable.  "Reproduces its residual
    # exactly": the residual per observation (one thread each, no atomics) bit for bit.  The cost itself is summed with
    # one fp64 atomic add per workgroup, in whatever order the workgroups retire -- two calls on an untouched handle
    # differ in the last bit (seen: 4873.489767645002 / ...003) -- so it is held to the rounding of that sum: at most
    # 256 non-negative terms (the grid is capped there) in another order, |diff| <= 256 eps cost
    e, cost = H.compute_exQT(), H.residual(0)
    bad = capi.Problem(p54)
    for k in ("iidx", "jidx", "impts"):
        a = np.array(p54[k])
        a[[0, -1]] = a[[-1, 0]]
        bad[k] = a
    with pytest.raises(capi.PsbaError) as exc:
        H.upload_problem(bad)
    assert exc.value.code == E_INVALID
    assert H.schur_path() == 0
    again = H.residual(0)
    print(f"rejected upload: residual before {cost:.17g}, after {again:.17g}")
    assert np.array_equal(H.compute_exQT(), e)
    assert abs(again - cost) <= 256 * np.finfo(float).eps * cost
    H.close()
