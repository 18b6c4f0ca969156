"""The twin of the damping rules (tests/damping_twin.py) on the host: N + mu D with Marquardt's D against N + mu I on
the project's own problems (CPU only).  The figures in the docstrings are those of DESIGN 7g."""
import functools

import numpy as np

from damping_twin import DMAX, DMIN, IDENTITY, MARQUARDT, TwinDamp, damp_diag
from freekd_twin import BAL, TwinKD, ring_problem, start_kc, tiny_problem
from test_freekd_twin import P7


@functools.lru_cache(maxsize=None)
def ring_run(damping):
    start, kc0, _, _ = ring_problem()
    return TwinDamp(start, kc0, BAL).levmar(max_iter=8, stop_small=False, damping=damping)


@functools.lru_cache(maxsize=None)
def p7_run(damping):
    p = P7()
    return TwinDamp(p, start_kc(p["nC"]), BAL).levmar(max_iter=8, stop_small=False, damping=damping)


def test_identity_is_the_log_of_twinkd():
    """D = 1 and mu_0 = tau max diag: the restated loop is TwinKD.levmar, number for number"""
    start, kc0, _, _ = ring_problem()
    want, wlog = TwinKD(start, kc0, BAL).levmar(max_iter=8, stop_small=False)
    res, log = ring_run(IDENTITY)
    assert log.tobytes() == wlog.tobytes() and len(log) >= 8
    assert (res.mu0, res.final_err, res.mu_final, res.iters, res.tries) == (
        want.mu0, want.final_err, want.mu_final, want.iters, want.tries)


def test_marquardt_converges_where_identity_stalls_on_the_ring_scene():
    """8 iterations, BAL mask, no absolute stop: 4.9e-25 under mu D against 8.0e1 under mu I, of 3.8e4"""
    m, _ = ring_run(MARQUARDT)
    i, _ = ring_run(IDENTITY)
    print(f"ring: init {m.init_err:.3e}, Marquardt {m.final_err:.3e} (mu0 {m.mu0:g}), identity {i.final_err:.3e} "
          f"(mu0 {i.mu0:.3e})")
    assert m.mu0 == 1e-3 and m.init_err == i.init_err
    assert m.final_err <= 1e-15 * m.init_err
    assert i.final_err >= 1e6 * m.final_err


def test_marquardt_is_no_worse_on_real_data():
    """7camsvarK, BAL mask, start_kc, 8 iterations: 1270 against 1370"""
    m, _ = p7_run(MARQUARDT)
    i, _ = p7_run(IDENTITY)
    print(f"P7: init {m.init_err:.6e}, Marquardt {m.final_err:.6e}, identity {i.final_err:.6e}")
    assert m.final_err <= i.final_err


def test_both_clamps_bite_on_the_projects_own_inputs():
    """The GPU tests compare clamped entries for exact equality: the sets must not be empty.  tiny_problem with all
    ten free has diagonal entries of 1.1e-10 and 4.1e-10 (below dmin = 1e-6); the rotations of the ring scene reach
    1e7 (above dmax = 1e5)."""
    p = tiny_problem()
    t = TwinDamp(p, start_kc(p["nC"]), None)
    _, N, _ = t.normal()
    d = np.diag(N)
    assert np.allclose(d, t.diag_normal(), rtol=1e-13, atol=0)      # the blockwise diagonal is the dense one
    low = np.flatnonzero(d < DMIN)
    print("tiny, all free: below dmin", d[low])
    assert low.size >= 2 and np.all(d[low] > 0) and np.all(damp_diag(N)[low] == DMIN)
    assert np.array_equal(np.delete(damp_diag(N), low), np.delete(d, low))
    start, kc0, _, _ = ring_problem()
    tr = TwinDamp(start, kc0, BAL)
    dr = tr.diag_normal()
    high = np.flatnonzero(dr > 1e5)
    print(f"ring, BAL: {high.size} entries above 1e5, max {dr.max():.3e}, min {dr.min():.3e}")
    assert high.size >= 6 and dr.max() >= 1e7
    D = damp_diag(dr, DMIN, 1e5)
    assert np.all(D[high] == 1e5) and np.array_equal(np.delete(D, high), np.delete(dr, high))
    assert DMAX == 1e32 and np.all(D[:tr.nA][~tr.free_a] == 1.0)       # held coordinates: clamp(1) = 1
