"""Development helper: psba_sparse_point_covariance beside the single-column solver it is measured against,
on 7m's inputs -- wide_problem(300, nP=1200) and the band of 2050 cameras, blocks of 11 and 16.  Per case:
  * psba_schur_solve (one right-hand side): HIP-event ms of the solve and its iterations (psba_profile_get, K_CHOLESKY),
    and 3 x that per point, the yardstick (7o's);
  * the verb for 1, 5 and 40 chosen points (one column triple, one full panel, one full batch): HIP-event ms of its
    solves and contraction (the same profile class), wall ms of the whole call, the iterations per column (min / mean /
    max) and ms per iteration of the batch.
Means of REPS calls after WARM warm-ups, one process.  Usage: python scripts/sparse_ptcov_time.py [wide|band]
[fk|kd-bal] [n1|n5|n40]."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import psba_amd  # noqa: E402
from psba_amd import capi  # noqa: E402
import freepcg_ref as fp  # noqa: E402
from freekd_twin import BAL, start_kc, wide_problem  # noqa: E402

WARM, REPS = 2, 5


def open_handle(p, route):
    h = psba_amd.Psba(0)
    h.set_solver(psba_amd.SOLVER_SPARSE, tol=1e-10, max_iter=2000)
    if route == "fk":
        h.set_camera_model(psba_amd.CAMERA_FREE_K)
        h.upload_problem(p)
    else:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        h.upload_problem(p)
        h.set_distortion(start_kc(p["nC"]))
        h.set_intrinsics_mask(BAL)
    return h


def timed(h, call):
    for _ in range(WARM):
        call()
    h.profile_reset()
    t0 = time.perf_counter()
    for _ in range(REPS):
        out = call()
    wall = 1e3 * (time.perf_counter() - t0) / REPS
    ms, n = h.profile_get(capi.K_CHOLESKY)
    return out, ms / REPS, wall


def main():
    kinds = [a for a in sys.argv[1:] if a in ("wide", "band")] or ["wide", "band"]
    routes = [a for a in sys.argv[1:] if a in ("fk", "kd-bal")] or ["fk", "kd-bal"]
    counts = [int(a[1:]) for a in sys.argv[1:] if a in ("n1", "n5", "n40")] or [1, 5, 40]
    psba_amd.Psba(0).close()
    for kind in kinds:
        p = wide_problem(300, nP=1200) if kind == "wide" else fp.band_scene(2050)
        nC, nP = p["nC"], p["nP"]
        seen = np.flatnonzero(np.bincount(p["iidx"], minlength=nP) >= 3)
        for route in routes:
            h = open_handle(p, route)
            cnp = h.camera_block()
            h.linearize(1.0, 1.0)
            mu = 1e-3 * h.max_diag()
            h.profile_enable(True)

            def single():
                h.schur_assemble(mu)
                return h.schur_solve()
            # the single solve: the assembly is profiled under its own class, the solve under K_CHOLESKY
            _, ms1, _ = timed(h, single)
            it1 = h.pcg_info()[0]
            print(f"{kind} {nC} cameras, {route} (cnp {cnp}, nA {cnp * nC}): single solve {ms1:.3f} ms, {it1} iterations, "
                  f"{ms1 / max(it1, 1):.4f} ms / iteration; 3 x single per point = {3 * ms1:.3f} ms", flush=True)
            for n_sel in counts:
                sel = seen[np.linspace(0, seen.size - 1, n_sel + 2).astype(int)[1:-1]]
                (C, info), msv, wall = timed(h, lambda: h.sparse_point_covariance(sel, mu=mu))
                it = info["iters"]
                print(f"  verb, {n_sel} chosen ({3 * n_sel} columns): status {info['status']}, solves + contraction {msv:.3f} ms "
                      f"(wall of the call {wall:.3f} ms), iterations per column {it.min()} / {it.mean():.1f} / {it.max()}, "
                      f"{msv / max(int(it.max()), 1):.4f} ms / iteration of the batch; "
                      f"{3 * n_sel} single solves = {3 * n_sel * ms1:.3f} ms, ratio {msv / (3 * n_sel * ms1):.3f}", flush=True)
            h.close()


if __name__ == "__main__":
    main()
