"""Development helper: psba_sparse_camera_covariance beside the single-column solver it is measured
against, on 7m's inputs -- wide_problem(300, nP=1200) and the band of 2050 cameras, blocks of 11 and 16.  Per case:
  * psba_schur_solve (one right-hand side): HIP-event ms of the solve and its iterations (psba_profile_get, K_CHOLESKY),
    and cnp x that, the yardstick;
  * the verb for 1 and 8 chosen cameras: HIP-event ms of its solves (the same profile class), wall ms of the whole call,
    the iterations per column (min / mean / max), and ms per iteration of a batch (= one k_fpcgm_spmm + update +
    direction over all the batch's panels) beside ms per iteration of the single solve (k_fpcg_spmv + update +
    direction);
  * the device memory the handle holds before and after the verb's first call.
Means of REPS calls after WARM warm-ups, one process.  Usage: python scripts/sparse_cov_time.py [wide|band] [fk|kd-bal]
[n1|n8].  The product kernels alone: run one input, one block and one count under `rocprofv3 --kernel-trace --stats` and
read the mean durations of k_fpcgm_spmm and k_fpcg_spmv from its kernel statistics."""
import ctypes
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

WARM, REPS = 3, 10


def free_bytes():
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


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
    counts = [int(a[1:]) for a in sys.argv[1:] if a in ("n1", "n8")] or [1, 8]
    psba_amd.Psba(0).close()
    for kind in kinds:
        p = wide_problem(300, nP=1200) if kind == "wide" else fp.band_scene(2050)
        nC = p["nC"]
        for route in routes:
            free0 = free_bytes()
            h = open_handle(p, route)
            cnp = h.camera_block()
            h.linearize(1.0, 1.0)
            mu = 1e-3 * h.max_diag()
            h.profile_enable(True)
            mem_handle = free0 - free_bytes()

            def single():
                h.schur_assemble(mu)
                return h.schur_solve()
            # the single solve: the assembly is profiled under its own class, the solve under K_CHOLESKY
            _, ms1, _ = timed(h, single)
            it1 = h.pcg_info()[0]
            print(f"{kind} {nC} cameras, {route} (cnp {cnp}, nA {cnp * nC}): single solve {ms1:.3f} ms, {it1} iterations, "
                  f"{ms1 / max(it1, 1):.4f} ms / iteration; cnp x single = {cnp * ms1:.3f} ms", flush=True)
            for n_sel in counts:
                sel = np.linspace(0, nC - 1, n_sel + 2).astype(int)[1:-1]
                (C, info), msv, wall = timed(h, lambda: h.sparse_camera_covariance(sel, mu=mu))
                it = info["iters"]
                # the assembly inside the verb is profiled under its own class; a batch iterates until its slowest column stops
                print(f"  verb, {n_sel} chosen ({cnp * n_sel} columns): status {info['status']}, solves {msv:.3f} ms (wall of the call "
                      f"{wall:.3f} ms), iterations per column (a dead column counts 0) {it.min()} / {it.mean():.1f} / {it.max()}, "
                      f"{msv / max(int(it.max()), 1):.4f} ms / iteration of the batch; "
                      f"{cnp * n_sel} single solves = {cnp * n_sel * ms1:.3f} ms, ratio {msv / (cnp * n_sel * ms1):.3f}", flush=True)
            print(f"  device memory: the handle {mem_handle / 2**20:.1f} MiB, with the verb's buffers {(free0 - free_bytes()) / 2**20:.1f} MiB",
                  flush=True)
            h.close()


if __name__ == "__main__":
    main()
