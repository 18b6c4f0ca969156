"""HIP-event times of one psba_free_covariance_compute(reassemble = 1) with camera blocks of 11 (PSBA_CAMERA_FREE_K) and
of 16 (PSBA_CAMERA_FREE_KD: all ten intrinsics free, and the mask {f, k1, k2}), split into the existing linearize +
assemble (psba_profile_get) and the factor, inverse and points of psba_free_covariance_times, on 54camsvarK / 54pts and
on the venice-shaped problem, the poses of cameras 0 and 1 held, mu = 1e-6 of the largest diagonal entry (two of the
three routes are singular at mu = 0 with holds alone) -- beside one LM iteration of the same handle, and beside the
point kernel of the fixed-K covariance (psba_covariance_compute, cameras 0 and 1 fixed) on the same geometry, scaled by
(cnp / 6)^2 products.  Every figure is the mean of the middle half of the timed runs (one warm-up run first).
Usage: python scripts/freecov_time.py [--runs N] [--problems p54,venice]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import psba_amd  # noqa: E402
from psba_amd import capi, synth  # noqa: E402

ROUTES = [("FREE_K (11)", psba_amd.CAMERA_FREE_K, None), ("FREE_KD all free", psba_amd.CAMERA_FREE_KD, None),
          ("FREE_KD f,k1,k2", psba_amd.CAMERA_FREE_KD, psba_amd.INTRINSICS_BAL)]


def middle(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    q = len(v) // 4
    return float(v[q:len(v) - q].mean())


def problems(name):
    """(the problem of the free routes, the same geometry for six-parameter blocks)"""
    if name == "p54":
        from sba_text import KK
        data = os.path.join(ROOT, "tests", "golden", "data")
        return (psba_amd.read_problem(os.path.join(data, "54camsvarK.txt"), os.path.join(data, "54pts.txt")),
                psba_amd.read_problem(os.path.join(data, "54cams.txt"), os.path.join(data, "54pts.txt"), KK))
    if name == "venice":
        p = synth.venice_shaped()
        return p, p
    raise SystemExit(f"unknown problem {name}")


def fixed_points_ms(prob, runs):
    """k_cov_points of the fixed-K covariance on the geometry: middle mean of `runs` computes"""
    fc = np.zeros(prob["nC"], dtype=np.uint8)
    fc[:2] = 1
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    h.set_fixed(fc, None)
    h.linearize(1.0, 1.0)
    mu = 1e-6 * h.max_diag()
    ms = []
    for run in range(runs + 1):
        if h.covariance(mu, 1.0) != capi.PSBA_OK:
            raise SystemExit("psba_covariance_compute failed")
        if run:
            ms.append(h.covariance_times()[2])
    h.close()
    return middle(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--problems", default="p54,venice")
    args = ap.parse_args()
    for name in args.problems.split(","):
        prob, prob6 = problems(name)
        pts6 = fixed_points_ms(prob6, args.runs)
        print(f"{name}: {prob['nC']} cameras, {prob['nP']} points, {prob['nO']} observations; {args.runs} runs; the fixed-K "
              f"point kernel on this geometry {pts6:.3f} ms", flush=True)
        for rname, model, free in ROUTES:
            h = psba_amd.Psba(0)
            h.set_camera_model(model)
            h.upload_problem(prob)
            if model == psba_amd.CAMERA_FREE_KD:
                h.set_intrinsics_mask(free)
            poses = np.zeros(prob["nC"], dtype=np.uint8)
            poses[:2] = 1
            h.set_held(poses, None)
            cnp = h.camera_block()
            h.linearize(1.0, 1.0)
            mu = 1e-6 * h.max_diag()
            rows = []
            for run in range(args.runs + 1):
                h.reset_params()  # the linearization is part of the timed compute
                h.profile_enable(True)
                h.profile_reset()
                t0 = time.perf_counter()
                st = h.free_covariance(mu, 1.0)
                wall = 1e3 * (time.perf_counter() - t0)
                if st != capi.PSBA_OK:
                    raise SystemExit(f"{name} {rname}: psba_free_covariance_compute returned {st}")
                lin = sum(h.profile_get(k)[0] for k in (capi.K_LINEARIZE, capi.K_SCHUR))
                h.profile_enable(False)
                if run:
                    rows.append([lin, *h.free_covariance_times(), wall])
            lm = []
            for run in range(args.runs + 1):
                h.reset_params()
                res, _ = h.levmar(max_iter=10)
                if run:
                    lm.append(1e3 * res.seconds / max(res.iters, 1))
            rows = np.asarray(rows)
            lin, fac, inv, pts, wall = (middle(rows[:, k]) for k in range(5))
            n32 = (cnp * prob["nC"] + 31) // 32 * 32
            print(f"  {rname:17s} n32 = {n32}, ms: linearize+assemble {lin:.3f}  factor {fac:.3f}  inverse {inv:.3f}  "
                  f"points {pts:.3f} (fixed-K x (cnp/6)^2 = {pts6 * (cnp / 6.0) ** 2:.3f})  whole call (host clock) {wall:.3f}"
                  f"  |  one LM iteration {middle(lm):.3f}", flush=True)
            h.close()


if __name__ == "__main__":
    main()
