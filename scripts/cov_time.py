"""HIP-event times of one psba_covariance_compute(reassemble = 1), split into the existing linearize + assemble
(psba_profile_get: K1, K2, the S-reduce) and the new factor, inverse and points (psba_covariance_times), on the
54-camera golden problem, the venice-shaped problem (52 cameras) and an 850-camera synthetic one, cameras 0 and 1 fixed,
mu = 0 -- beside one LM iteration of the same problem on the same handle (the loop's code is not touched by the
covariance).  Every figure is the mean of the middle half of the timed runs (one warm-up run first).
Usage: python scripts/cov_time.py [--runs N] [--problems 54,venice,850]"""
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


def middle(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    q = len(v) // 4
    return float(v[q:len(v) - q].mean())


def problem(name):
    if name == "54":
        from sba_text import KK
        data = os.path.join(ROOT, "tests", "golden", "data")
        return psba_amd.read_problem(os.path.join(data, "54cams.txt"), os.path.join(data, "54pts.txt"), KK)
    if name == "venice":
        return synth.venice_shaped()
    if name == "850":
        return synth.make_problem(850, 30000, 6.0, 0x5BA0 + 5)
    raise SystemExit(f"unknown problem {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--problems", default="54,venice,850")
    args = ap.parse_args()
    for name in args.problems.split(","):
        prob = problem(name)
        fc = np.zeros(prob["nC"], dtype=np.uint8)
        fc[:2] = 1
        h = psba_amd.Psba(0)
        h.upload_problem(prob)
        h.set_fixed(fc, None)
        rows = []
        for run in range(args.runs + 1):
            h.reset_params()  # the linearization is part of the timed compute
            h.profile_enable(True)
            h.profile_reset()
            t0 = time.perf_counter()
            st = h.covariance(0.0, 1.0)
            wall = 1e3 * (time.perf_counter() - t0)
            if st != capi.PSBA_OK:
                raise SystemExit(f"{name}: psba_covariance_compute returned {st}")
            lin = sum(h.profile_get(k)[0] for k in (capi.K_LINEARIZE, capi.K_SCHUR, capi.K_SCHUR_REDUCE))
            h.profile_enable(False)
            if run:
                rows.append([lin, *h.covariance_times(), wall])
        lm = []
        for run in range(args.runs + 1):
            h.reset_params()
            res, _ = h.levmar(max_iter=10)
            if run:
                lm.append(1e3 * res.seconds / max(res.iters, 1))
        rows = np.asarray(rows)
        lin, fac, inv, pts, wall = (middle(rows[:, k]) for k in range(5))
        n32 = (6 * prob["nC"] + 31) // 32 * 32
        print(f"{name}: {prob['nC']} cameras (n32 = {n32}), {prob['nP']} points, {prob['nO']} observations; "
              f"{args.runs} runs, ms: linearize+assemble {lin:.3f}  factor {fac:.3f}  inverse {inv:.3f}  points {pts:.3f}  "
              f"whole call (host clock) {wall:.3f}  |  one LM iteration {middle(lm):.3f}", flush=True)
        h.close()


if __name__ == "__main__":
    main()
