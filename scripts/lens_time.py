"""ms per LM iteration on the venice-shaped problem with the four lens models (plain / distortion / covariance /
both), and the K1, K3 and residual times of psba_profile_get.  Usage: python scripts/lens_time.py [--reps N]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psba_amd  # noqa: E402
from psba_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    prob = synth.venice_shaped()
    rng = np.random.default_rng(0)
    kc = np.column_stack([0.1 + 0.01 * rng.normal(size=prob["nC"]), -0.05 * np.ones(prob["nC"]),
                          1e-4 * rng.normal(size=prob["nC"]), 1e-4 * rng.normal(size=prob["nC"]), np.zeros(prob["nC"])])
    G = rng.normal(scale=0.3, size=(prob["nO"], 2, 2))
    cov = G @ np.transpose(G, (0, 2, 1)) + np.eye(2)[None]
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    print(f"venice-shaped: {prob['nC']} cameras, {prob['nP']} points, {prob['nO']} observations; "
          f"{args.iters} LM iterations x {args.reps}")
    for name, k, c in [("plain", None, None), ("distortion", kc, None), ("covariance", None, cov), ("both", kc, cov)]:
        h.set_distortion(k)
        h.set_obs_covariance(c)
        ms = []
        for rep in range(args.reps + 1):
            h.reset_params()
            h.profile_enable(False)
            res, _ = h.levmar(max_iter=args.iters)
            if rep:  # the first run warms up
                ms.append(1e3 * res.seconds / max(res.iters, 1))
        h.reset_params()
        h.profile_enable(True)
        h.profile_reset()
        h.levmar(max_iter=args.iters)
        kt = {}
        for kn, kk in [("K1", 0), ("K3", 3), ("residual", 4)]:
            t, n = h.profile_get(kk)
            kt[kn] = 1e3 * t / max(n, 1)
        h.profile_enable(False)
        print(f"{name:11s} ms/iter median {np.median(ms):.4f} (min {min(ms):.4f} max {max(ms):.4f});  "
              + "  ".join(f"{kn} {v:.1f} us" for kn, v in kt.items()), flush=True)
    h.close()


if __name__ == "__main__":
    main()
