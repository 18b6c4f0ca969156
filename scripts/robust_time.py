"""ms per LM iteration on the venice-shaped problem (5 % of its observations moved by 20-80 px) with each robust loss,
with and without covariances, and the K1, K3 and residual times of psba_profile_get.  The variants are alternated
within one process (one LM run of each per round), so that drift of the machine hits all of them alike.
Usage: python scripts/robust_time.py [--rounds N] [--iters N]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psba_amd  # noqa: E402
from psba_amd import synth  # noqa: E402

LOSSES = [("plain", psba_amd.LOSS_NONE), ("huber", psba_amd.LOSS_HUBER), ("cauchy", psba_amd.LOSS_CAUCHY),
          ("soft_l1", psba_amd.LOSS_SOFT_L1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scale", type=float, default=2.0)
    args = ap.parse_args()
    prob, _ = synth.add_outliers(synth.venice_shaped(), 0.05, 20.0, 80.0, 0)
    rng = np.random.default_rng(0)
    G = rng.normal(scale=0.3, size=(prob["nO"], 2, 2))
    cov = G @ np.transpose(G, (0, 2, 1)) + np.eye(2)[None]
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    print(f"venice-shaped + 5 % outliers: {prob['nC']} cameras, {prob['nP']} points, {prob['nO']} observations; "
          f"{args.iters} LM iterations per run, {args.rounds} rounds (+1 warm-up), c = {args.scale}")
    variants = [(f"{ln}{'+cov' if cv else ''}", lk, cv) for cv in (False, True) for ln, lk in LOSSES]

    def setup(lk, cv):
        h.set_obs_covariance(cov if cv else None)
        h.set_robust_loss(lk, args.scale)
        h.reset_params()

    ms = {v[0]: [] for v in variants}
    tries = {v[0]: [] for v in variants}
    h.profile_enable(False)
    for rnd in range(args.rounds + 1):
        for name, lk, cv in variants:
            setup(lk, cv)
            res, _ = h.levmar(max_iter=args.iters)
            if rnd:  # round 0 warms up
                ms[name].append(1e3 * res.seconds / max(res.iters, 1))
                tries[name].append(res.tries / max(res.iters, 1))
    kt = {}
    for name, lk, cv in variants:
        setup(lk, cv)
        h.profile_enable(True)
        h.profile_reset()
        h.levmar(max_iter=args.iters)
        kt[name] = {}
        for kn, kk in [("K1", 0), ("K3", 3), ("residual", 4)]:
            t, n = h.profile_get(kk)
            kt[name][kn] = 1e3 * t / max(n, 1)
        h.profile_enable(False)
    for name, _, cv in variants:
        base = "plain+cov" if cv else "plain"
        m = np.median(ms[name])
        print(f"{name:13s} ms/iter median {m:.4f} (min {min(ms[name]):.4f} max {max(ms[name]):.4f}, "
              f"x{m / np.median(ms[base]):.3f} of {base}; tries/iter {np.mean(tries[name]):.2f});  "
              + "  ".join(f"{kn} {v:.1f} us (x{v / kt[base][kn]:.3f})" for kn, v in kt[name].items()), flush=True)
    h.close()


if __name__ == "__main__":
    main()
