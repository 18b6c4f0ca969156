"""ms per LM iteration on the venice-shaped problem with fixed parameter blocks (psba_set_fixed): no mask, cameras
{0, 1}, cameras {0, 1} + 10 % of the points, and every camera fixed with the structure-only shortcut and without it
(PSBA_FIXED_NO_SHORTCUT=1), with the K1, K2, Cholesky and K3 times of psba_profile_get.  The variants are alternated
within one process (one LM run of each per round), so that drift of the machine hits all of them alike.
Usage: python scripts/fixed_time.py [--rounds N] [--iters N]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psba_amd  # noqa: E402
from psba_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    prob = synth.venice_shaped()
    nC, nP = prob["nC"], prob["nP"]
    rng = np.random.default_rng(0)
    two = np.zeros(nC, dtype=np.uint8)
    two[:2] = 1
    tenth = np.zeros(nP, dtype=np.uint8)
    tenth[rng.choice(nP, nP // 10, replace=False)] = 1
    allc = np.ones(nC, dtype=np.uint8)
    # (name, fixed cameras, fixed points, PSBA_FIXED_NO_SHORTCUT)
    variants = [("none", None, None, False), ("cams01", two, None, False), ("cams01+10%pts", two, tenth, False),
                ("all cams", allc, None, False), ("all cams, general route", allc, None, True)]
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    print(f"venice-shaped: {nC} cameras, {nP} points, {prob['nO']} observations; {args.iters} LM iterations per run, "
          f"{args.rounds} rounds (+1 warm-up)")

    def setup(fc, fp, general):
        if general:
            os.environ["PSBA_FIXED_NO_SHORTCUT"] = "1"
        else:
            os.environ.pop("PSBA_FIXED_NO_SHORTCUT", None)
        h.set_fixed(fc, fp)
        h.reset_params()

    ms = {v[0]: [] for v in variants}
    tries = {v[0]: [] for v in variants}
    h.profile_enable(False)
    for rnd in range(args.rounds + 1):
        for name, fc, fp, general in variants:
            setup(fc, fp, general)
            res, _ = h.levmar(max_iter=args.iters)
            if rnd:  # round 0 warms up
                ms[name].append(1e3 * res.seconds / max(res.iters, 1))
                tries[name].append(res.tries / max(res.iters, 1))
    kt = {}
    kinds = [("K1", psba_amd.capi.K_LINEARIZE), ("K2", psba_amd.capi.K_SCHUR), ("chol", psba_amd.capi.K_CHOLESKY),
             ("K3", psba_amd.capi.K_BACKSUB)]
    for name, fc, fp, general in variants:
        setup(fc, fp, general)
        h.profile_enable(True)
        h.profile_reset()
        h.levmar(max_iter=args.iters)
        kt[name] = {}
        for kn, kk in kinds:
            t, n = h.profile_get(kk)
            kt[name][kn] = (1e3 * t / n, n) if n else (0.0, 0)
        h.profile_enable(False)
    os.environ.pop("PSBA_FIXED_NO_SHORTCUT", None)
    base = np.median(ms["none"])
    for name, _, _, _ in variants:
        m = np.median(ms[name])

        def fmt(kn):
            v, n = kt[name][kn]
            b = kt["none"][kn][0]
            return f"{kn} {v:.1f} us (x{v / b:.3f}, {n} launches)" if n else f"{kn} not launched"

        print(f"{name:24s} ms/iter median {m:.4f} (min {min(ms[name]):.4f} max {max(ms[name]):.4f}, x{m / base:.3f} of "
              f"none; tries/iter {np.mean(tries[name]):.2f});  " + "  ".join(fmt(kn) for kn, _ in kinds), flush=True)
    h.close()


if __name__ == "__main__":
    main()
