"""ms per damping try and the per-class kernel times of psba_profile_get (linearize, S assembly, Cholesky,
back-substitution) of PSBA_CAMERA_FREE_KD with and without shared intrinsics (psba_set_intrinsics_groups),
on 54camsvarK / 54pts and on the venice-shaped problem, mask {fu, k1, k2}.  Every variant starts from the same
parameters (the K of camera j % G on every camera, kc = 0) so that the ungrouped handle -- which runs the kernels of a
handle that never set groups -- and the grouped ones do the same linearization work; the variants are alternated
within one process (one LM run of each per round), so that drift of the machine hits all of them alike.
Usage: python scripts/shared_time.py [--rounds N] [--iters N] [--groups 4] [--problem p54|venice|both]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import psba_amd  # noqa: E402
from psba_amd import synth  # noqa: E402

CLASSES = [("linearize", 0), ("S assembly", 1), ("Cholesky", 2), ("back-subst.", 3)]


def open_handle(prob, labels):
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(prob)
    h.set_intrinsics_mask(psba_amd.INTRINSICS_BAL)
    if labels is not None:
        h.set_intrinsics_groups(labels)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--problem", default="both")
    args = ap.parse_args()
    data = os.path.join(ROOT, "tests", "golden", "data")
    probs = []
    if args.problem in ("p54", "both"):
        probs.append(("54camsvarK", psba_amd.read_problem(os.path.join(data, "54camsvarK.txt"), os.path.join(data, "54pts.txt"))))
    if args.problem in ("venice", "both"):
        probs.append(("venice-shaped", synth.venice_shaped()))
    for pname, prob in probs:
        nC = prob["nC"]
        G = max(1, min(args.groups, nC))
        heads = np.arange(nC) % G
        prob = dict(prob, K=np.asarray(prob["K"], dtype=np.float64).reshape(-1, 5)[heads].copy())
        print(f"{pname}: {nC} cameras, {prob['nP']} points, {prob['nO']} observations; {args.iters} LM iterations per run, "
              f"{args.rounds} rounds (+1 warm-up)", flush=True)
        variants = [("ungrouped", None), (f"{G} groups", heads), ("1 group", np.zeros(nC, dtype=np.int32))]
        handles = [(name, open_handle(prob, labels)) for name, labels in variants]
        ms = {name: [] for name, _ in handles}
        for rnd in range(args.rounds + 1):
            for name, h in handles:
                h.reset_params()
                res, _ = h.levmar(max_iter=args.iters)
                if rnd:  # round 0 warms up
                    ms[name].append(1e3 * res.seconds / max(res.tries, 1))
        for name, h in handles:
            h.reset_params()
            h.profile_enable(True)
            h.profile_reset()
            res, _ = h.levmar(max_iter=args.iters)
            parts = []
            for cn, ck in CLASSES:
                t, n = h.profile_get(ck)
                parts.append(f"{cn} {1e3 * t / max(res.tries, 1):.1f} us")
            h.profile_enable(False)
            print(f"  {name:12s} ms/try median {np.median(ms[name]):.4f} (min {min(ms[name]):.4f} max {max(ms[name]):.4f}); "
                  f"per try: " + "  ".join(parts) + f"  [{res.tries} tries, cost {res.init_err:.4e} -> {res.final_err:.4e}]",
                  flush=True)
            h.close()


if __name__ == "__main__":
    main()
