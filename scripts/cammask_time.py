"""ms per damping try and the per-class kernel times of psba_profile_get (linearize, S assembly, Cholesky,
back-substitution) of PSBA_CAMERA_FREE_KD with per-camera masks (psba_set_camera_masks), on 54camsvarK /
54pts and on the venice-shaped problem, all ten intrinsics free globally.  Three handles: one that never set a table
(it runs the code of a build without the verb: no load of the table), one with the mixed table (by j % 4: all free,
{fu, k1, k2}, none, {fu}) and one whose rows are all none.  The variants are alternated within one process (one LM
run of each per round), so that drift of the machine hits all of them alike.  Nothing is gated on these times.
--package-root DIR imports psba_amd from another checkout and runs the no-table handle alone: the figures of a build
without the verb (the parent commit) from the same script on the same box, to hold the no-table handle against.
Usage: python scripts/cammask_time.py [--rounds N] [--iters N] [--problem p54|venice|both] [--package-root DIR]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [("linearize", 0), ("S assembly", 1), ("Cholesky", 2), ("back-subst.", 3)]
ROWS = np.array([[1] * 10, [1, 0, 0, 0, 0, 1, 1, 0, 0, 0], [0] * 10, [1] + [0] * 9], dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--problem", default="both")
    ap.add_argument("--package-root", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root) if args.package_root else ROOT)
    import psba_amd
    from psba_amd import synth

    def open_handle(prob, table):
        h = psba_amd.Psba(0)
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        h.upload_problem(prob)
        if table is not None:
            h.set_camera_masks(table)
        return h
    data = os.path.join(ROOT, "tests", "golden", "data")
    probs = []
    if args.problem in ("p54", "both"):
        probs.append(("54camsvarK", psba_amd.read_problem(os.path.join(data, "54camsvarK.txt"), os.path.join(data, "54pts.txt"))))
    if args.problem in ("venice", "both"):
        probs.append(("venice-shaped", synth.venice_shaped()))
    for pname, prob in probs:
        nC = prob["nC"]
        print(f"{pname}: {nC} cameras, {prob['nP']} points, {prob['nO']} observations; {args.iters} LM iterations per run, "
              f"{args.rounds} rounds (+1 warm-up)" + (f"; psba_amd of {args.package_root}" if args.package_root else ""), flush=True)
        variants = [("no table", None)]
        if not args.package_root:
            variants += [("mixed table", ROWS[np.arange(nC) % 4]), ("all none", np.zeros((nC, 10), dtype=np.uint8))]
        handles = [(name, open_handle(prob, table)) for name, table in variants]
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
