"""The two damping rules of the free-intrinsics route (psba_set_damping) on one handle in one process:
ms per damping try and per LM iteration of PSBA_CAMERA_FREE_KD with the mask {f, k1, k2} on 54camsvarK / 54pts under
N + mu I and under N + mu D, alternated round by round so that drift of the machine hits both alike, and the
per-class kernel times of psba_profile_get.  --ring adds the count of iterations and damping tries either rule needs
to reach 1e-15 of the initial cost on the noise-free ring scene of tests/freekd_twin.py.
On a tree without psba_set_damping the script times the identity rule alone (the figure to compare a parent commit by).
Usage: python scripts/damping_time.py [--rounds N] [--iters N] [--ring]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import psba_amd  # noqa: E402

CLASSES = [("linearize", 0), ("S assembly", 1), ("Cholesky", 2), ("back-subst.", 3)]
HAS_DAMPING = hasattr(psba_amd.Psba, "set_damping")
RULES = [("identity", 0)] + ([("Marquardt", 1)] if HAS_DAMPING else [])


def set_rule(h, kind):
    if HAS_DAMPING:
        h.set_damping(kind)


def time_rules(args):
    data = os.path.join(ROOT, "tests", "golden", "data")
    prob = psba_amd.read_problem(os.path.join(data, "54camsvarK.txt"), os.path.join(data, "54pts.txt"))
    print(f"54camsvarK: {prob['nC']} cameras, {prob['nP']} points, {prob['nO']} observations; {args.iters} LM iterations "
          f"per run, {args.rounds} rounds (+1 warm-up), rules alternated on one handle", flush=True)
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(prob)
    h.set_intrinsics_mask(psba_amd.INTRINSICS_BAL)
    per_try = {name: [] for name, _ in RULES}
    per_it = {name: [] for name, _ in RULES}
    last = {}
    for rnd in range(args.rounds + 1):
        for name, kind in RULES:
            set_rule(h, kind)
            h.reset_params()
            res, _ = h.levmar(max_iter=args.iters)
            last[name] = res
            if rnd:  # round 0 warms up
                per_try[name].append(1e3 * res.seconds / max(res.tries, 1))
                per_it[name].append(1e3 * res.seconds / max(res.iters, 1))
    for name, kind in RULES:
        set_rule(h, kind)
        h.reset_params()
        h.profile_enable(True)
        h.profile_reset()
        res, _ = h.levmar(max_iter=args.iters)
        parts = []
        for cn, ck in CLASSES:
            t, n = h.profile_get(ck)
            parts.append(f"{cn} {1e3 * t / max(res.tries, 1):.1f} us")
        h.profile_enable(False)
        r = last[name]
        print(f"  {name:10s} ms/try median {np.median(per_try[name]):.4f} (min {min(per_try[name]):.4f} max "
              f"{max(per_try[name]):.4f}); ms/iteration median {np.median(per_it[name]):.4f} (min {min(per_it[name]):.4f} "
              f"max {max(per_it[name]):.4f}); per try: " + "  ".join(parts) +
              f"  [{r.iters} iterations, {r.tries} tries, cost {r.init_err:.4e} -> {r.final_err:.4e}]", flush=True)
    h.close()


def ring_counts():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from freekd_twin import ring_problem
    start, kc0, _, _ = ring_problem()
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(start)
    h.set_distortion(kc0)
    h.set_intrinsics_mask(psba_amd.INTRINSICS_BAL)
    for name, kind in RULES:
        set_rule(h, kind)
        h.reset_params()
        res, log = h.levmar(max_iter=40, tr_handoff=False, log_cap=512, stop_cost=-1.0)
        acc = log[log[:, 4] > 0]
        hit = np.flatnonzero(acc[:, 1] <= 1e-15 * res.init_err)
        if hit.size:
            itno = int(acc[hit[0], 0])
            tries = int(np.flatnonzero((log[:, 0] == itno) & (log[:, 4] > 0))[0]) + 1
            reach = f"1e-15 of the initial cost after {itno + 1} iterations / {tries} tries"
        else:
            reach = "1e-15 of the initial cost not reached"
        print(f"  ring scene, {name:10s} mu0 {res.mu0:.3e}: {reach}; costs of the first accepted steps "
              + " ".join(f"{c:.1e}" for c in acc[:12, 1]) + f"; end {res.final_err:.3e} of {res.init_err:.3e} after "
              f"{res.iters} iterations / {res.tries} tries (flag {res.flag})", flush=True)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ring", action="store_true")
    args = ap.parse_args()
    time_rules(args)
    if args.ring:
        ring_counts()


if __name__ == "__main__":
    main()
