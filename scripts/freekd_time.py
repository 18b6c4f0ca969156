"""ms per LM iteration and the per-class kernel times of psba_profile_get (linearize, S assembly, Cholesky,
back-substitution) with camera blocks of 11 (PSBA_CAMERA_FREE_K) and of 16 (PSBA_CAMERA_FREE_KD: all ten intrinsics
free, and the mask of Bundle Adjustment in the Large), on 54camsvarK / 54pts and on the venice-shaped problem.  The
variants are alternated within one process (one LM run of each per round), so that drift of the machine hits all of
them alike; both blocks run the kernels of kernels_free.hip.  --seg sweeps the segment length of the S assembly
(PSBA_FKD_SEG, read at upload; the sweep opens handles of the 16-block only).  --held adds every variant once more
with the poses of cameras 0 and 1 held (psba_set_held, DESIGN 7i: the same launches and the same products).  --priors
adds every variant once more with a weak diagonal prior about the start on every camera and on every 16th point
(psba_set_priors, DESIGN 7j: the PRIOR instantiations of the same launches, two more cost kernels per psba_residual;
the variant without is the PRIOR = false code).  --weights adds every variant once more with Cauchy, c = 2, and sigmas
drawn log-uniform in [0.5, 2] (psba_set_obs_weighting, DESIGN 7k: the WGT instantiations of the same launches; the
variant without is the WGT = false code).  --problem wide65 is tests/freekd_twin.py's wide_problem(65).
Usage: python scripts/freekd_time.py [--rounds N] [--iters N] [--seg 16,64,256] [--problem p54|venice|both|wide65]
       [--held] [--priors] [--weights]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import psba_amd  # noqa: E402
from psba_amd import synth  # noqa: E402

CLASSES = [("linearize", 0), ("S assembly", 1), ("Cholesky", 2), ("back-subst.", 3)]


def open_handle(prob, model, free, seg, held=False, priors=False, weights=False):
    if seg:
        os.environ["PSBA_FKD_SEG"] = str(seg)
    else:
        os.environ.pop("PSBA_FKD_SEG", None)
    h = psba_amd.Psba(0)
    h.set_camera_model(model)
    h.upload_problem(prob)
    if model == psba_amd.CAMERA_FREE_KD:
        h.set_intrinsics_mask(free)
    if held:
        poses = np.zeros(prob["nC"], dtype=np.uint8)
        poses[:2] = 1
        h.set_held(poses, None)
    if priors:
        cams, pts = h.get_params(0)
        pt_info = np.zeros(pts.shape)
        pt_info[::16] = 1e-6
        h.set_priors(cams, np.full(cams.shape, 1e-6), pts, pt_info)
    if weights:
        sigma = np.exp(np.random.default_rng(5).uniform(np.log(0.5), np.log(2.0), int(prob["nO"])))
        h.set_obs_weighting(psba_amd.LOSS_CAUCHY, 2.0, sigma)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seg", default="")
    ap.add_argument("--problem", default="both")
    ap.add_argument("--held", action="store_true")
    ap.add_argument("--priors", action="store_true")
    ap.add_argument("--weights", action="store_true")
    args = ap.parse_args()
    data = os.path.join(ROOT, "tests", "golden", "data")
    probs = []
    if args.problem in ("p54", "both"):
        probs.append(("54camsvarK", psba_amd.read_problem(os.path.join(data, "54camsvarK.txt"), os.path.join(data, "54pts.txt"))))
    if args.problem in ("venice", "both"):
        probs.append(("venice-shaped", synth.venice_shaped()))
    if args.problem == "wide65":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from freekd_twin import wide_problem
        probs.append(("wide_problem(65)", wide_problem(65)))
    segs = [int(s) for s in args.seg.split(",") if s] or [0]
    for pname, prob in probs:
        print(f"{pname}: {prob['nC']} cameras, {prob['nP']} points, {prob['nO']} observations; {args.iters} LM iterations "
              f"per run, {args.rounds} rounds (+1 warm-up)", flush=True)
        variants = [("FREE_K (11)", psba_amd.CAMERA_FREE_K, None, 0)]
        for s in segs:
            tag = f" L={s}" if s else ""
            variants.append((f"FREE_KD all free{tag}", psba_amd.CAMERA_FREE_KD, None, s))
            variants.append((f"FREE_KD f,k1,k2{tag}", psba_amd.CAMERA_FREE_KD, psba_amd.INTRINSICS_BAL, s))
        variants = [v + (False,) for v in variants]
        if args.held:
            variants = [w for v in variants for w in (v, (v[0] + " held", v[1], v[2], v[3], True))]
        variants = [v + (False,) for v in variants]
        if args.priors:
            variants = [w for v in variants for w in (v, (v[0] + " priors",) + v[1:5] + (True,))]
        variants = [v + (False,) for v in variants]
        if args.weights:
            variants = [w for v in variants for w in (v, (v[0] + " weights",) + v[1:6] + (True,))]
        handles = [(name, open_handle(prob, model, free, s, held, pri, wgt)) for name, model, free, s, held, pri, wgt in variants]
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
            print(f"  {name:33s} ms/try median {np.median(ms[name]):.4f} (min {min(ms[name]):.4f} max {max(ms[name]):.4f}); "
                  f"per try: " + "  ".join(parts) + f"  [{res.tries} tries, cost {res.init_err:.4e} -> {res.final_err:.4e}]",
                  flush=True)
            h.close()


if __name__ == "__main__":
    main()
