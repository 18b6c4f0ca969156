"""A bounded soak of the try-scalar handshake (psba_amd/csrc/scal_publish.h): fresh-handle psba_levmar runs
of ten iterations on the pair in which the stale block was captured -- wide_problem(65), PSBA_CAMERA_FREE_KD,
Marquardt damping, the dense solver, alternately a handle with a table of per-camera masks whose rows are all
{f, k1, k2} and a handle with that global mask and no table.  Every log is compared bit for bit with the first of its
kind, and psba_publish_stats is read before each handle is closed.

The size comes from DESIGN 7n's own rate, 10 stale readings in about 265 000 tries: the script stops once --tries
(default 265 000, which predicts ten) damping tries have run, or after --seconds, whichever comes first.  It measures
wrong values, not faults: it stops at the first call that fails.  One line per --report runs, and one JSON line at
the end: runs, tries, takes, torn (tries that met a torn reading: the wanted stamp over a block that failed its
check, read again), odd (logs that differ from the first).  odd must be 0; torn > 0 shows the located cause at work
and caught, torn = 0 shows nothing either way.
--package-root DIR imports psba_amd from another checkout (a build without psba_publish_stats: only odd is counted).
Usage: python scripts/publish_soak.py [--tries N] [--seconds S] [--iters N] [--report N] [--package-root DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_K1_K2 = (1, 0, 0, 0, 0, 1, 1, 0, 0, 0)
ALL = (1,) * 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tries", type=int, default=265000)
    ap.add_argument("--seconds", type=float, default=900.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--report", type=int, default=2000)
    ap.add_argument("--package-root", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(args.package_root) if args.package_root else ROOT)
    import psba_amd
    from freekd_twin import start_kc, wide_problem

    prob = wide_problem(65)
    kc = start_kc(prob["nC"])
    table = np.tile(np.asarray(F_K1_K2, dtype=np.uint8).reshape(1, 10), (prob["nC"], 1))
    stats = hasattr(psba_amd.Psba, "publish_stats")
    first, runs, tries, takes, torn, odd = {}, 0, 0, 0, 0, []
    t0 = time.time()
    while tries < args.tries and time.time() - t0 < args.seconds:
        kind = "table" if runs % 2 == 0 else "global"
        h = psba_amd.Psba(0)
        try:
            h.set_camera_model(psba_amd.CAMERA_FREE_KD)
            h.upload_problem(prob)
            h.set_distortion(kc)
            h.set_intrinsics_mask(ALL if kind == "table" else F_K1_K2)
            h.set_damping(psba_amd.DAMPING_MARQUARDT, 0.0, 0.0)
            if kind == "table":
                h.set_camera_masks(table)
            res, log = h.levmar(max_iter=args.iters, tr_handoff=False, log_cap=256)
            if stats:
                a, b = h.publish_stats()
                takes += a
                torn += b
        finally:
            h.close()
        blob = log.tobytes()
        if first.setdefault(kind, blob) != blob:
            odd.append(runs)
            print(f"run {runs} ({kind}): its log differs from the first\n{log}", flush=True)
        runs += 1
        tries += res.tries
        if runs % args.report == 0:
            print(f"{runs} runs, {tries} tries, takes {takes}, torn {torn}, odd {len(odd)}, {time.time() - t0:.0f} s", flush=True)
    same_kinds = len(first) == 2 and first["table"] == first["global"]
    print(json.dumps(dict(runs=runs, tries=tries, takes=takes if stats else None, torn=torn if stats else None,
                          odd=len(odd), odd_runs=odd[:20], table_equals_global=same_kinds, iters=args.iters,
                          seconds=round(time.time() - t0, 1), complete=tries >= args.tries)), flush=True)
    return 1 if odd else 0


if __name__ == "__main__":
    sys.exit(main())
