"""Development helper: the band scene of 2050 cameras as blocks of 16 under PSBA_SOLVER_SPARSE, ungrouped
against psba_set_sparse_intrinsics_groups with one group, eight contiguous groups and labels j % 3 -- alternated in one
process, two rounds, so that the run-to-run spread of the ungrouped handle shows beside the grouped figures.  Per class
of psba_profile_get, the iterations of the conjugate gradients, and the device memory of the handle."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import psba_amd
from psba_amd import capi
import freepcg_ref as fp
import shared_ref as sr
from freekd_twin import BAL, start_kc

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2050
scene = fp.band_scene(N)
LABELS = {"ungrouped": None, "one group": np.zeros(N, dtype=np.int32),
          "eight contiguous": (np.arange(N) * 8 // N).astype(np.int32), "j % 3": (np.arange(N) % 3).astype(np.int32)}


def used_mib():
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 2.0 ** 20


for rnd in range(2):
    for name, lab in LABELS.items():
        p, kc = (scene, start_kc(N)) if lab is None else sr.share_problem(scene, start_kc(N), lab)
        before = used_mib()
        h = psba_amd.Psba(0)
        h.set_solver(psba_amd.SOLVER_SPARSE, tol=1e-10, max_iter=2000)
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        h.upload_problem(p)
        h.set_distortion(kc)
        h.set_intrinsics_mask(BAL)
        if lab is not None:
            h.set_sparse_intrinsics_groups(lab)
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        h.profile_enable(True)
        for _ in range(2):
            h.schur_assemble(mu); h.schur_solve(); h.backsub(mu)
        h.profile_reset()
        reps = 5
        for _ in range(reps):
            h.schur_assemble(mu); h.schur_solve(); h.backsub(mu)
        out = []
        for what, k in (("schur", capi.K_SCHUR), ("solve", capi.K_CHOLESKY), ("backsub", capi.K_BACKSUB)):
            ms, n = h.profile_get(k)
            out.append(f"{what} {1e3 * ms / reps:9.1f} us")
        it, rel, nb, nd = h.pcg_info()
        ms, _ = h.profile_get(capi.K_CHOLESKY)
        mem = used_mib() - before
        print(f"round {rnd} {N} cameras {name:17s}: " + ", ".join(out) + f", iterations {it} (relres {rel:.1e}), "
              f"solve / iteration {1e3 * ms / reps / max(it, 1):7.2f} us, device memory {mem:7.1f} MiB", flush=True)
        h.close()
