"""Intrinsics shared between cameras on the 16-block route (psba_set_intrinsics_groups) on the GPU, against
the host reference tests/shared_ref.py (which derives every bound; nothing here is fitted).  Needs an MI355X.

Inputs: those of test_gpu_free_entrywise.py with the members' K and start_kc set to their representative's --
tiny_problem (both cameras one group), wide_problem(64 / 65) with the labelling shared_ref.wide_labels (a group of
64 + 65 + 63 observations, a lone camera with one observation, a group whose representative has none, singletons next
to groups of nine; either side of the finalize kernels' grid-stride boundary, which k_kd_finalize_sym and
k_kd_fold_finish share; the two fold passes have no launch cap) and wide_problem(65) with all 65 cameras one group
under the BAL mask.  Masks: all free and {fu, k1, k2}.  Dampings: 1e-3 max diag (folded, free) and 1e-6 median diag N.
  * G1  S (both triangles, padding) and e_a within shared_tol; upper == lower exactly; folded-away rows exactly zero
        off the diagonal with coeff + mu on it and e_a = 0 -- also after psba_linearize(2, -2) (placeholder 2 + mu).
  * G2  the fold alone against the 80-bit fold of the same handle's own unfolded buffer, entry by entry.
  * G3  dp_a by solve_judge, members' expanded dp and proposed intrinsics bit-identical to the representative's,
        dp_b by dpb_residual, the four try scalars on the reduced vectors.
  * G4  psba_max_diag / psba_begin against the folded maximum, relative 1e-11.
  * G5  all-singleton labels and NULL are bit-identical to a handle that never set groups; grouped runs repeat.
  * G6  psba_levmar against the shared twin's LM.   G7  recovery of the shared ring scene.   G8  the interface.
  * G1 and G3 again under Marquardt's damping (psba_set_damping) on wide-above and one-group, BAL mask, at
    mu = 1e-3 and 1e-6: D of the embedded system, mu D added once after the fold, gain_den with a shared parameter
    counted once.  The module prints the worst ratios of those cases per input and quantity."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
import shared_ref as sr
from freekd_twin import BAL, CNP, start_kc, tiny_problem, wide_problem
from test_freekd_twin import P7
from test_gpu_dense_solve import ETA_MAX

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

MASKS = {"all": fr.ALL, "bal": BAL}
CASES = [("tiny", "all"), ("tiny", "bal"), ("wide-below", "all"), ("wide-below", "bal"), ("wide-above", "all"),
         ("wide-above", "bal"), ("one-group", "bal")]
P7_LABELS = {"one": [0] * 7, "two": [0, 1, 0, 1, 0, 1, 0]}
TWIN_FLAG = {0: 3, 1: 5, 2: 4, 3: 6}   # freekd_twin's LM flags -> PSBA_ITER_CONTINUE, _DP_NO_CHANGE, _ERR, _ERR_SMALL_ENOUGH


@functools.lru_cache(maxsize=None)
def base(name):
    """(problem, labels) of a named input"""
    if name == "tiny":
        return tiny_problem(), np.zeros(2, dtype=np.int32)
    if name == "one-group":
        return wide_problem(65), np.zeros(65, dtype=np.int32)
    if name.startswith("P7"):
        return P7(), np.asarray(P7_LABELS[name[3:]], dtype=np.int32)
    nC = {"wide-below": 64, "wide-above": 65}[name]
    return wide_problem(nC), sr.wide_labels(nC).astype(np.int32)


@functools.lru_cache(maxsize=None)
def ref(name, mask):
    """(SharedRoute, its extended-precision sums, the dampings, the folded diagonal): computed once, shared"""
    p, lab = base(name)
    rt = sr.SharedRoute(p, lab, MASKS[mask])
    sm = fr.sums(rt)
    mus, fdiag = sr.dampings(rt, sm)
    return rt, sm, mus, fdiag


@functools.lru_cache(maxsize=None)
def schur_ref(name, mask, mu):
    rt = ref(name, mask)[0]
    S, ea = sr.fold(*rt.twin.schur_blocks(mu), rt.rep, rt.free, mu)
    S, ea = S.astype(np.float64), ea.astype(np.float64)
    S.setflags(write=False)
    ea.setflags(write=False)
    return S, ea


def handle(rt, groups=True):
    import psba_amd
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    h.upload_problem(rt.p)
    h.set_distortion(rt.kc)
    h.set_intrinsics_mask(rt.free)
    if groups:
        h.set_intrinsics_groups(rt.labels)
    assert h.schur_path() == 5
    return h


def read_system(h, nA):
    n32 = (nA + 31) // 32 * 32
    M = h.get_reduce_buffer().reshape(n32 + 1, n32)
    return M[:nA, :nA].copy(), M[n32, :nA].copy(), M


def check_padding(M, nA):
    n32 = M.shape[1]
    pad = np.zeros((n32 - nA, n32))
    pad[np.arange(n32 - nA), nA + np.arange(n32 - nA)] = 1.0
    assert np.array_equal(M[nA:n32], pad) and np.all(M[:nA, nA:] == 0.0) and np.all(M[n32, nA:] == 0.0)


def check_system(rt, sm, fdiag, S, ea, M, S_want, ea_want, mu_ref, placeholder, label):
    d = np.sqrt(fdiag[:rt.nA] + mu_ref)
    eS, ee = sr.scaled_errors(S, ea, S_want, ea_want, d, sm["cost"])
    print(f"{label}: S {eS / rt.tol:.3e}, e_a {ee / rt.tol:.3e} of tol {rt.tol:.3e}")
    assert eS <= rt.tol and ee <= rt.tol, f"{label}: scaled S {eS:.3e}, e_a {ee:.3e}, tol {rt.tol:.3e}"


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name,mask", CASES)
def test_one_damping_try_entrywise(name, mask, which_mu):
    """G1 to G4 for one try."""
    rt, sm, mus, fdiag = ref(name, mask)
    nA, mu, cost = rt.nA, mus[which_mu], sm["cost"]
    label = f"{name} {mask} {which_mu}"
    h = handle(rt, groups=False)
    try:
        # the same handle's unfolded buffer first (G2), then the groups on top of the mask
        h.linearize(1.0, 1.0)
        h.schur_assemble(mu)
        M0 = h.get_reduce_buffer().reshape(-1, (nA + 31) // 32 * 32).copy()
        h.set_intrinsics_groups(rt.labels)
        rep, ngroups = h.intrinsics_groups()
        assert np.array_equal(rep, rt.rep) and ngroups == np.unique(rt.rep).size
        assert abs(h.residual() - cost) <= 1e-12 * cost
        h.linearize(1.0, 1.0)
        # ---- G4
        assert abs(h.max_diag() - 1e3 * mus["big"]) <= 1e-11 * 1e3 * mus["big"]
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        # ---- G1
        check_system(rt, sm, fdiag, S, ea, M, *schur_ref(name, mask, mu), mu, 1.0 + mu, label)
        check_padding(M, nA)
        sr.check_mirror(S)
        sr.check_embedded(S, ea, rt.away, 1.0 + mu)
        held = rt.held
        off = S[held].copy()
        off[np.arange(held.size), held] = 0.0
        assert np.all(off == 0.0) and np.all(S[held, held] == 1.0 + mu) and np.all(ea[held] == 0.0)
        # ---- G2
        Fx, Fb, ex, eb, _ = sr.fold_bound(M0, rt.rep, rt.free, mu)
        low = np.tril(np.ones((nA, nA), dtype=bool))
        rS, kS = ar.excess(S[low], Fx[low], Fb[low])
        re, ke = ar.excess(ea, ex, eb)
        print(f"{label}: the fold alone S {rS:.3e}, e_a {re:.3e} of the bound")
        assert rS <= 1.0 and re <= 1.0, f"{label}: fold S {rS:.3e} (lower entry {kS}), e_a {re:.3e} (entry {ke})"
        # ---- G3
        h.schur_reduce()
        h.schur_solve()
        sc = h.backsub(mu)
        assert sc.status == 0
        dp = h.get_dp()
        newcams, newpts = h.get_params(1)
        cams, _ = h.get_params(0)
        dpa = dp[:nA].reshape(-1, CNP)
        assert np.array_equal(dpa[:, :10], dpa[rt.rep][:, :10])
        assert np.array_equal(newcams[:, :10], newcams[rt.rep][:, :10])
        assert np.all(dp[:nA][held] == 0.0)
        cols = np.flatnonzero(~np.asarray(rt.free, dtype=bool))
        assert np.array_equal(newcams[:, cols], cams[:, cols])
        emb = dp[:nA].copy()
        emb[rt.away] = 0.0
        eta, fe, kappa = fr.solve_judge(S, ea, emb)
        print(f"{label}: dp_a eta {eta / ETA_MAX:.3e}, forward {fe / (2 * kappa * 1e-14):.3e} (cond {kappa:.2e})")
        assert eta <= ETA_MAX, f"{label}: backward error {eta:.3e} of the scaled system"
        assert fe <= 2 * kappa * 1e-14, f"{label}: forward error {fe:.3e} (cond {kappa:.2e})"
        r, bound = fr.dpb_residual(rt, sm, dp, mu)
        ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), bound)
        print(f"{label}: dp_b {ratio:.3e}")
        assert ratio <= 1.0, f"{label}: point {k // 3} entry {k % 3}: residual {float(r[k]):.3e} > {bound[k]:.3e}"
        got = dict(dp_l2=sc.dp_l2, gain_den=sc.gain_den, newp_l2=sc.newp_l2, new_cost=sc.new_cost)
        bad = []
        for what, (x, b) in sr.scalars(rt, sm, dp, newcams, newpts, mu).items():
            ratio = float(abs(ar.LD(got[what]) - x) / b)
            print(f"{label}: {what} {ratio:.3e}")
            if not ratio <= 1.0:
                bad.append(f"{what} = {got[what]!r}, exact {float(x)!r}, bound {b:.3e}")
        assert not bad, f"{label}: " + "; ".join(bad)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["tiny", "wide-above"])
def test_begin_and_coefficients(name):
    """G4: psba_begin's maximum; G1 after psba_linearize(2, -2): S / 2 and e_a / -2 are the reference's at mu / 2
    (powers of two: exact) and the placeholder of a folded-away coordinate is 2 + mu."""
    rt, sm, mus, fdiag = ref(name, "bal")
    nA, cost = rt.nA, sm["cost"]
    mu = 2.0 * mus["big"]
    h = handle(rt)
    try:
        c, md = h.begin(1.0, 1.0)
        assert abs(c - cost) <= 1e-12 * cost and abs(md - 1e3 * mus["big"]) <= 1e-11 * 1e3 * mus["big"]
        h.linearize(2.0, -2.0)
        assert abs(h.max_diag() - 2e3 * mus["big"]) <= 1e-11 * 2e3 * mus["big"]
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        check_system(rt, sm, fdiag, S / 2.0, ea / -2.0, M, *schur_ref(name, "bal", mu / 2.0), mu / 2.0, 2.0 + mu,
                     f"{name} (2, -2)")
        check_padding(M, nA)
        sr.check_mirror(S)
        sr.check_embedded(S, ea, rt.away, 2.0 + mu)
        assert np.all(S[rt.held, rt.held] == 2.0 + mu)
        h.schur_solve()
        assert h.backsub(mu).status == 0
        dpa = h.get_dp()[:nA].reshape(-1, CNP)
        assert np.array_equal(dpa[:, :10], dpa[rt.rep][:, :10]) and np.any(dpa[:, 0] != 0.0)
    finally:
        h.close()


def lm_run(rt, labels):
    """(reduce buffer of one assembly, 8-iteration LM log, final cameras) of a fresh handle; labels: 'never' = the
    entry point is not called, None = NULL, else an array"""
    h = handle(rt, groups=False)
    try:
        if not isinstance(labels, str):
            h.set_intrinsics_groups(labels)
        h.linearize(1.0, 1.0)
        h.schur_assemble(1e-3 * h.max_diag())
        buf = h.get_reduce_buffer().tobytes()
        h.reset_params()
        res, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
        return buf, log.tobytes(), h.get_params()[0]
    finally:
        h.close()


def test_no_grouping_is_bit_identical_and_grouped_runs_repeat():
    """G5 on wide_problem(65), BAL mask."""
    rt = ref("wide-above", "bal")[0]
    never = lm_run(rt, "never")
    for labels in (None, np.arange(rt.nC)[::-1].copy()):
        got = lm_run(rt, labels)
        assert got[0] == never[0] and got[1] == never[1] and len(got[1]) > 0
    a, b = lm_run(rt, rt.labels), lm_run(rt, rt.labels)
    assert a[0] == b[0] and a[1] == b[1] and len(a[1]) > 0 and np.array_equal(a[2], b[2])
    assert a[0] != never[0]
    assert np.array_equal(a[2][:, :10], a[2][rt.rep][:, :10])


@functools.lru_cache(maxsize=None)
def twin_levmar(which):
    p = P7()
    return sr.SharedTwin(p, P7_LABELS[which], start_kc(p["nC"]), BAL).levmar_shared(max_iter=8)


@pytest.mark.parametrize("which", list(P7_LABELS))
def test_levmar_against_the_shared_twin(which):
    """G6: the tolerances of test_gpu_freekd.py::test_levmar_against_the_twin."""
    rt = ref("P7-" + which, "bal")[0]
    want, wlog = twin_levmar(which)
    h = handle(rt)
    try:
        res, log = h.levmar(max_iter=8, tr_handoff=False, log_cap=256)
        assert abs(res.init_err - want.init_err) <= 1e-12 * want.init_err
        n = min(len(log), len(wlog), 6)
        assert n >= 4
        np.testing.assert_allclose(log[:n, 1], wlog[:n, 1], rtol=1e-6)
        assert np.array_equal(log[:n, 4], wlog[:n, 4])
        assert abs(res.final_err - want.final_err) <= 1e-5 * want.final_err
        # the stop tests agree (the twin numbers its flags 0 none, 1 dp no change, 2 error, 3 cost small enough)
        assert res.iters == want.iters and res.flag == TWIN_FLAG[want.flag]
        cams, _ = h.get_params()
        assert np.array_equal(cams[:, :10], cams[rt.rep][:, :10])
        held = [k for k in range(10) if not BAL[k]]
        assert np.array_equal(cams[:, held], np.hstack([np.asarray(rt.p["K"]).reshape(-1, 5), rt.kc])[:, held])
        assert np.abs(cams[:, 0] - np.asarray(rt.p["K"]).reshape(-1, 5)[:, 0]).max() > 0
    finally:
        h.close()


def test_recovery_of_the_shared_ring_scene():
    """G7: true K and kc shared by {0, 2, 4} and {1, 3, 5}, start at fu x 1.03 and kc = 0, no absolute stop; the
    thresholds of test_gpu_freekd.py::test_recovery_of_the_ring_scene (the host twin keeps 25x under each:
    test_shared_ref.py)."""
    import psba_amd
    lab = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    start, kc0, K_true, kc_true = sr.shared_ring(lab)
    h = psba_amd.Psba(0)
    try:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        h.upload_problem(start)
        h.set_distortion(kc0)
        h.set_intrinsics_mask(BAL)
        h.set_intrinsics_groups(lab)
        res, log = h.levmar(max_iter=30, tr_handoff=False, log_cap=256, stop_cost=-1.0)
        cams, _ = h.get_params()
    finally:
        h.close()
    f = np.abs(cams[:, 0] / K_true[:, 0] - 1).max()
    k1 = np.abs(cams[:, 5] - kc_true[:, 0]).max()
    k2 = np.abs(cams[:, 6] - kc_true[:, 1]).max()
    print(f"iterations {res.iters} flag {res.flag}: cost {res.final_err:.3e} of {res.init_err:.3e}, f {f:.2e}, "
          f"k1 {k1:.2e}, k2 {k2:.2e}")
    assert res.final_err <= 1e-15 * res.init_err
    assert f <= 1e-9 and k1 <= 1e-8 and k2 <= 1e-7
    rep = sr.representatives(lab)
    assert np.array_equal(cams[:, :10], cams[rep][:, :10])


def test_interface():
    """G8."""
    import psba_amd
    rt = ref("P7-two", "bal")[0]
    p, lab, nC = rt.p, rt.labels, rt.nC

    def refused(call, code, *words):
        with pytest.raises(psba_amd.PsbaError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), str(ei.value)

    # wrong model, before upload
    for model in (psba_amd.CAMERA_FIXED_K, psba_amd.CAMERA_FREE_K):
        ho = psba_amd.Psba(0)
        ho.set_camera_model(model)
        ho.upload_problem(p)
        refused(lambda: ho.set_intrinsics_groups(lab), -6, "PSBA_CAMERA_FREE_KD")
        refused(lambda: ho.intrinsics_groups(), -6, "PSBA_CAMERA_FREE_KD")
        ho.close()
    h = psba_amd.Psba(0)
    h.set_camera_model(psba_amd.CAMERA_FREE_KD)
    refused(lambda: h.set_intrinsics_groups(None), -6, "no problem uploaded")
    h.upload_problem(p)
    h.set_distortion(rt.kc)
    # the getter round-trips; labels are any ints; NULL and all-alone are no grouping
    assert np.array_equal(h.intrinsics_groups()[0], np.arange(nC)) and h.intrinsics_groups()[1] == nC
    h.set_intrinsics_groups(lab * -1000 + 7)
    rep, n = h.intrinsics_groups()
    assert np.array_equal(rep, rt.rep) and n == 2
    h.set_intrinsics_groups(None)
    assert h.intrinsics_groups()[1] == nC
    h.set_intrinsics_groups(lab)
    h.set_intrinsics_groups(np.arange(nC) + 5)
    assert np.array_equal(h.intrinsics_groups()[0], np.arange(nC)) and h.intrinsics_groups()[1] == nC
    # mask and groups compose in both orders: the same system
    bufs = []
    for order in ("mask first", "groups first"):
        h.set_intrinsics_mask(None)
        h.set_intrinsics_groups(None)
        for what in (("mask", "groups") if order == "mask first" else ("groups", "mask")):
            h.set_intrinsics_mask(BAL) if what == "mask" else h.set_intrinsics_groups(lab)
        assert h.intrinsics_mask() == BAL and h.intrinsics_groups()[1] == 2
        h.linearize(1.0, 1.0)
        h.schur_assemble(1e-3 * h.max_diag())
        bufs.append(h.get_reduce_buffer().tobytes())
    assert bufs[0] == bufs[1]
    # members that differ: the message names the camera and the column; nothing changes
    h.set_intrinsics_groups(None)
    cams, pts = h.get_params()
    split = cams.copy()
    split[4, 6] += 1e-9
    h.set_params(split, pts)
    refused(lambda: h.set_intrinsics_groups(lab), -1, "camera 4", "column 6")
    assert h.intrinsics_groups()[1] == nC
    h.set_params(cams, pts)
    h.set_intrinsics_groups(lab)
    # ... also a difference in the copy psba_reset_params restores (here: a K that is not shared)
    hk = psba_amd.Psba(0)
    hk.set_camera_model(psba_amd.CAMERA_FREE_KD)
    Ks = np.asarray(p["K"], dtype=np.float64).reshape(-1, 5).copy()
    Ks[2, 0] *= 1.01
    hk.upload_problem(dict(p, K=Ks))
    refused(lambda: hk.set_intrinsics_groups(lab), -1, "camera 2", "column 0")
    c7, p7 = hk.get_params()
    c7[:, :10] = c7[rt.rep][:, :10]
    hk.set_params(c7, p7)
    refused(lambda: hk.set_intrinsics_groups(lab), -1, "psba_reset_params", "camera 2")
    assert hk.intrinsics_groups()[1] == nC
    hk.close()
    # set_params / set_distortion that would split a group: refused before the device is touched
    refused(lambda: h.set_params(split, pts), -1, "psba_set_params", "camera 4", "column 6")
    assert np.array_equal(h.get_params()[0], cams)
    kc_split = rt.kc.copy()
    kc_split[5, 2] = 1e-3
    refused(lambda: h.set_distortion(kc_split), -1, "psba_set_distortion", "camera 5", "column 7")
    assert np.array_equal(h.get_params()[0], cams) and h.intrinsics_groups()[1] == 2
    h.set_distortion(rt.kc)
    h.set_params(cams, pts)
    # refused while a try is in flight, and then nothing changes
    h.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h.schur_solve()
    h.backsub_async(mu)
    refused(lambda: h.set_intrinsics_groups(None), -6, "in flight")
    h.backsub_wait()
    assert np.array_equal(h.intrinsics_groups()[0], rt.rep)
    # a new upload resets the groups
    h.upload_problem(p)
    assert h.intrinsics_groups()[1] == nC and np.array_equal(h.intrinsics_groups()[0], np.arange(nC))
    h.close()


# ---- groups under Marquardt's damping (psba_set_damping) ---------------------------------------------------
MQ_RULE = fr.Rule(fr.MARQUARDT)
MQ_MUS = {"big": 1e-3, "small": 1e-6}   # Marquardt's mu is relative (test_gpu_damping.py)
WORST_MQ = {}


@pytest.fixture(scope="module", autouse=True)
def _report_marquardt():
    yield
    if WORST_MQ:
        print("\ngroups under Marquardt, worst ratio found / allowed per input and quantity:")
        for name in sorted({n for n, _ in WORST_MQ}):
            print(f"  {name}: " + ", ".join(f"{q} {v:.2e}" for (n, q), v in WORST_MQ.items() if n == name))


def note_mq(name, what, ratio):
    WORST_MQ[(name, what)] = max(WORST_MQ.get((name, what), 0.0), float(ratio))
    print(f"{name} marquardt {what}: {float(ratio):.3e}")


@functools.lru_cache(maxsize=None)
def schur_ref_marquardt(name, mask, mu):
    rt, sm, _, _ = ref(name, mask)
    S, ea = sr.schur_ref(rt, sm, mu, MQ_RULE)
    S.setflags(write=False)
    ea.setflags(write=False)
    return S, ea


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name", ["wide-above", "one-group"])
def test_one_damping_try_entrywise_marquardt(name, which_mu):
    """G1, G3 under PSBA_DAMPING_MARQUARDT, BAL mask: wide_labels on 65 cameras and all 65 cameras one group (a member
    sum of 65 terms in k_free_damp_diag).  D of the embedded system is the clamp of the members' sum at a
    representative's shared coordinate and clamp(coeff) at a folded-away one; mu D is added once, after the fold;
    gain_den counts a shared parameter once (shared_ref.scalars with the device's D)."""
    import psba_amd
    rt, sm, mus, fdiag = ref(name, "bal")
    nA, mu, cost = rt.nA, MQ_MUS[which_mu], sm["cost"]
    label = f"{name} bal {which_mu} marquardt"
    h = handle(rt)
    try:
        h.set_damping(psba_amd.DAMPING_MARQUARDT, MQ_RULE.dmin, MQ_RULE.dmax)
        assert h.damping() == tuple(MQ_RULE) and h.intrinsics_groups()[1] == np.unique(rt.rep).size
        h.linearize(1.0, 1.0)
        assert abs(h.max_diag() - 1e3 * mus["big"]) <= 1e-11 * 1e3 * mus["big"]
        # ---- D of the embedded system
        D = h.get_damping_diag()
        x, env, fixed = sr.folded_damp_diag(rt, sm)
        ratio, k, nlow, nhigh = fr.check_damp_diag(D, x, env, MQ_RULE, fixed)
        note_mq(name, "D", ratio)
        assert ratio <= 1.0, f"{label}: D[{k}] = {D[k]!r} outside its envelope"
        assert nlow >= 3 and np.all(D[np.flatnonzero(rt.away)] == 1.0)
        # ---- G1
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        D_ref = sr.damp_ref(rt, sm, MQ_RULE)[0]
        d = np.sqrt(fdiag[:nA] + mu * D_ref[:nA])
        eS, ee = sr.scaled_errors(S, ea, *schur_ref_marquardt(name, "bal", mu), d, cost)
        note_mq(name, "S", eS / rt.tol)
        note_mq(name, "e_a", ee / rt.tol)
        assert eS <= rt.tol and ee <= rt.tol, f"{label}: scaled S {eS:.3e}, e_a {ee:.3e}, tol {rt.tol:.3e}"
        check_padding(M, nA)
        sr.check_mirror(S)
        sr.check_embedded(S, ea, rt.away, 1.0 + mu)
        held = rt.held
        off = S[held].copy()
        off[np.arange(held.size), held] = 0.0
        assert np.all(off == 0.0) and np.all(S[held, held] == 1.0 + mu) and np.all(ea[held] == 0.0)
        # ---- G3
        h.schur_reduce()
        h.schur_solve()
        sc = h.backsub(mu)
        assert sc.status == 0
        dp = h.get_dp()
        newcams, newpts = h.get_params(1)
        dpa = dp[:nA].reshape(-1, CNP)
        assert np.array_equal(dpa[:, :10], dpa[rt.rep][:, :10])
        assert np.array_equal(newcams[:, :10], newcams[rt.rep][:, :10])
        assert np.all(dp[:nA][held] == 0.0)
        emb = dp[:nA].copy()
        emb[rt.away] = 0.0
        eta, fe, kappa = fr.solve_judge(S, ea, emb)
        note_mq(name, "dp_a eta", eta / ETA_MAX)
        note_mq(name, "dp_a forward", fe / (2 * kappa * 1e-14))
        assert eta <= ETA_MAX, f"{label}: backward error {eta:.3e} of the scaled system"
        assert fe <= 2 * kappa * 1e-14, f"{label}: forward error {fe:.3e} (cond {kappa:.2e})"
        r, bound = fr.dpb_residual(rt, sm, dp, mu, MQ_RULE)
        ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), bound)
        note_mq(name, "dp_b", ratio)
        assert ratio <= 1.0, f"{label}: point {k // 3} entry {k % 3}: residual {float(r[k]):.3e} > {bound[k]:.3e}"
        assert np.all(dp[nA + 3 * (rt.nP - 1):] == 0.0)      # the point without observations
        got = dict(dp_l2=sc.dp_l2, gain_den=sc.gain_den, newp_l2=sc.newp_l2, new_cost=sc.new_cost)
        bad = []
        for what, (x, b) in sr.scalars(rt, sm, dp, newcams, newpts, mu, D=D).items():
            ratio = float(abs(ar.LD(got[what]) - x) / b)
            note_mq(name, what, ratio)
            if not ratio <= 1.0:
                bad.append(f"{what} = {got[what]!r}, exact {float(x)!r}, bound {b:.3e}")
        assert not bad, f"{label}: " + "; ".join(bad)
    finally:
        h.close()
