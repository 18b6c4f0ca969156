"""The per-observation camera model of camera_model.h entry by entry on every route that evaluates it, against the exact
values and the derived per-entry bounds of tests/camera_ref.py.  Needs an MI355X.

One problem per input family (camera_ref.family: 9 cameras, 111 points, 333 observations, camera 0 holds 65); every
output the ABI exposes per observation must satisfy |got - exact| <= that entry's own bound:
  * k_residual   psba_compute_exQT and psba_obs_sq_residuals at PARAMS_CUR, and at PARAMS_NEW after psba_set_step
                 (the proposal is read back with psba_get_params: the kernel's own inputs);
  * dump         psba_compute_jacobiQT (A, B of the dumping K1), psba_compute_Wblks against exact c A^T B
                 (camera_ref.w_bound);
  * k_jmul       psba_compute_Jmultiply with the nine unit directions: the result is column k of that kernel's own A
                 or B exactly (every other term is an exact zero), judged like the dumped blocks;
  * fused K1     a single-observation problem (observation a joins camera a to point a, so every K1 sum has one
                 term): psba_linearize, psba_get_gradient = c_g J^T e of the non-dumping instantiation, at 200 cameras
                 (camera sums in LDS) and at 333 (the camera-major pass k_cam_sums), on benign, far and dist;
  * free         psba_get_free_obs_blocks after psba_linearize with camera blocks of 11 and 16: B, e and
                 W = c A^T B as k_free_linearize stored them (every column of A enters W, the 1.0 and 0.0 constants
                 with a zero bound of their own; a masked intrinsic's rows are zero).
Exact structure: A[9] = 0.0 without distortion, fixed blocks 0.0 in A or B (not -0.0) while e is judged as ever.
Slack checks as the entrywise suites assume them (tests/assembly_ref.py; no new number): on 54cams, trafalgar21 and the
lens problem |A_jmul - A_dump| <= JACOBIAN_SLACK |A| and the same for B, per entry.  (This is the check that found the
kernels' only fault: with the compiler free to contract across statements the two instantiations differed by
2.7 JACOBIAN_SLACK |A| in entry 11 of observation 22413 of 54cams, (v0 - y) / Pz where y cancels v0.  camera_model.h
now pins the contraction, PSBA_FP_PINNED, and the blocks agree bit for bit, which is asserted too.)  The residual the dumping K1
forms (dbg_ex) is exposed by no verb -- psba_compute_exQT runs k_residual -- so |e(k_residual) - e(K1)| against
assembly_ref.residual_slack cannot be read off; the single-observation gradient judges K1's e through c_g J^T e.
The module prints the worst found / allowed ratio per route, family and quantity; DESIGN 7f keeps the table."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import camera_ref as cr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not cr.LD_OK, reason="needs an 80-bit long double")]

W_COEFF, G_COEFF = 0.7, -1.3  # not powers of two: the scalings round
FREE = {"fk-far": ("far", 11, cr.KD_ALL_FREE), "fk-rot": ("rot", 11, cr.KD_ALL_FREE),
        "kd-dist": ("dist", 16, cr.KD_ALL_FREE), "kd-dist-bal": ("dist", 16, cr.BAL_MASK),
        "kd-rot-kc0": ("rot", 16, cr.KD_ALL_FREE)}
WORST = {}  # (route, family, quantity) -> worst found / allowed


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        keys = list(dict.fromkeys((r, f) for r, f, _ in WORST))
        lines = [f"  {r} {f}: " + ", ".join(f"{q} {v:.3f}" for (rr, ff, q), v in WORST.items() if (rr, ff) == (r, f))
                 for r, f in keys]
        print("\nworst ratio found / allowed per route, family and quantity:\n" + "\n".join(lines))


def judge(route, fam, what, got, exact, bound):
    got = np.asarray(got).reshape(np.shape(exact))
    r, k = ar.excess(got, exact, bound)
    WORST[(route, fam, what)] = max(WORST.get((route, fam, what), 0.0), r)
    if not r <= 1.0:
        g, x = got.reshape(-1)[k], float(np.asarray(exact).reshape(-1)[k])
        raise AssertionError(f"{route} {fam} {what}: entry {k} = {g!r}, exact {x!r}, |diff| {abs(g - x):.3e} > bound "
                             f"{float(np.asarray(bound).reshape(-1)[k]):.3e} (ratio {r:.3e})")


def reference(case, cnp=6, mask=cr.KD_ALL_FREE, cams=None, pts=None):
    """exact values and bounds of one case: e, A, B (linearization), er, s (k_residual); each (exact, bound)"""
    kw = dict(cnp=cnp, free_mask=mask, cams=cams, pts=pts)
    eE, AE, BE = cr.linearize(cr.gather(case, "E", **kw))
    ex, Ax, Bx, sx = cr.exact(cr.gather(case, "raw", **kw))
    out = dict(e=(ex, cr.stack(eE)[1]), A=(Ax, cr.stack(AE)[1]), B=(Bx, cr.stack(BE)[1]))
    if cnp == 6:
        rE, sE = cr.residual(cr.gather(case, "E", **kw))
        out["er"] = (ex, cr.stack(rE)[1])
        out["s"] = (sx[:, None], cr.stack([sE])[1])
    return out


@functools.lru_cache(maxsize=None)
def family_reference(fam, cnp=6, mask=cr.KD_ALL_FREE):
    return reference(cr.family(fam), cnp, mask)


def handle(case, cnp=6, mask=cr.KD_ALL_FREE):
    import psba_amd
    prob = case["prob"]
    h = psba_amd.Psba(0)
    if cnp != 6:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD if cnp == 16 else psba_amd.CAMERA_FREE_K)
    h.upload_problem(prob)
    assert h.camera_block() == cnp
    if cnp == 16:
        h.set_distortion(case.get("kc"))
        h.set_intrinsics_mask([(mask >> k) & 1 for k in range(10)])
    if cnp == 6:
        if case.get("kc") is not None:
            h.set_distortion(case["kc"])
        if case.get("cov") is not None:
            h.set_obs_covariance(case["cov"])
        if case.get("loss") is not None:
            h.set_robust_loss(*case["loss"])
        if case.get("fixed_cams") is not None or case.get("fixed_pts") is not None:
            h.set_fixed(case.get("fixed_cams"), case.get("fixed_pts"))
    return h


def _step(case, rng):
    """a step that keeps every point in front of its cameras and |v| below 1"""
    prob = case["prob"]
    x = cr.gather(case, "f64")
    depth = cr._pose(x["q0"], x["cam"], x["M"])[3][2].min()
    cams = np.asarray(prob["cams"], dtype=np.float64)
    dc = np.concatenate([-1e-3 * cams[:, :3] - 1e-4 * rng.random((cams.shape[0], 3)) * np.sign(cams[:, :3]),
                         1e-2 * depth * rng.uniform(-1, 1, (cams.shape[0], 3))], axis=1)
    dp = 1e-2 * depth * rng.uniform(-1, 1, (int(prob["nP"]), 3))
    return np.concatenate([dc.reshape(-1), dp.reshape(-1)])


def _exact_zeros(route, fam, what, block, rows):
    """the entries a contract sets to 0.0 are +0.0"""
    z = np.asarray(block)[rows]
    assert not np.any(z) and not np.any(np.signbit(z)), f"{route} {fam}: {what} is not +0.0 everywhere"


@pytest.mark.parametrize("fam", cr.FAMILIES)
def test_fixed_intrinsics_routes(fam):
    from psba_amd import capi
    case = cr.family(fam)
    ref = family_reference(fam)
    prob = case["prob"]
    nC, nP, nO = int(prob["nC"]), int(prob["nP"]), int(prob["nO"])
    i, j = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    fc = None if case["fixed_cams"] is None else (np.asarray(case["fixed_cams"]) != 0)[j]
    fp = None if case["fixed_pts"] is None else (np.asarray(case["fixed_pts"]) != 0)[i]
    h = handle(case)
    try:
        # ---- k_residual at the current parameters
        judge("k_residual", fam, "e", h.compute_exQT(capi.PARAMS_CUR), *ref["er"])
        judge("k_residual", fam, "s", h.obs_sq_residuals(capi.PARAMS_CUR), *ref["s"])
        # ---- the dumping K1
        JA, JB = h.compute_jacobiQT()
        JA, JB = JA.reshape(nO, 12), JB.reshape(nO, 6)
        judge("dump", fam, "A", JA, *ref["A"])
        judge("dump", fam, "B", JB, *ref["B"])
        if case["kc"] is None:
            _exact_zeros("dump", fam, "A[9]", JA[:, 9], slice(None))
        if fc is not None:
            _exact_zeros("dump", fam, "A of a fixed camera", JA, fc)
            _exact_zeros("dump", fam, "B of a fixed point", JB, fp)
            assert np.any(JA[~fc]) and np.any(JB[~fp])
        W = h.compute_Wblks(W_COEFF)
        judge("dump", fam, "W", W, *cr.w_bound(ref["A"][0], ref["A"][1], ref["B"][0], ref["B"][1], W_COEFF, 6))
        if fc is not None:
            assert not np.any(W.reshape(nO, 18)[fc | fp])
        # ---- k_jmul: unit directions
        A_j, B_j = np.empty((nO, 12)), np.empty((nO, 6))
        for k in range(6):
            x = np.zeros(6 * nC + 3 * nP)
            x[k:6 * nC:6] = 1.0
            A_j[:, [k, 6 + k]] = h.compute_Jmultiply(x).reshape(nO, 2)
        for k in range(3):
            x = np.zeros(6 * nC + 3 * nP)
            x[6 * nC + k::3] = 1.0
            B_j[:, [k, 3 + k]] = h.compute_Jmultiply(x).reshape(nO, 2)
        judge("k_jmul", fam, "A", A_j, *ref["A"])
        judge("k_jmul", fam, "B", B_j, *ref["B"])
        if case["kc"] is None:
            _exact_zeros("k_jmul", fam, "A[9]", A_j[:, 9], slice(None))
        if fc is not None:
            _exact_zeros("k_jmul", fam, "A of a fixed camera", A_j, fc)
            _exact_zeros("k_jmul", fam, "B of a fixed point", B_j, fp)
        # ---- k_residual at a proposal
        h.set_step(_step(case, np.random.default_rng(5)))
        cams, pts = h.get_params(capi.PARAMS_NEW)
        assert not np.array_equal(cams, prob["cams"]) and not np.array_equal(pts, prob["pts"])
        new = reference(case, cams=cams, pts=pts)
        judge("k_residual", fam, "e (proposal)", h.compute_exQT(capi.PARAMS_NEW), *new["er"])
        judge("k_residual", fam, "s (proposal)", h.obs_sq_residuals(capi.PARAMS_NEW), *new["s"])
        # (the current parameters are untouched)
        judge("k_residual", fam, "e", h.compute_exQT(capi.PARAMS_CUR), *ref["er"])
    finally:
        h.close()


@pytest.mark.parametrize("n", [200, 333], ids=["lds-sums", "camera-major"])
@pytest.mark.parametrize("fam", ["benign", "far", "dist"])
def test_fused_k1_single_observation(fam, n):
    case = cr.single_observation(cr.family(fam), n)
    ref = reference(case)
    (ex, be), (Ax, bA), (Bx, bB) = ref["e"], ref["A"], ref["B"]
    h = handle(case)
    try:
        h.linearize(W_COEFF, G_COEFF)
        g = h.get_gradient()
    finally:
        h.close()
    # g_a,a = c_g A_a^T e_a, g_b,a = c_g B_a^T e_a: one term per sum
    ga, bga = cr.gradient_bound(Ax, bA, ex, be, G_COEFF, 6)
    gb, bgb = cr.gradient_bound(Bx, bB, ex, be, G_COEFF, 3)
    route = "fused K1 (camera-major)" if n > 222 else "fused K1"
    judge(route, fam, "g_a", g[:6 * n], ga, bga)
    judge(route, fam, "g_b", g[6 * n:], gb, bgb)


@pytest.mark.parametrize("name", list(FREE))
def test_free_intrinsics_blocks(name):
    fam, cnp, mask = FREE[name]
    case = cr.family(fam)
    ref = family_reference(fam, cnp, mask)
    nO = int(case["prob"]["nO"])
    h = handle(case, cnp, mask)
    try:
        assert h.schur_path() == 5
        h.linearize(W_COEFF, 1.0)
        W, B, e = h.free_obs_blocks()
    finally:
        h.close()
    judge("free", name, "e", e, *ref["e"])
    judge("free", name, "B", B.reshape(nO, 6), *ref["B"])
    judge("free", name, "W", W, *cr.w_bound(ref["A"][0], ref["A"][1], ref["B"][0], ref["B"][1], W_COEFF, cnp))
    held = [k for k in range(10 if cnp == 16 else 0) if not (mask >> k) & 1]
    assert not np.any(W[:, held, :]) and (cnp != 16 or mask == cr.KD_ALL_FREE or len(held) == 7)
    assert np.all(np.any(W[:, [k for k in range(cnp) if k not in held], :] != 0, axis=(0, 2)))


def test_free_obs_blocks_refusals():
    import psba_amd
    from psba_amd import capi
    case = cr.family("benign")

    def refused(hh, word=None):
        with pytest.raises(capi.PsbaError) as ei:
            hh.free_obs_blocks()
        assert ei.value.code == -6
        assert word is None or word in str(ei.value)

    h = psba_amd.Psba(0)
    try:
        with pytest.raises(capi.PsbaError) as ei:  # nothing uploaded
            h._ck(capi.lib.psba_get_free_obs_blocks(h._h, None, None))
        assert ei.value.code == -6
        h.upload_problem(case["prob"])
        refused(h, "free-intrinsics")  # six-parameter blocks
        h.linearize(1.0, 1.0)
        refused(h, "free-intrinsics")
    finally:
        h.close()
    h = handle(case, 11)
    try:
        refused(h, "psba_linearize first")
        h.linearize(1.0, 1.0)
        W0, B0, e0 = h.free_obs_blocks()
        assert capi.lib.psba_get_free_obs_blocks(h._h, None, None) == 0  # null pointers: nothing copied
        cams, pts = h.get_params()
        h.set_params(cams, pts)
        refused(h, "psba_linearize first")
        h.linearize(1.0, 1.0)
        W1, B1, e1 = h.free_obs_blocks()
        assert np.array_equal(W0, W1) and np.array_equal(B0, B1) and np.array_equal(e0, e1)
        # one try; the linearization queued ahead reuses the B | e buffer
        mu = 1e-3 * h.max_diag()
        h.schur_assemble(mu)
        h.schur_reduce()
        assert h.schur_solve() == capi.PSBA_OK
        assert h.backsub(mu).status == 0
        assert np.array_equal(h.free_obs_blocks()[0], W0)  # the try reads W, it does not write it
        h.linearize_ahead()
        refused(h, "psba_linearize first")
        newc, newp = h.get_params(capi.PARAMS_NEW)
        h.accept()
        refused(h, "psba_linearize first")  # (not linearized as far as the caller knows)
        h.linearize(1.0, 1.0)  # nothing left to do: the blocks queued ahead are the current ones
        W2, B2, e2 = h.free_obs_blocks()
        assert not np.array_equal(W2, W0)
        h.set_params(newc, newp)
        h.linearize(1.0, 1.0)
        W3, B3, e3 = h.free_obs_blocks()
        assert np.array_equal(W2, W3) and np.array_equal(B2, B3) and np.array_equal(e2, e3)
        h.reset_params()
        refused(h, "psba_linearize first")
    finally:
        h.close()
    h = handle(cr.family("dist"), 16)
    try:
        h.linearize(1.0, 1.0)
        h.free_obs_blocks()
        h.set_intrinsics_mask(list(capi.INTRINSICS_BAL))
        refused(h, "psba_linearize first")
        h.linearize(1.0, 1.0)
        h.free_obs_blocks()
        h.set_distortion(None)
        refused(h, "psba_linearize first")
    finally:
        h.close()


def _lens_handle(prob, lens):
    import psba_amd
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    if lens is not None:
        kc, cov, c = lens
        h.set_distortion(kc)
        h.set_obs_covariance(cov)
        h.set_robust_loss(cr.LOSS_HUBER, c)
    return h


@pytest.mark.parametrize("name", ["54cams", "trafalgar21", "lens54"])
def test_jacobian_slack_between_instantiations(name, problems):
    """JACOBIAN_SLACK as tests/assembly_ref.py and tests/tr_ref.py assume it: k_jmul's blocks against the dumped ones"""
    lens = None
    if name == "lens54":
        from test_gpu_robust import _one_try_case
        prob, kc, cov = _one_try_case("default")
        lens = (kc, cov, 2.0)
    else:
        prob = problems[name]
    nC, nP, nO = int(prob["nC"]), int(prob["nP"]), int(prob["nO"])
    h = _lens_handle(prob, lens)
    try:
        JA, JB = h.compute_jacobiQT()
        JA, JB = JA.reshape(nO, 12), JB.reshape(nO, 6)
        A_j, B_j = np.empty((nO, 12)), np.empty((nO, 6))
        for k in range(6):
            x = np.zeros(6 * nC + 3 * nP)
            x[k:6 * nC:6] = 1.0
            A_j[:, [k, 6 + k]] = h.compute_Jmultiply(x).reshape(nO, 2)
        for k in range(3):
            x = np.zeros(6 * nC + 3 * nP)
            x[6 * nC + k::3] = 1.0
            B_j[:, [k, 3 + k]] = h.compute_Jmultiply(x).reshape(nO, 2)
    finally:
        h.close()
    judge("slack k_jmul / dump", name, "A", A_j, JA.astype(ar.LD), ar.JACOBIAN_SLACK * np.abs(JA))
    judge("slack k_jmul / dump", name, "B", B_j, JB.astype(ar.LD), ar.JACOBIAN_SLACK * np.abs(JB))
    # camera_model.h pins the contraction of the model's text (PSBA_FP_PINNED): the two kernels get the same bits
    assert np.array_equal(A_j, JA) and np.array_equal(B_j, JB), f"{name}: k_jmul's blocks are not the dumped ones"
