"""K1 (U, V, W, g), K2 (V*^-1, Y, S, e_a) and K3 (e_b, dp_b, the try scalars) entry by entry against the
extended-precision reference of tests/assembly_ref.py, on every route of the assembly.  Needs an MI355X.

Each case uploads one problem to one handle (two for `ranks`) and runs two layers:
  * mirror: every sba_func.h verb judged from the GPU's own dumped inputs -- U, V, W, g against sums of the dumped
    A, B and e (K1 sums linearize_obs's residual, the readable one is residual_obs's: RESIDUAL_SLACK; with the
    camera-major pass U and g_a are summed from blocks k_cam_sums recomputes: JACOBIAN_SLACK), U* and V* against
    U + mu, V + mu, V*^-1 against the exact inverse of the GPU's V*, Y, S and e_a against the reference built from
    the GPU's U*, W, V*, g, e_b and dp_b from the GPU's dpa (and e_b).
  * fused: psba_linearize, psba_schur_assemble(mu), the reduce buffer (or the block-sparse S), psba_schur_reduce,
    psba_schur_solve, psba_backsub(mu), psba_get_dp: S (the lower triangle, the one every route writes and the
    Cholesky reads), e_a, dp_b and the four try scalars against the same reference built from the dumped A, B, e,
    with the K1 accumulation envelope and JACOBIAN_SLACK carried through (the fused instantiations' U, V, W, g are
    not readable).  `ranks`: two point shards with a rank layout and the packed route, their packed sums added on
    the host (r = 2).
Every entry must satisfy |got - exact| <= its own bound; the module prints the worst bound ratio per route and quantity.

Cases with a `fixed=` option run the same two layers under psba_set_fixed (the LENS_FIXED instantiations, k_fixed_diag,
k_max_diag_fixed): the mask is computed from the problem (tests/fixed_ref.py: mixed, island, long) and printed, the
reference has the placeholder rule installed (exact values, zero envelopes), and the exact parts -- zeros, placeholders,
the rows and columns of fixed cameras in S, the bits of fixed blocks in the proposal, camera 0's zero rotation
coordinates set to -0.0 first -- are compared with no tolerance, on bit patterns where a sign could hide."""
import contextlib

import numpy as np
import pytest

import assembly_ref as ar
import fixed_ref as fr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

CAM_ACC = 27  # K1's sums per camera: the upper triangle of U_j and g_a,j (psba_internal.h)
CAM_LDS_MAX = 48 * 1024  # bytes of them K1 keeps in LDS; beyond, the camera-major pass (psba_api.cpp)
EA_SLOT = [1, 2, 3, 4, 5, 8]  # the upper slots of a packed diagonal block that carry e_a (schur_common.h)
LOSS_HUBER = 1

# id -> (problem, environment, options); path: psba_schur_path of the fused route (0 LDS partitions, 1 owner,
# 2 global atomics, 4 block-sparse); plan: what capi.schur_plan must show for the route
CASES = {
    "rows-54cams": ("54cams", {}, dict(path=0)),
    "rows-trafalgar21": ("trafalgar21", {}, dict(path=0)),
    "runs": ("venice16", {}, dict(path=0, plan="runs")),
    "runs-forced": ("venice1", {"PSBA_SCHUR_RUNS": "1"}, dict(path=0, plan="runs")),
    "block-ranges": ("54cams", {"PSBA_SCHUR_BLOCK_GROUPS": "1", "PSBA_SCHUR_SPLIT": "3"},
                     dict(path=0, plan="split3")),
    "sep-diag": ("54cams", {"PSBA_CHOL_SEPARATE_DIAG": "1"}, dict(path=0)),
    "owner": ("trafalgar21", {"PSBA_SCHUR_OWNER": "1"}, dict(path=1, mirror_label="owner (mirror: atomic)")),
    "atomic": ("54cams", {"PSBA_SCHUR_ATOMIC": "1"}, dict(path=2)),
    "long": ("long", {}, dict(path=1, mirror_label="long (mirror: atomic)")),
    "cam-major": ("54cams", {"PSBA_LIN_GLOBAL_ACC": "1"}, dict(path=0)),
    "v1": ("54cams", {"PSBA_LIN_V1": "1"}, dict(path=0)),
    "read-w": ("54cams", {"PSBA_BACK_READ_W": "1"}, dict(path=0, read_w=True)),
    "sparse": ("sparse60", {}, dict(path=4, solver=1)),
    "ranks": ("54cams", {"PSBA_SCHUR_PACKED": "1"}, dict(path=0, ranks=2)),
    "lens-robust": ("lens54", {}, dict(path=0, lens=True)),
    "lens-robust-owner": ("lens54", {"PSBA_SCHUR_OWNER": "1"},
                          dict(path=1, lens=True, mirror_label="lens-robust-owner (mirror: atomic)")),
    "tr-coeff": ("7cams", {}, dict(path=0, coeff=(2.0, -2.0))),
    # ---- fixed blocks (psba_set_fixed): the module's small shapes under the masks of tests/fixed_ref.py ----
    "fixed-rows-mixed": ("54cams", {}, dict(path=0, fixed="mixed")),
    "fixed-rows-island": ("54cams", {}, dict(path=0, fixed="island")),
    "fixed-owner-mixed": ("54cams", {"PSBA_SCHUR_OWNER": "1"},
                          dict(path=1, fixed="mixed", mirror_label="fixed-owner-mixed (mirror: atomic)")),
    "fixed-owner-island": ("54cams", {"PSBA_SCHUR_OWNER": "1"},
                           dict(path=1, fixed="island", mirror_label="fixed-owner-island (mirror: atomic)")),
    "fixed-atomic-mixed": ("54cams", {"PSBA_SCHUR_ATOMIC": "1"}, dict(path=2, fixed="mixed")),
    "fixed-atomic-island": ("54cams", {"PSBA_SCHUR_ATOMIC": "1"}, dict(path=2, fixed="island")),
    "fixed-read-w-mixed": ("54cams", {"PSBA_BACK_READ_W": "1"}, dict(path=0, read_w=True, fixed="mixed")),
    "fixed-read-w-island": ("54cams", {"PSBA_BACK_READ_W": "1"}, dict(path=0, read_w=True, fixed="island")),
    "fixed-sparse-mixed": ("sparse60", {}, dict(path=4, solver=1, fixed="mixed")),
    "fixed-sparse-island": ("sparse60", {}, dict(path=4, solver=1, fixed="island")),
    "fixed-runs-forced-mixed": ("venice1", {"PSBA_SCHUR_RUNS": "1"}, dict(path=0, plan="runs", fixed="mixed")),
    "fixed-cam-major-mixed": ("54cams", {"PSBA_LIN_GLOBAL_ACC": "1"}, dict(path=0, fixed="mixed")),
    "fixed-v1-mixed": ("54cams", {"PSBA_LIN_V1": "1"}, dict(path=0, fixed="mixed")),
    "fixed-block-ranges-mixed": ("54cams", {"PSBA_SCHUR_BLOCK_GROUPS": "1", "PSBA_SCHUR_SPLIT": "3"},
                                 dict(path=0, plan="split3", fixed="mixed")),
    "fixed-tr-coeff-mixed": ("7cams", {}, dict(path=0, coeff=(2.0, -2.0), fixed="mixed")),  # the placeholder is 2
    "fixed-lens-robust-mixed": ("lens54", {}, dict(path=0, lens=True, fixed="mixed")),
    "fixed-ranks-mixed": ("54cams", {"PSBA_SCHUR_PACKED": "1"}, dict(path=0, ranks=2, fixed="mixed")),
    "fixed-long": ("long", {}, dict(path=1, fixed="long", mirror_label="fixed-long (mirror: atomic)")),
    # 54cams scaled by 2^-22: the largest free diagonal entry lies below the placeholder (test_gpu_fixed_entrywise.py)
    "fixed-rows-scaled-mixed": ("54cams-scaled", {}, dict(path=0, fixed="mixed")),
}

WORST = {}  # (route, quantity) -> worst bound ratio
FINDINGS = []  # the exact parts that did not hold inside the running exact_parts(): all of them, not only the first


def exact(cond, msg):
    if not cond:
        FINDINGS.append(msg)


@contextlib.contextmanager
def exact_parts():
    """Collects what exact() finds in its body and reports all of it at the end, also when the body raised."""
    del FINDINGS[:]
    try:
        yield
    except Exception as err:
        if FINDINGS:
            raise AssertionError("\n".join(FINDINGS) + f"\n(and then: {err!r})") from err
        raise
    assert not FINDINGS, "\n".join(FINDINGS)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        routes = sorted({r for r, _ in WORST})
        lines = [f"  {r}: " + ", ".join(f"{q} {v:.2e}" for (rr, q), v in WORST.items() if rr == r) for r in routes]
        print("\nworst bound ratio per route and quantity:\n" + "\n".join(lines))


def judge(route, what, got, exact, bound, mask=None):
    got = np.asarray(got)
    if mask is not None:
        got, exact, bound = got[mask], exact[mask], np.asarray(bound)[mask]
    r, k = ar.excess(got.reshape(exact.shape), exact, bound)
    WORST[(route, what)] = max(WORST.get((route, what), 0.0), r)
    if not r <= 1.0:
        g = got.reshape(-1)[k]
        x = float(np.asarray(exact).reshape(-1)[k])
        b = float(np.asarray(bound).reshape(-1)[k])
        raise AssertionError(f"{route} {what}: entry {k} = {g!r}, exact {x!r}, |diff| {abs(g - x):.3e} "
                             f"> bound {b:.3e} (ratio {r:.3e})")


def judge_scalar(route, what, got, exact, bound):
    judge(route, what, np.array([got]), np.array([exact]), np.array([bound]))


def _long_problem():
    """400 cameras, 300 ordinary points and two points seen by 300 cameras each (test_gpu_configs.py)."""
    import psba_amd.synth as synth
    from psba_amd.capi import Problem
    base = synth.make_problem(n_cams=400, n_pts=300, mean_track=5.0, seed=4242)
    lng = synth.make_problem(n_cams=400, n_pts=2, mean_track=300.0, seed=4242, min_track=300, max_track=300, shard=1)
    cut = 150
    ocut = int(np.searchsorted(base["iidx"], cut))
    l0 = lng["iidx"] == 0

    def cat(a, b, c, d):
        return np.concatenate([a, b, c, d])
    iidx = cat(base["iidx"][:ocut], np.full(300, cut, np.int32), base["iidx"][ocut:] + 1, np.full(300, 301, np.int32))
    jidx = cat(base["jidx"][:ocut], lng["jidx"][l0], base["jidx"][ocut:], lng["jidx"][~l0])
    impts = cat(base["impts"][:ocut], lng["impts"][l0], base["impts"][ocut:], lng["impts"][~l0])
    pts = np.concatenate([base["pts"][:cut], lng["pts"][:1], base["pts"][cut:], lng["pts"][1:]])
    return Problem(K=base["K"], initrot=base["initrot"], cams=base["cams"], pts=pts, impts=impts,
                   iidx=iidx.astype(np.int32), jidx=jidx.astype(np.int32), nC=400, nP=302, nO=int(iidx.size))


def problem(name, problems):
    import psba_amd.synth as synth
    if name == "venice16":
        return synth.venice_shaped(n_pts=12000, cluster=16)
    if name == "venice1":
        return synth.venice_shaped(n_pts=12000, cluster=1)
    if name == "long":
        return _long_problem()
    if name == "sparse60":
        return synth.make_problem(n_cams=60, n_pts=6000, mean_track=5.0, seed=137)
    if name == "lens54":  # distortion, covariances and 5 % outliers of the robust tests' default one-try case
        from test_gpu_robust import _one_try_case
        return _one_try_case("default")
    if name == "54cams-scaled":
        return fr.scaled_problem(problems["54cams"])
    return problems[name]


_MASKS = {}  # (problem name, mask name) -> (fc, fp, info)


def mask_of(name, kind, prob, lens=None):
    """The mask `kind` of tests/fixed_ref.py for the problem, computed once on the host and printed.  mixed: the camera
    with the largest diagonal entry of U = sum A^T A is taken from the numpy twin's Jacobian blocks (with the
    distortion of a lens case), not from the code under test."""
    if (name, kind) not in _MASKS:
        if kind == "mixed":
            from lens_twin import Twin
            A = (Twin(prob) if lens is None else Twin(prob, lens[0])).linearize()[1]
            d = np.zeros((int(prob["nC"]), 6))
            np.add.at(d, np.asarray(prob["jidx"]), (A * A).sum(axis=1))
            m = fr.mixed_mask(prob, int(np.argmax(d.max(axis=1))))
        else:
            m = {"island": fr.island_mask, "long": fr.long_mask}[kind](prob)
        assert 0 < int(m[0].sum()) < int(prob["nC"]) and 0 < int(m[1].sum()) < int(prob["nP"])
        print(f"\n{name} {kind} mask: {m[2]}")
        _MASKS[(name, kind)] = m
    return _MASKS[(name, kind)]


def minus_zero_rotation(h):
    """Camera 0 (fixed under every mask): its zero rotation coordinates become -0.0 through psba_set_params, so a
    proposal formed as cams + 0.0 instead of a select shows as +0.0.  Returns how many were set."""
    cams, pts = h.get_params()
    z = cams[0, :3] == 0.0
    cams[0, :3] = np.where(z, -0.0, cams[0, :3])
    h.set_params(cams, pts)
    back = h.get_params()[0]
    assert fr.same_bits(back, cams)
    return int(z.sum())


def _handle(prob, lens, solver=0, rank=None, fixed=None):
    import psba_amd
    h = psba_amd.Psba(0)
    if solver:
        h.set_solver(solver)
    if rank is not None:
        h.set_rank_layout(*rank)
    h.upload_problem(prob)
    if lens is not None:
        kc, cov, c = lens
        h.set_distortion(kc)
        h.set_obs_covariance(cov)
        h.set_robust_loss(LOSS_HUBER, c)
    if fixed is not None:
        h.set_fixed(fixed[0], fixed[1])
        assert h.fixed_counts() == (int(np.count_nonzero(fixed[0])), int(np.count_nonzero(fixed[1])))
    return h


def _slack(prob, e, lens):
    """RESIDUAL_SLACK per observation: |proj| from k_residual's e (no lens model) or from the numpy twin."""
    m = np.asarray(prob["impts"], dtype=np.float64).reshape(-1, 2)
    if lens is None:
        return ar.residual_slack(m, m - np.asarray(e).reshape(-1, 2))
    from lens_twin import Twin, whitening
    kc, cov, _ = lens
    return ar.residual_slack(m, Twin(prob, kc).project(), whitening(np.asarray(cov, dtype=np.float64).reshape(-1, 2, 2)))


def _jac_slack(es, lens):
    return None if lens is None else ar.robust_jac_slack(es, lens[2])


def _mirror_k1(route, h, prob, coeff, coeff_g, lens, cam_major, fixed=None, owner=True):
    """K1 through the mirror verbs, judged from the dumped blocks; returns (JA, JB, e, W, g) of the last linearization.
    fixed = (fc, fp): the placeholder rule on the reference and the exact parts; owner: this rank owns the camera
    terms (the placeholder of a fixed camera is written there only)."""
    from psba_amd import capi
    nC, nP = int(prob["nC"]), int(prob["nP"])
    JA, JB = h.compute_jacobiQT()
    ex = h.compute_exQT(capi.PARAMS_CUR)
    es = _slack(prob, ex, lens)
    k1 = ar.k1_sums(JA, JB, ex, prob["iidx"], prob["jidx"], nC, nP, coeff, coeff_g, e_slack=es,
                    recomputed=("U", "ga") if cam_major else (), jac_slack=_jac_slack(es, lens))
    if fixed is not None:
        k1 = fr.install(k1, fixed[0], fixed[1], coeff, owner)
    U, V = h.compute_U(coeff), h.compute_V(coeff)
    judge(route, "U", U, *k1["U"])
    judge(route, "V", V, *k1["V"])
    W = h.compute_Wblks(coeff)
    judge(route, "W", W, *k1["W"])
    g = h.compute_g(coeff_g)  # the last relinearization: K2 and K3 read its U, V, g
    judge(route, "g", g, *k1["g"])
    if fixed is not None:
        fc, fp = fr.flags(*fixed)
        oc, op = fc[np.asarray(prob["jidx"])], fp[np.asarray(prob["iidx"])]
        exact(fr.plus_zero(JA.reshape(-1, 12)[oc]) and fr.plus_zero(JB.reshape(-1, 6)[op]), f"{route}: masked A, B")
        assert np.all(np.any(JA.reshape(-1, 12)[~oc] != 0, axis=1)) and np.all(np.any(JB.reshape(-1, 6)[~op] != 0, axis=1))
        place = coeff if owner else 0.0
        exact(fr.same_bits(U.reshape(-1, 6, 6)[fc], np.broadcast_to(place * np.eye(6), (int(fc.sum()), 6, 6))),
              f"{route}: U of a fixed camera is not {place} I")
        exact(fr.same_bits(V.reshape(-1, 3, 3)[fp], np.broadcast_to(coeff * np.eye(3), (int(fp.sum()), 3, 3))),
              f"{route}: V of a fixed point is not {coeff} I")
        exact(fr.plus_zero(W.reshape(-1, 18)[oc | op]), f"{route}: a masked row of W is not +0.0")
        exact(fr.plus_zero(g[fr.fixed_entries(fc, fp)]), f"{route}: g of a fixed block is not +0.0")
        # the maximum against the one over the free blocks of these very U, V (the GPU's own; their sums are redone by
        # compute_g's relinearization in another order of the adds: the relative 1e-12 of tests/test_gpu_fixed.py).
        # This holds the verb to the blocks it reads; it sees a forgotten mask only where the free entries lie below
        # the placeholder, i.e. on fixed-rows-scaled-mixed (and in test_gpu_fixed_entrywise.py), not on the others
        want = fr.free_max(U, V, fc, fp)
        for what, got in (("psba_max_diag", h.max_diag()), ("psba_maxElmOfUV", h.maxElmOfUV())):
            assert abs(got - want) <= 1e-12 * want, f"{route}: {what} {got!r}, over the free blocks {want!r}"
    return JA, JB, ex, W, g


def _exact_dense_S(what, S, fc, d, lower):
    """Rows and columns of fixed cameras in a dense S: exactly zero off the diagonal block, the block d I on its bit
    patterns.  lower: only the lower triangle is written (the fused routes)."""
    S = np.asarray(S)
    nA = S.shape[0]
    tri = np.tril(np.ones((6, 6), dtype=bool)) if lower else np.ones((6, 6), dtype=bool)
    for j in np.flatnonzero(fc):
        j0 = 6 * j
        blk = S[j0:j0 + 6, j0:j0 + 6]
        exact(fr.same_bits(blk[tri], (d * np.eye(6))[tri]),
              f"{what}: diagonal block of fixed camera {j} is not {d!r} I")
        exact(fr.plus_zero(S[j0:j0 + 6, :j0]) and fr.plus_zero(S[j0 + 6:, j0:j0 + 6]),
              f"{what}: row / column of fixed camera {j} is not +0.0 off the diagonal block")
        if not lower:
            exact(fr.plus_zero(S[j0:j0 + 6, j0 + 6:]) and fr.plus_zero(S[:j0, j0:j0 + 6]),
                  f"{what}: row / column of fixed camera {j} is not +0.0 off the diagonal block (upper triangle)")
    return nA


def _exact_block_S(what, jk, blocks, fc, d):
    """The same on a list of 6 x 6 blocks (block-sparse and packed layouts); of a diagonal block the lower triangle."""
    tri = np.tril(np.ones((6, 6), dtype=bool))
    seen = 0
    for (j, k), B in zip(jk, blocks):
        if j == k and fc[j]:
            exact(fr.same_bits(B[tri], (d * np.eye(6))[tri]),
                  f"{what}: diagonal block of fixed camera {j} is not {d!r} I")
            seen += 1
        elif fc[j] or fc[k]:
            exact(fr.plus_zero(B), f"{what}: block ({j}, {k}) of a fixed camera is not +0.0")
    assert seen == int(np.count_nonzero(fc)), f"{what}: {seen} diagonal blocks of fixed cameras"


def _fused_reference(JA, JB, ex, prob, coeff, coeff_g, lens, mu, r=1, fixed=None):
    """The reference of the fused chain from the dumped blocks, the K1 envelope and JACOBIAN_SLACK carried through.
    fixed = (fc, fp): the placeholder rule, (coeff + mu) I once rounded on the fixed blocks (also summed over ranks:
    only the rank that owns the camera terms writes it)."""
    nC, nP = int(prob["nC"]), int(prob["nP"])
    iidx, jidx = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    es = _slack(prob, ex, lens)
    k1 = ar.k1_sums(JA, JB, ex, iidx, jidx, nC, nP, coeff, coeff_g, e_slack=es,
                    recomputed=("U", "ga", "V", "W", "gb"), jac_slack=_jac_slack(es, lens))
    if fixed is None:
        Ux, eU = ar.damped(*k1["U"], mu)
        Vx, eV = ar.damped(*k1["V"], mu)
    else:
        k1 = fr.install(k1, fixed[0], fixed[1], coeff)
        Ux, eU = fr.damped(*k1["U"], mu, fixed[0], coeff)
        Vx, eV = fr.damped(*k1["V"], mu, fixed[1], coeff)
    Wx, eW = k1["W"]
    gx, eg = k1["g"]
    ref = ar.schur(Ux, Wx, Vx, gx, iidx, jidx, nC, nP, r=r, envU=eU, envW=eW, envV=eV, envg=eg)
    return ref, Wx, eW, gx, eg


def _judge_k3(route, prob, ref, dp, JA, JB, ex, Wx, eW, gx, eg, coeff, read_w, sc_sum, newp, s_new, e_new, mu, lens,
              r=1):
    nC, nP = int(prob["nC"]), int(prob["nP"])
    nA = 6 * nC
    iidx, jidx = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    dpa = dp[:nA]
    if read_w:
        eb, e_eb = ar.eb_ref(gx, dpa, iidx, jidx, nC, nP, W=Wx, envW=eW, envg=eg)
    else:
        eb, e_eb = ar.eb_ref(gx, dpa, iidx, jidx, nC, nP, JA=JA, JB=JB, coeff=coeff, envg=eg,
                             jac_slack=_jac_slack(_slack(prob, ex, lens), lens))
    judge(route, "dpb", dp[nA:], *ar.dpb_ref(ref["Vinv"], ref["Vinv_env"], eb, e_eb))
    loss = (LOSS_HUBER, lens[2]) if lens is not None else (0, 1.0)
    want = ar.try_scalars(dp, newp, mu, gx, nA, s_new, e_slack=_slack(prob, e_new, lens), envg=eg, loss=loss, r=r)
    for what, (x, b) in want.items():
        judge_scalar(route, what, sc_sum[what], x, b)


def _pin_route(case, opt, h, prob):
    from psba_amd import capi
    if "path" in opt:
        assert h.schur_path() == opt["path"], f"{case}: psba_schur_path {h.schur_path()}"
    if "plan" in opt:
        plan = capi.schur_plan(prob["nC"], prob["nP"], prob["iidx"], prob["jidx"])
        if opt["plan"] == "runs":
            assert plan["run_tasks"] > 0, f"{case}: the plan has no runs"
        else:  # block-range groups, three workgroups (slabs) each
            assert plan["run_tasks"] == 0 and plan["wg"].shape[0] >= 3 * plan["groups"], f"{case}: {plan['groups']} groups"


@pytest.mark.parametrize("case", list(CASES))
def test_assembly_entrywise(case, problems, monkeypatch):
    name, env, opt = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = problem(name, problems)
    lens = None
    if opt.get("lens"):
        prob, kc, cov = prob
        lens = (kc, cov, 2.0)  # the robust tests' Huber scale (whitened pixels)
    fixed = mask_of(name, opt["fixed"], prob, lens)[:2] if "fixed" in opt else None
    if opt.get("ranks"):
        with exact_parts():
            _ranks_case(case, opt, prob, fixed)
        return
    coeff, coeff_g = opt.get("coeff", (1.0, 1.0))
    sparse = opt.get("solver", 0) == 1
    cam_major = CAM_ACC * 8 * int(prob["nC"]) > CAM_LDS_MAX or "PSBA_LIN_GLOBAL_ACC" in env
    h = _handle(prob, lens, opt.get("solver", 0), fixed=fixed)
    with contextlib.ExitStack() as stack:  # (left in reverse: the exact parts are reported, then the handle closed)
        stack.callback(h.close)
        stack.enter_context(exact_parts())
        _pin_route(case, opt, h, prob)
        if fixed is not None:
            print(f"\n{case}: {minus_zero_rotation(h)} rotation coordinates of camera 0 set to -0.0")
        JA, JB, ex, mu, W, g = mirror_layer(opt.get("mirror_label", case), h, prob, coeff, coeff_g, lens, cam_major,
                                            opt.get("read_w", False), sparse, fixed)
        fused_layer(case, h, prob, JA, JB, ex, mu, coeff, coeff_g, lens, opt.get("read_w", False), sparse, fixed)
        if fixed is not None and opt["fixed"] == "island":
            _island_properties(case, h, prob, mask_of(name, "island", prob)[2], sparse, W, g, mu)


def mirror_layer(route, h, prob, coeff, coeff_g, lens, cam_major, read_w, sparse, fixed=None):
    """Every sba_func.h verb from the GPU's own dumped inputs; returns the dumped (JA, JB, e), mu = 1e-3 max diag and
    the W and g of the last linearization."""
    from psba_amd import capi
    nC, nP = int(prob["nC"]), int(prob["nP"])
    nA = 6 * nC
    iidx, jidx = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    JA, JB, ex, W, g = _mirror_k1(route, h, prob, coeff, coeff_g, lens, cam_major, fixed)
    mu = 1e-3 * h.max_diag()
    if sparse:
        return JA, JB, ex, mu, W, g
    Us, Vs = h.update_UV(mu)
    Us, Vs = Us.reshape(-1, 6, 6), Vs.reshape(-1, 3, 3)
    Uc, Vc = h.update_UV(0.0)
    h.update_UV(mu)
    for what, got, base in (("U*", Us, Uc.reshape(-1, 6, 6)), ("V*", Vs, Vc.reshape(-1, 3, 3))):
        x, e = ar.damped(base, np.zeros(base.shape), mu)
        judge(route, what, got, x, e)
    if fixed is not None:  # the placeholders after update_UV: coeff I, and the once-rounded (coeff + mu) I
        fc, fp = fr.flags(*fixed)
        fx = fr.fixed_entries(fc, fp)
        d = np.float64(coeff) + np.float64(mu)
        for got, f, n, v in ((Uc, fc, 6, coeff), (Vc, fp, 3, coeff), (Us, fc, 6, d), (Vs, fp, 3, d)):
            exact(fr.same_bits(got.reshape(-1, n, n)[f], np.broadcast_to(v * np.eye(n), (int(f.sum()), n, n))),
                  f"{route}: a fixed block of update_UV is not {v!r} I")
    rc, Vinv = h.compute_Vinv()
    assert rc == capi.PSBA_OK
    ref = ar.schur(Us, W, Vs, g, iidx, jidx, nC, nP)
    judge(route, "Vinv", Vinv, ref["Vinv"], ref["Vinv_env"])
    judge(route, "Y", h.compute_Yblks(), ref["Y"], ref["Y_env"])
    S = h.compute_S()
    blk, _ = ar.dense_to_blocks(S, ref["jk"])
    judge(route, "S", blk, ref["S"], ref["S_env"])
    assert not np.any(ar.outside_blocks(S, ref["jk"], nC)), f"{route}: S has entries outside its blocks"
    ea = h.compute_ea()
    judge(route, "ea", ea, ref["ea"], ref["ea_env"])
    rc, dpa = h.SPDinv_matVec()
    assert rc == capi.PSBA_OK
    eb = h.compute_eb()
    want = ar.eb_ref(g, dpa, iidx, jidx, nC, nP, W=W) if read_w else \
        ar.eb_ref(g, dpa, iidx, jidx, nC, nP, JA=JA, JB=JB, coeff=coeff,
                  jac_slack=_jac_slack(_slack(prob, ex, lens), lens))
    judge(route, "eb", eb, *want)
    dp = h.compute_dpb()
    assert np.array_equal(dp[:nA], dpa)
    judge(route, "dpb", dp[nA:], *ar.dpb_ref(ref["Vinv"], ref["Vinv_env"], eb))
    if fixed is not None:
        _exact_dense_S(f"{route} S", S, fc, d, lower=False)
        exact(fr.plus_zero(ea[fx[:nA]]), f"{route}: e_a of a fixed camera is not +0.0")
        exact(fr.plus_zero(dp[fx]), f"{route}: dp of a fixed block is not +0.0")
    h.restore_UVdiag()
    return JA, JB, ex, mu, W, g


def fused_layer(route, h, prob, JA, JB, ex, mu, coeff, coeff_g, lens, read_w, sparse, fixed=None, linearize=True):
    """psba_linearize ... psba_get_dp against the reference built from the dumped blocks (JA, JB, e).  linearize=False:
    the handle already holds the linearization to judge (the one psba_linearize_ahead queued and psba_accept kept)."""
    from psba_amd import capi
    nC, nP = int(prob["nC"]), int(prob["nP"])
    nA = 6 * nC
    ref, Wx, eW, gx, eg = _fused_reference(JA, JB, ex, prob, coeff, coeff_g, lens, mu, fixed=fixed)
    if fixed is not None:
        fc, fp = fr.flags(*fixed)
        fx = fr.fixed_entries(fc, fp)
        d = np.float64(coeff) + np.float64(mu)
        cur = np.concatenate([x.reshape(-1) for x in h.get_params(capi.PARAMS_CUR)])
    if linearize:
        h.linearize(coeff, coeff_g)
    if fixed is not None:
        exact(fr.plus_zero(h.get_gradient()[fx]), f"{route}: the gradient of a fixed block is not +0.0")
    h.schur_assemble(mu)
    if sparse:
        jk, val, ea = h.get_sparse_S()
        slot = np.searchsorted(ref["jk"][:, 0] * nC + ref["jk"][:, 1], jk[:, 0] * nC + jk[:, 1])
        assert np.array_equal(ref["jk"][slot], jk), f"{route}: a block outside the pattern"
        diag = jk[:, 0] == jk[:, 1]
        mask = np.ones(val.shape, dtype=bool)
        mask[diag] &= np.tril(np.ones((6, 6), dtype=bool))
        judge(route, "S", val, ref["S"][slot], ref["S_env"][slot], mask)
        # every block of the pattern is held, as (j, k) or as (k, j)
        held = jk[:, 0] * nC + jk[:, 1]
        jr, kr = ref["jk"][:, 0], ref["jk"][:, 1]
        assert np.all(np.isin(jr * nC + kr, held) | np.isin(kr * nC + jr, held)), \
            f"{route}: the block-sparse S misses blocks"
        if fixed is not None:
            _exact_block_S(f"{route} S", jk, val, fc, d)
    else:
        buf = h.get_reduce_buffer()
        n32 = (nA + 31) // 32 * 32
        S = buf[:n32 * n32].reshape(n32, n32)[:nA, :nA]
        ea = buf[n32 * n32:n32 * n32 + nA]
        blk, mask = ar.dense_to_blocks(S, ref["jk"], lower=True)
        judge(route, "S", blk, ref["S"], ref["S_env"], mask)
        assert not np.any(ar.outside_blocks(S, ref["jk"], nC, lower=True)), \
            f"{route}: the lower triangle of S has entries outside its blocks"
        if fixed is not None:
            _exact_dense_S(f"{route} S", S, fc, d, lower=True)
    judge(route, "ea", ea, ref["ea"], ref["ea_env"])
    if fixed is not None:
        exact(fr.plus_zero(ea[fx[:nA]]), f"{route}: e_a of a fixed camera is not +0.0")
    h.schur_reduce()
    rc = h.schur_solve()
    assert rc == capi.PSBA_OK
    sc = h.backsub(mu)
    assert sc.status == 0
    dp = h.get_dp()
    cams, pts = h.get_params(capi.PARAMS_NEW)
    newp = np.r_[cams.reshape(-1), pts.reshape(-1)]
    if fixed is not None:
        exact(fr.plus_zero(dp[fx]), f"{route}: dp of a fixed block is not +0.0")
        exact(fr.same_bits(newp[fx], cur[fx]), f"{route}: the proposal's fixed blocks are not the current bits")
        assert not np.array_equal(newp[~fx], cur[~fx])
    e_new = h.compute_exQT(capi.PARAMS_NEW)
    s_new = h.obs_sq_residuals(capi.PARAMS_NEW) if lens is not None else \
        (ar.ld(e_new).reshape(-1, 2) ** 2).sum(axis=1)
    sums = {k: getattr(sc, k) for k in ("dp_l2", "gain_den", "new_cost", "newp_l2")}
    _judge_k3(route, prob, ref, dp, JA, JB, ex, Wx, eW, gx, eg, coeff, read_w, sums, newp, s_new, e_new, mu, lens)
    return sc, dp


def _island_properties(case, h, prob, info, sparse, W, g, mu):
    """The island mask on an assembled try: every W of the free point that sees only fixed cameras is +0.0 (and its
    g_b is not), and the free camera that sees only fixed points has no entry in S off its diagonal block (the block
    itself is U*_j: the reference of the judge above has no other term in it)."""
    iidx = np.asarray(prob["iidx"])
    nA = 6 * int(prob["nC"])
    pt, cam = info["island_point"], info["island_cam"]
    assert fr.plus_zero(W.reshape(-1, 18)[iidx == pt]) and np.all(g[nA + 3 * pt:nA + 3 * pt + 3] != 0.0), \
        f"{case}: the island point {pt}"
    h.linearize(1.0, 1.0)
    h.schur_assemble(mu)
    if sparse:
        jk, val, _ = h.get_sparse_S()
        off = ((jk[:, 0] == cam) | (jk[:, 1] == cam)) & (jk[:, 0] != jk[:, 1])
        assert not np.any(val[off]), f"{case}: the island camera {cam} has entries off its diagonal block"
        assert np.all(np.diagonal(val[(jk[:, 0] == cam) & (jk[:, 1] == cam)][0]) > 0)
    else:
        n32 = (nA + 31) // 32 * 32
        S = h.get_reduce_buffer()[:n32 * n32].reshape(n32, n32)[:nA, :nA]
        c0 = 6 * cam
        assert not np.any(S[c0:c0 + 6, :c0]) and not np.any(S[c0 + 6:, c0:c0 + 6]), \
            f"{case}: the island camera {cam} has entries off its diagonal block"
        assert np.all(np.diagonal(S[c0:c0 + 6, c0:c0 + 6]) > 0)


def _ranks_case(case, opt, prob, fixed=None):
    """Two point shards (capi.shard_problem), one handle each with a rank layout; PSBA_SCHUR_PACKED makes them take
    the packed route, whose buffers (the lower block triangle in canonical order, e_a in six upper slots of each
    diagonal block) are added on the host, as the all-reduce would.  fixed: camera flags replicated, point flags
    sharded with the points; only rank 0 writes the placeholder of a fixed camera, so the summed diagonal block is
    (coeff + mu) I exactly, as on a single handle."""
    from psba_amd import capi
    nr = opt["ranks"]
    nC = int(prob["nC"])
    nA = 6 * nC
    if fixed is not None:
        prob = capi.Problem(prob, fixed_cams=fixed[0], fixed_pts=fixed[1])
    shards = [capi.shard_problem(prob, nr, r) for r in range(nr)]
    masks = [(sh["fixed_cams"], sh["fixed_pts"]) if fixed is not None else None for sh in shards]
    hs = [_handle(sh, None, rank=(nr, r), fixed=m) for r, (sh, m) in enumerate(zip(shards, masks))]
    try:
        for h, sh in zip(hs, shards):
            _pin_route(case, opt, h, sh)
            if fixed is not None:
                minus_zero_rotation(h)
        if fixed is not None:
            assert sum(int(np.count_nonzero(m[1])) for m in masks) == int(np.count_nonzero(fixed[1]))
        # mirror: K1 of each shard against its own sums
        parts = [_mirror_k1(f"{case} (rank {r})", h, sh, 1.0, 1.0, None, False, m, owner=r == 0)[:3]
                 for r, (h, sh, m) in enumerate(zip(hs, shards, masks))]
        JA, JB, ex = (np.concatenate([p[k] for p in parts]) for k in range(3))
        ref0 = ar.k1_sums(JA, JB, ex, prob["iidx"], prob["jidx"], nC, int(prob["nP"]))
        if fixed is None:
            mu = 1e-3 * max(float(np.max(np.diagonal(ref0["U"][0], axis1=1, axis2=2))),
                            float(np.max(np.diagonal(ref0["V"][0], axis1=1, axis2=2))))
        else:
            mu = 1e-3 * fr.free_max(ref0["U"][0].astype(np.float64), ref0["V"][0].astype(np.float64), *fixed)
        ref, Wx, eW, gx, eg = _fused_reference(JA, JB, ex, prob, 1.0, 1.0, None, mu, r=nr, fixed=fixed)
        if fixed is not None:
            fc, fp = fr.flags(*fixed)
            fx = fr.fixed_entries(fc, fp)
            cur = np.concatenate([hs[0].get_params()[0].reshape(-1)] + [h.get_params()[1].reshape(-1) for h in hs])
        for h in hs:
            h.linearize(1.0, 1.0)
            h.schur_assemble(mu)
        nblk = nC * (nC + 1) // 2
        assert hs[0].reduce_buffer_size() == 36 * nblk
        total = sum(h.get_reduce_buffer() for h in hs)
        P = total.reshape(nblk, 6, 6)
        j, k = ref["jk"][:, 0], ref["jk"][:, 1]
        low = j >= k
        canon = j[low] * (j[low] + 1) // 2 + k[low]
        mask = np.ones((int(low.sum()), 6, 6), dtype=bool)
        mask[j[low] == k[low]] &= np.tril(np.ones((6, 6), dtype=bool))
        judge(case, "S", P[canon], ref["S"][low], ref["S_env"][low], mask)
        absent = np.ones(nblk, dtype=bool)
        absent[canon] = False
        assert not np.any(P[absent]), f"{case}: packed blocks outside the pattern are not zero"
        dslot = np.arange(nC) * (np.arange(nC) + 1) // 2 + np.arange(nC)
        ea = P[dslot].reshape(nC, 36)[:, EA_SLOT].reshape(-1)
        judge(case, "ea", ea, ref["ea"], ref["ea_env"])
        if fixed is not None:
            d = np.float64(1.0) + np.float64(mu)
            offd = P[canon].copy()
            offd[j[low] == k[low]] = np.tril(offd[j[low] == k[low]])  # (the upper slots of a diagonal block carry e_a)
            _exact_block_S(f"{case} summed packed S", ref["jk"][low], offd, fc, d)
            exact(fr.plus_zero(ea[fx[:nA]]), f"{case}: e_a of a fixed camera is not +0.0")
        sums = dict.fromkeys(("dp_l2", "gain_den", "new_cost", "newp_l2"), 0.0)
        dps, props, e_new = [], [], []
        for h in hs:
            h.set_reduce_buffer(total)
            assert h.schur_solve() == capi.PSBA_OK
            sc = h.backsub(mu)
            assert sc.status == 0
            for key in sums:
                sums[key] += getattr(sc, key)
            dps.append(h.get_dp())
            props.append(h.get_params(capi.PARAMS_NEW))
            e_new.append(h.compute_exQT(capi.PARAMS_NEW))
        assert all(np.array_equal(d[:nA], dps[0][:nA]) for d in dps)  # cameras are replicated
        dp = np.concatenate([dps[0][:nA]] + [d[nA:] for d in dps])
        newp = np.concatenate([props[0][0].reshape(-1)] + [p.reshape(-1) for _, p in props])
        if fixed is not None:
            exact(fr.plus_zero(dp[fx]), f"{case}: dp of a fixed block is not +0.0")
            exact(fr.same_bits(newp[fx], cur[fx]), f"{case}: the proposal's fixed blocks are not the current bits")
            assert all(fr.same_bits(c[fc], props[0][0][fc]) for c, _ in props)
        e_new = np.concatenate(e_new)
        s_new = (ar.ld(e_new).reshape(-1, 2) ** 2).sum(axis=1)
        _judge_k3(case, prob, ref, dp, JA, JB, ex, Wx, eW, gx, eg, 1.0, False, sums, newp, s_new, e_new, mu, None,
                  r=nr)
    finally:
        for h in hs:
            h.close()
