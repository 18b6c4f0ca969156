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
Every entry must satisfy |got - exact| <= its own bound; the module prints the worst bound ratio per route and quantity."""
import numpy as np
import pytest

import assembly_ref as ar

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
}

WORST = {}  # (route, quantity) -> worst bound ratio


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
    return problems[name]


def _handle(prob, lens, solver=0, rank=None):
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


def _mirror_k1(route, h, prob, coeff, coeff_g, lens, cam_major):
    """K1 through the mirror verbs, judged from the dumped blocks; returns (JA, JB, e, W, g) of the last linearization."""
    from psba_amd import capi
    nC, nP = int(prob["nC"]), int(prob["nP"])
    JA, JB = h.compute_jacobiQT()
    ex = h.compute_exQT(capi.PARAMS_CUR)
    es = _slack(prob, ex, lens)
    k1 = ar.k1_sums(JA, JB, ex, prob["iidx"], prob["jidx"], nC, nP, coeff, coeff_g, e_slack=es,
                    recomputed=("U", "ga") if cam_major else (), jac_slack=_jac_slack(es, lens))
    judge(route, "U", h.compute_U(coeff), *k1["U"])
    judge(route, "V", h.compute_V(coeff), *k1["V"])
    W = h.compute_Wblks(coeff)
    judge(route, "W", W, *k1["W"])
    g = h.compute_g(coeff_g)  # the last relinearization: K2 and K3 read its U, V, g
    judge(route, "g", g, *k1["g"])
    return JA, JB, ex, W, g


def _fused_reference(JA, JB, ex, prob, coeff, coeff_g, lens, mu, r=1):
    """The reference of the fused chain from the dumped blocks, the K1 envelope and JACOBIAN_SLACK carried through."""
    nC, nP = int(prob["nC"]), int(prob["nP"])
    iidx, jidx = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    es = _slack(prob, ex, lens)
    k1 = ar.k1_sums(JA, JB, ex, iidx, jidx, nC, nP, coeff, coeff_g, e_slack=es,
                    recomputed=("U", "ga", "V", "W", "gb"), jac_slack=_jac_slack(es, lens))
    Ux, eU = ar.damped(*k1["U"], mu)
    Vx, eV = ar.damped(*k1["V"], mu)
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
    from psba_amd import capi
    name, env, opt = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = problem(name, problems)
    lens = None
    if opt.get("lens"):
        prob, kc, cov = prob
        lens = (kc, cov, 2.0)  # the robust tests' Huber scale (whitened pixels)
    if opt.get("ranks"):
        return _ranks_case(case, opt, prob)
    coeff, coeff_g = opt.get("coeff", (1.0, 1.0))
    read_w = opt.get("read_w", False)
    sparse = opt.get("solver", 0) == 1
    nC, nP = int(prob["nC"]), int(prob["nP"])
    nA = 6 * nC
    iidx, jidx = np.asarray(prob["iidx"]), np.asarray(prob["jidx"])
    cam_major = CAM_ACC * 8 * nC > CAM_LDS_MAX or "PSBA_LIN_GLOBAL_ACC" in env
    h = _handle(prob, lens, opt.get("solver", 0))
    try:
        _pin_route(case, opt, h, prob)
        # ---- mirror layer ----
        route = opt.get("mirror_label", case)
        JA, JB, ex, W, g = _mirror_k1(route, h, prob, coeff, coeff_g, lens, cam_major)
        mu = 1e-3 * h.max_diag()
        if not sparse:
            Us, Vs = h.update_UV(mu)
            Us, Vs = Us.reshape(-1, 6, 6), Vs.reshape(-1, 3, 3)
            Uc, Vc = h.update_UV(0.0)
            h.update_UV(mu)
            for what, got, base in (("U*", Us, Uc.reshape(-1, 6, 6)), ("V*", Vs, Vc.reshape(-1, 3, 3))):
                x, e = ar.damped(base, np.zeros(base.shape), mu)
                judge(route, what, got, x, e)
            rc, Vinv = h.compute_Vinv()
            assert rc == capi.PSBA_OK
            ref = ar.schur(Us, W, Vs, g, iidx, jidx, nC, nP)
            judge(route, "Vinv", Vinv, ref["Vinv"], ref["Vinv_env"])
            judge(route, "Y", h.compute_Yblks(), ref["Y"], ref["Y_env"])
            S = h.compute_S()
            blk, _ = ar.dense_to_blocks(S, ref["jk"])
            judge(route, "S", blk, ref["S"], ref["S_env"])
            assert not np.any(ar.outside_blocks(S, ref["jk"], nC)), f"{case}: S has entries outside its blocks"
            judge(route, "ea", h.compute_ea(), ref["ea"], ref["ea_env"])
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
            h.restore_UVdiag()
        # ---- fused layer ----
        route = case
        ref, Wx, eW, gx, eg = _fused_reference(JA, JB, ex, prob, coeff, coeff_g, lens, mu)
        h.linearize(coeff, coeff_g)
        h.schur_assemble(mu)
        if sparse:
            jk, val, ea = h.get_sparse_S()
            slot = np.searchsorted(ref["jk"][:, 0] * nC + ref["jk"][:, 1], jk[:, 0] * nC + jk[:, 1])
            assert np.array_equal(ref["jk"][slot], jk), f"{case}: a block outside the pattern"
            diag = jk[:, 0] == jk[:, 1]
            mask = np.ones(val.shape, dtype=bool)
            mask[diag] &= np.tril(np.ones((6, 6), dtype=bool))
            judge(route, "S", val, ref["S"][slot], ref["S_env"][slot], mask)
            # every block of the pattern is held, as (j, k) or as (k, j)
            held = jk[:, 0] * nC + jk[:, 1]
            jr, kr = ref["jk"][:, 0], ref["jk"][:, 1]
            assert np.all(np.isin(jr * nC + kr, held) | np.isin(kr * nC + jr, held)), \
                f"{case}: the block-sparse S misses blocks"
        else:
            buf = h.get_reduce_buffer()
            n32 = (nA + 31) // 32 * 32
            S = buf[:n32 * n32].reshape(n32, n32)[:nA, :nA]
            ea = buf[n32 * n32:n32 * n32 + nA]
            blk, mask = ar.dense_to_blocks(S, ref["jk"], lower=True)
            judge(route, "S", blk, ref["S"], ref["S_env"], mask)
            assert not np.any(ar.outside_blocks(S, ref["jk"], nC, lower=True)), \
                f"{case}: the lower triangle of S has entries outside its blocks"
        judge(route, "ea", ea, ref["ea"], ref["ea_env"])
        h.schur_reduce()
        rc = h.schur_solve()
        assert rc == capi.PSBA_OK
        sc = h.backsub(mu)
        assert sc.status == 0
        dp = h.get_dp()
        cams, pts = h.get_params(capi.PARAMS_NEW)
        newp = np.r_[cams.reshape(-1), pts.reshape(-1)]
        e_new = h.compute_exQT(capi.PARAMS_NEW)
        s_new = h.obs_sq_residuals(capi.PARAMS_NEW) if lens is not None else \
            (ar.ld(e_new).reshape(-1, 2) ** 2).sum(axis=1)
        sums = {k: getattr(sc, k) for k in ("dp_l2", "gain_den", "new_cost", "newp_l2")}
        _judge_k3(route, prob, ref, dp, JA, JB, ex, Wx, eW, gx, eg, coeff, read_w, sums, newp, s_new, e_new, mu, lens)
    finally:
        h.close()


def _ranks_case(case, opt, prob):
    """Two point shards (capi.shard_problem), one handle each with a rank layout; PSBA_SCHUR_PACKED makes them take
    the packed route, whose buffers (the lower block triangle in canonical order, e_a in six upper slots of each
    diagonal block) are added on the host, as the all-reduce would."""
    from psba_amd import capi
    nr = opt["ranks"]
    nC = int(prob["nC"])
    nA = 6 * nC
    shards = [capi.shard_problem(prob, nr, r) for r in range(nr)]
    hs = [_handle(sh, None, rank=(nr, r)) for r, sh in enumerate(shards)]
    try:
        for h, sh in zip(hs, shards):
            _pin_route(case, opt, h, sh)
        # mirror: K1 of each shard against its own sums
        parts = [_mirror_k1(f"{case} (rank {r})", h, sh, 1.0, 1.0, None, False)[:3] for r, (h, sh) in
                 enumerate(zip(hs, shards))]
        JA, JB, ex = (np.concatenate([p[k] for p in parts]) for k in range(3))
        ref0 = ar.k1_sums(JA, JB, ex, prob["iidx"], prob["jidx"], nC, int(prob["nP"]))
        mu = 1e-3 * max(float(np.max(np.diagonal(ref0["U"][0], axis1=1, axis2=2))),
                        float(np.max(np.diagonal(ref0["V"][0], axis1=1, axis2=2))))
        ref, Wx, eW, gx, eg = _fused_reference(JA, JB, ex, prob, 1.0, 1.0, None, mu, r=nr)
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
        e_new = np.concatenate(e_new)
        s_new = (ar.ld(e_new).reshape(-1, 2) ** 2).sum(axis=1)
        _judge_k3(case, prob, ref, dp, JA, JB, ex, Wx, eW, gx, eg, 1.0, False, sums, newp, s_new, e_new, mu, None,
                  r=nr)
    finally:
        for h in hs:
            h.close()
