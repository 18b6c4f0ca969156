"""PSBA_CAMERA_FREE_K (camera blocks of 11) and PSBA_CAMERA_FREE_KD (blocks of 16) on the GPU, one damping try entry by
entry against the extended-precision sums of the numpy twin (tests/free_ref.py holds the judges and derives every
constant; tests/freekd_twin.py the inputs).  Needs an MI355X.

Inputs: the two-camera problem whose points 1 and 2 are seen once, 7camsvarK, 54camsvarK (first 450 points), and
wide_problem on either side of the camera count at which the finalize kernels' grid-stride loop first takes a second
trip (64 / 65 cameras of 16, 93 / 94 of 11); its cameras 0..4 have 64, 65, 63, 1 and 0 observations, one point has
none and an eighth of the points are seen once.  Dampings: mu = 1e-3 max diag and mu = 1e-6 median diag N.
  * C1  S (both triangles) and e_a in the scale of their own row and column, tol = scaled_tol(p); the identity
        padding; held coordinates; the camera without observations (its block is mu I plus the placeholder, its
        off-diagonal blocks, e_a and dp are exactly zero).
  * C2  dp_a as a solve of the S and e_a read back from the device, in the scaling D = diag(S)^-1/2.
  * C3  dp_b per point as a residual with the device's dp_a, bounded entry by entry.
  * C4  the four try scalars from the device's own step and proposal.
  * C5  many_obs_problem (66 000 observations, 16 units per camera, blocks of several default-length segments):
        cost, gradient (16-block route), one assembly.
  * C6  psba_linearize(2, -2): S / 2 and e_a / -2 are the twin's at mu / 2; held diagonals are exactly 2 + mu.
  * C7  two assemblies are bit-identical beyond 64 (93) cameras and with many segments, for both blocks.
Every case above runs under N + mu I.  Under Marquardt's rule (psba_set_damping, N + mu D) C1 to C7 run
again in tests of their own (..._marquardt), at mu = 1e-3 and 1e-6 (Marquardt's mu is relative), with the default
clamps and with (1e-6, 1e5) beyond the boundary: D itself (psba_get_damping_diag) against the clamp of the
extended-precision diagonal, S and e_a against U_kk + mu D_k and V_i + mu diag(D_i) with d_r = sqrt(N_rr + mu D_r),
the exact parts restated (the camera without observations: fl(mu dmin)), dp_b against V_i + mu diag(D_i), gain_den with
the weights mu D; and a try linearized ahead and accepted on 65 cameras against a fresh handle.
The module prints the worst ratio (found / allowed) per route, input, rule and quantity; DESIGN 7d and 7g keep the
tables."""
import functools

import numpy as np
import pytest

import assembly_ref as ar
import free_ref as fr
from freekd_twin import BAL, many_obs_problem, start_kc, tiny_problem, wide_problem
from test_freekd_twin import P7, P54, scaled_tol
from test_gpu_dense_solve import ETA_MAX

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

ROUTES = {"kd-all": (16, fr.ALL), "kd-bal": (16, BAL), "fk": (11, None)}
SEG_LEN = 64   # the default segment length of the product lists
WIDE = {16: {"wide-below": 64, "wide-above": 65}, 11: {"wide-below": 93, "wide-above": 94}}
INPUTS = ["tiny", "P7", "P54", "wide-below", "wide-above"]
WORST = {}  # (route, input, quantity) -> worst found / allowed
MQ = {"default": fr.Rule(fr.MARQUARDT), "1e5": fr.Rule(fr.MARQUARDT, 1e-6, 1e5)}   # psba_set_damping's clamps
MQ_MUS = {"big": 1e-3, "small": 1e-6}   # Marquardt's mu is relative (test_gpu_damping.py)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        keys = sorted({(r, n) for r, n, _ in WORST})
        lines = [f"  {r} {n}: " + ", ".join(f"{q} {v:.2e}" for (rr, nn, q), v in WORST.items() if (rr, nn) == (r, n))
                 for r, n in keys]
        print("\nworst ratio found / allowed per route, input and quantity:\n" + "\n".join(lines))


def note(route, name, what, ratio):
    WORST[(route, name, what)] = max(WORST.get((route, name, what), 0.0), float(ratio))
    print(f"{route} {name} {what}: {float(ratio):.3e}")


@functools.lru_cache(maxsize=None)
def prob(name, cnp=16):
    if name.startswith("wide"):
        return wide_problem(WIDE[cnp][name])
    return {"tiny": tiny_problem, "P7": P7, "P54": P54, "many": many_obs_problem}[name]()


@functools.lru_cache(maxsize=None)
def ref(name, route):
    """(Route, its extended-precision sums) of one input: computed once, shared, never modified"""
    cnp, free = ROUTES[route]
    rt = fr.Route(prob(name, cnp), cnp, free)
    return rt, fr.sums(rt)


def dampings(rt, sm):
    """(mu = 1e-3 max diag over the free entries, mu = 1e-6 median diag N) and the diagonal of N"""
    diag = np.concatenate([sm["diagU"], sm["diagV"]])
    free = np.ones(rt.nT, dtype=bool)
    free[rt.held] = False
    return {"big": 1e-3 * float(diag[free].max()), "small": 1e-6 * float(np.median(diag))}, diag


@functools.lru_cache(maxsize=None)
def schur_ref(name, route, mu, rule=fr.NO_RULE):
    """S and e_a of the twin's blocks summed in 80-bit (coefficients 1), rounded once to double"""
    rt, sm = ref(name, route)
    S, ea = fr.schur_ref(rt, sm, mu, rule)
    S.setflags(write=False)
    ea.setflags(write=False)
    return S, ea


def handle(name, route, rule=fr.NO_RULE):
    import psba_amd
    cnp, free = ROUTES[route]
    p = prob(name, cnp)
    h = psba_amd.Psba(0)
    if cnp == 16:
        h.set_camera_model(psba_amd.CAMERA_FREE_KD)
        h.upload_problem(p)
        h.set_distortion(start_kc(p["nC"]))
        h.set_intrinsics_mask(free)
    else:
        h.set_camera_model(psba_amd.CAMERA_FREE_K)
        h.upload_problem(p)
    assert h.camera_block() == cnp and h.schur_path() == 5
    if rule.marquardt:
        h.set_damping(rule.kind, rule.dmin, rule.dmax)
        assert h.damping() == tuple(rule)
    return h


def read_system(h, nA):
    """S [nA, nA], e_a [nA] and the whole padded buffer after psba_schur_assemble"""
    n32 = (nA + 31) // 32 * 32
    M = h.get_reduce_buffer().reshape(n32 + 1, n32)
    return M[:nA, :nA].copy(), M[n32, :nA].copy(), M


def check_padding(M, nA):
    n32 = M.shape[1]
    pad = np.zeros((n32 - nA, n32))
    pad[np.arange(n32 - nA), nA + np.arange(n32 - nA)] = 1.0
    assert np.array_equal(M[nA:n32], pad) and np.all(M[:nA, nA:] == 0.0) and np.all(M[n32, nA:] == 0.0)


def check_S_ea(route, name, S, ea, S_want, ea_want, d, cost, label=None):
    """C1's scaled measure; the whole square, so the mirrored upper triangle is judged too"""
    tol = scaled_tol(prob(name.split(" ")[0], ROUTES[route][0]))
    name = label or name
    eS = (np.abs(S - S_want) / np.outer(d, d)).max()
    ee = (np.abs(ea - ea_want) / (d * np.sqrt(cost))).max()
    note(route, name, "S", eS / tol)
    note(route, name, "e_a", ee / tol)
    assert eS <= tol and ee <= tol, f"{route} {name}: scaled S {eS:.3e}, e_a {ee:.3e}, tol {tol:.3e}"
    blk = np.arange(S.shape[0]) // ROUTES[route][0]
    upper = blk[:, None] < blk[None, :]                     # the blocks above the diagonal are copies of those below
    assert np.array_equal(S[upper], S.T[upper])


def check_D(route, label, h, rt, sm, rule, scale=1.0):
    """psba_get_damping_diag / scale against the clamp of the extended-precision diagonal (free_ref.check_damp_diag)"""
    D = h.get_damping_diag()
    assert D.shape == (rt.nT,)
    ratio, k, nlow, nhigh = fr.check_damp_diag(D / scale, np.concatenate([sm["diagUx"], sm["diagVx"]]),
                                               np.concatenate([sm["envdU"], sm["envdV"]]), rule, rt.held)
    note(route, label, "D", ratio)
    print(f"{route} {label}: {nlow} entries of D at dmin, {nhigh} at dmax")
    assert ratio <= 1.0, f"{route} {label}: D[{k}] = {D[k]!r} outside its envelope"
    return D, nlow, nhigh


def one_try(route, name, which_mu, rule=fr.NO_RULE):
    rt, sm = ref(name, route)
    cnp, nA, nT, nC = rt.cnp, rt.nA, rt.nT, rt.nC
    mus, diag = dampings(rt, sm)
    mu, cost = (MQ_MUS if rule.marquardt else mus)[which_mu], sm["cost"]
    tol = scaled_tol(rt.p)
    h = handle(name, route, rule)
    inp, name = name, (f"{name} {rule}" if rule.marquardt else name)
    D = None
    try:
        assert abs(h.residual() - cost) <= 1e-12 * cost
        h.linearize(1.0, 1.0)
        assert abs(h.max_diag() - 1e3 * mus["big"]) <= 1e-11 * 1e3 * mus["big"]
        if cnp == 16:
            gg = h.get_gradient()
            assert np.all(gg[:nA][rt.held] == 0.0)
            dg, allowed = np.abs(gg - sm["g"].astype(np.float64)), tol * np.sqrt(diag) * np.sqrt(cost)
            note(route, name, "g", (dg[diag > 0] / allowed[diag > 0]).max())
            assert np.all(dg <= allowed)                    # (an unobserved block: allowed = 0, g = 0 exactly)
        if rule.marquardt:
            D, nlow, nhigh = check_D(route, name, h, rt, sm, rule)
            if inp.startswith("wide"):                      # the clamps are not idle (test_free_entrywise_ref.py)
                assert (D[:nA] == rule.dmin).sum() >= cnp - (rt.held < cnp).sum() and (D[nA:] == rule.dmin).sum() >= 3
                seen = np.bincount(rt.j, minlength=nC) > 0
                assert rule.dmax > 1e5 or np.all((D[:nA].reshape(nC, cnp) == rule.dmax).sum(axis=1)[seen] >= 1)
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        # ---- C1
        S_want, ea_want = schur_ref(inp, route, mu, rule)
        check_S_ea(route, name, S, ea, S_want, ea_want, fr.scale_diag(rt, sm, mu, rule) if rule.marquardt
                   else np.sqrt(diag[:nA] + mu), cost)
        check_padding(M, nA)
        held = rt.held
        off = S[held].copy()
        off[np.arange(held.size), held] = 0.0
        assert np.all(off == 0.0) and np.all(S[held, held] == 1.0 + mu) and np.all(ea[held] == 0.0)
        empty = np.flatnonzero(np.bincount(rt.j, minlength=nC) == 0)
        if rule.marquardt:                                  # the same checks restated for mu D: fl(mu dmin), 1 + mu
            assert np.array_equal(fr.check_exact_parts(rt, S, ea, mu, rule), empty)
        for j in empty if not rule.marquardt else ():
            rows = np.arange(cnp * j, cnp * j + cnp)
            want = mu * np.eye(cnp)
            hj = held[(held >= rows[0]) & (held <= rows[-1])] - rows[0]
            want[hj, hj] = 1.0 + mu
            assert np.array_equal(S[np.ix_(rows, rows)], want)
            assert np.all(np.delete(S[rows], rows, axis=1) == 0.0) and np.all(ea[rows] == 0.0)
        h.schur_reduce()
        h.schur_solve()
        sc = h.backsub(mu)
        assert sc.status == 0
        dp = h.get_dp()
        newcams, newpts = h.get_params(1)
        assert np.all(dp[:nA][held] == 0.0)
        for j in empty:
            assert np.all(dp[cnp * j:cnp * j + cnp] == 0.0)
        # ---- C2
        eta, fe, kappa = fr.solve_judge(S, ea, dp[:nA])
        note(route, name, "dp_a eta", eta / ETA_MAX)
        note(route, name, "dp_a forward", fe / (2 * kappa * 1e-14))
        assert eta <= ETA_MAX, f"{route} {name}: backward error {eta:.3e} of the scaled system"
        assert fe <= 2 * kappa * 1e-14, f"{route} {name}: forward error {fe:.3e} (cond {kappa:.2e})"
        # ---- C3
        r, bound = fr.dpb_residual(rt, sm, dp, mu, rule)
        ratio, k = ar.excess(r, np.zeros(r.shape, ar.LD), bound)
        note(route, name, "dp_b", ratio)
        assert ratio <= 1.0, (f"{route} {name}: point {k // 3} entry {k % 3}: residual {float(r[k]):.3e} > bound "
                              f"{bound[k]:.3e}")
        unseen = np.flatnonzero(np.bincount(rt.i, minlength=rt.nP) == 0)
        for i in unseen:
            assert np.all(dp[nA + 3 * i:nA + 3 * i + 3] == 0.0)
        # ---- C4
        got = dict(dp_l2=sc.dp_l2, gain_den=sc.gain_den, newp_l2=sc.newp_l2, new_cost=sc.new_cost)
        want = fr.scalars(rt, sm, dp, newcams, newpts, mu, D=D)
        bad = []
        for what, (x, b) in want.items():
            ratio = float(abs(ar.LD(got[what]) - x) / b)
            note(route, name, what, ratio)
            if not ratio <= 1.0:
                bad.append(f"{what} = {got[what]!r}, exact {float(x)!r}, bound {b:.3e}")
        assert not bad, f"{route} {name}: " + "; ".join(bad)
    finally:
        h.close()


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_one_damping_try_entrywise(route, name, which_mu):
    """C1 to C4.  fk / tiny / small is the case Y and dp_b of the 11-block route are formed by substitution for: the
    closed-form inverse they used before gives, in the same fp64 arithmetic on the host, a scaled S error of 4.0e-10
    and e_a 1.5e-10 against tol 2.6e-13 (test_free_entrywise_ref.py)."""
    one_try(route, name, which_mu)


@pytest.mark.parametrize("route", ["kd-all", "fk"])
def test_many_observations(route):
    """C5: the residual kernels' stride loop, 16 units per camera, blocks of three and more segments."""
    from psba_amd import capi
    rt, sm = ref("many", route)
    p, nA, cost = rt.p, rt.nA, sm["cost"]
    tol = scaled_tol(p)
    plan = capi.blockprod_plan(p["nC"], p["nP"], p["iidx"], p["jidx"], SEG_LEN)
    assert np.bincount(plan["segs"][:, 0]).max() >= 3 and np.bincount(p["jidx"]).min() > 14 * 64
    h = handle("many", route)
    try:
        got = h.residual()
        note(route, "many", "cost", abs(got - cost) / (1e-12 * cost))
        assert abs(got - cost) <= 1e-12 * cost
        h.linearize(1.0, 1.0)
        mus, diag = dampings(rt, sm)
        mu = mus["big"]
        assert abs(h.max_diag() - 1e3 * mu) <= 1e-11 * 1e3 * mu
        if rt.cnp == 16:
            gg = h.get_gradient()
            allowed = tol * np.sqrt(diag) * np.sqrt(cost)
            note(route, "many", "g", (np.abs(gg - sm["g"].astype(np.float64)) / allowed).max())
            assert np.all(np.abs(gg - sm["g"].astype(np.float64)) <= allowed)
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        check_S_ea(route, "many", S, ea, *schur_ref("many", route, mu), np.sqrt(diag[:nA] + mu), cost)
        check_padding(M, nA)
    finally:
        h.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_linearize_with_coefficients(route):
    """C6: psba_linearize(2, -2) on 7camsvarK.  U, V, W scale by 2 and g by -2, so S(mu) = 2 S_1(mu / 2) and
    e_a(mu) = -2 e_a,1(mu / 2) (scalings by powers of two: exact), and the placeholder of a held coordinate is the
    coefficient: its diagonal is exactly 2 + mu."""
    rt, sm = ref("P7", route)
    nA = rt.nA
    mus, diag = dampings(rt, sm)
    mu, cost = 2.0 * mus["big"], sm["cost"]
    h = handle("P7", route)
    try:
        h.linearize(2.0, -2.0)
        assert abs(h.max_diag() - 2e3 * mus["big"]) <= 1e-11 * 2e3 * mus["big"]
        if rt.cnp == 16:
            gg = h.get_gradient()
            allowed = scaled_tol(rt.p) * np.sqrt(diag) * np.sqrt(cost)
            note(route, "P7 (2, -2)", "g", (np.abs(gg / -2.0 - sm["g"].astype(np.float64)) / allowed).max())
            assert np.all(np.abs(gg / -2.0 - sm["g"].astype(np.float64)) <= allowed)
            assert np.all(gg[:nA][rt.held] == 0.0)
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        check_S_ea(route, "P7", S / 2.0, ea / -2.0, *schur_ref("P7", route, mu / 2.0),
                   np.sqrt(diag[:nA] + mu / 2.0), cost, label="P7 (2, -2)")
        check_padding(M, nA)
        held = rt.held
        assert np.all(S[held, held] == 2.0 + mu) and np.all(ea[held] == 0.0)
        h.schur_reduce()
        h.schur_solve()
        assert h.backsub(mu).status == 0
        assert np.all(h.get_dp()[:nA][held] == 0.0)
        if route == "kd-bal":
            assert held.size == 7 * rt.nC
    finally:
        h.close()


def assembled_twice(name, route):
    bufs = []
    for _ in range(2):
        h = handle(name, route)
        try:
            h.linearize(1.0, 1.0)
            h.schur_assemble(1e-3 * h.max_diag())
            bufs.append(h.get_reduce_buffer().tobytes())
        finally:
            h.close()
    return bufs


@pytest.mark.parametrize("name", ["wide-above", "many"])
def test_two_assemblies_are_bit_identical(name):
    """C7: the 16-block route sums in an order the upload fixes (no floating-point atomics)."""
    bufs = assembled_twice(name, "kd-bal")
    assert bufs[0] == bufs[1]


@pytest.mark.parametrize("name", ["wide-above", "many"])
def test_two_assemblies_of_blocks_of_11_are_bit_identical(name):
    """C7 for blocks of 11, which run the same kernels: 94 cameras, and blocks of several segments."""
    bufs = assembled_twice(name, "fk")
    assert bufs[0] == bufs[1]


# ---- Marquardt's damping (psba_set_damping): the same judges with N + mu D ------------------------------------
MQ_TRIES = [(n, "default") for n in INPUTS] + [("wide-above", "1e5")]


@pytest.mark.parametrize("which_mu", ["big", "small"])
@pytest.mark.parametrize("name,clamps", MQ_TRIES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_one_damping_try_entrywise_marquardt(route, name, clamps, which_mu):
    """C1 to C4 under PSBA_DAMPING_MARQUARDT at mu = 1e-3 and 1e-6, and D itself (psba_get_damping_diag) against the
    clamp of the extended-precision diagonal.  wide-above is the first second trip of k_free_finalize's grid-stride
    loop, where it reads D[r]; its camera 4 and last point sit at dmin, camera 3 (one observation) just above."""
    one_try(route, name, which_mu, MQ[clamps])


@pytest.mark.parametrize("route", ["kd-all", "fk"])
def test_many_observations_marquardt(route):
    """C5 under Marquardt: D, S and e_a of one assembly."""
    rule, mu = MQ["default"], MQ_MUS["big"]
    rt, sm = ref("many", route)
    label = f"many {rule}"
    h = handle("many", route, rule)
    try:
        h.linearize(1.0, 1.0)
        check_D(route, label, h, rt, sm, rule)
        h.schur_assemble(mu)
        S, ea, M = read_system(h, rt.nA)
        check_S_ea(route, label, S, ea, *schur_ref("many", route, mu, rule), fr.scale_diag(rt, sm, mu, rule), sm["cost"])
        check_padding(M, rt.nA)
    finally:
        h.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_linearize_with_coefficients_marquardt(route):
    """C6 under Marquardt, clamps (1e-6, 1e5): D scales with the coefficient before it is clamped, so
    N_2 + mu clamp(N_2, dmin, dmax) = 2 (N + mu clamp(N, dmin / 2, dmax / 2)) exactly: D / 2, S / 2 and e_a / -2 are the
    reference's at the same mu with both clamps halved; a held diagonal is exactly 2 + mu clamp(2)."""
    rule, mu = MQ["1e5"], MQ_MUS["big"]
    half = rule.halved()
    rt, sm = ref("P7", route)
    nA, label = rt.nA, f"P7 (2, -2) {rule}"
    h = handle("P7", route, rule)
    try:
        h.linearize(2.0, -2.0)
        D, _, nhigh = check_D(route, label, h, rt, sm, half, scale=2.0)
        assert nhigh >= rt.nC and np.all(D[rt.held] == 2.0)
        h.schur_assemble(mu)
        S, ea, M = read_system(h, nA)
        check_S_ea(route, "P7", S / 2.0, ea / -2.0, *schur_ref("P7", route, mu, half), fr.scale_diag(rt, sm, mu, half),
                   sm["cost"], label=label)
        check_padding(M, nA)
        held = rt.held
        assert np.all(S[held, held] == 2.0 + mu * 2.0) and np.all(ea[held] == 0.0)
        h.schur_reduce()
        h.schur_solve()
        assert h.backsub(mu).status == 0
        assert np.all(h.get_dp()[:nA][held] == 0.0)
    finally:
        h.close()


def assembled_twice_marquardt(name, route):
    out = []
    for _ in range(2):
        h = handle(name, route, MQ["default"])
        try:
            h.linearize(1.0, 1.0)
            D = h.get_damping_diag().tobytes()
            h.schur_assemble(MQ_MUS["big"])
            out.append((h.get_reduce_buffer().tobytes(), D))
        finally:
            h.close()
    return out


@pytest.mark.parametrize("route", ["kd-bal", "fk"])
@pytest.mark.parametrize("name", ["wide-above", "many"])
def test_two_marquardt_assemblies_are_bit_identical(name, route):
    """C7 under Marquardt, both blocks; the D vectors of the two handles are bit-identical too."""
    a, b = assembled_twice_marquardt(name, route)
    assert a[0] == b[0] and a[1] == b[1] and len(a[1]) > 0


def full_try(h, mu):
    h.schur_assemble(mu)
    buf = h.get_reduce_buffer().tobytes()
    h.schur_reduce()
    h.schur_solve()
    sc = h.backsub(mu)
    assert sc.status == 0
    return buf, h.get_dp().tobytes(), (sc.dp_l2, sc.gain_den, sc.newp_l2, sc.new_cost)


def test_the_second_diagonal_set_beyond_64_cameras():
    """wide-above, kd-bal, Marquardt: a try whose proposal is linearized ahead (the sequence of
    test_gpu_damping.py::test_the_diagonal_follows_the_look_ahead), accepted; the next full try must be, bit for bit,
    that of a fresh handle set to the accepted parameters and linearized plainly: the second D set and the swap in
    psba_accept with 65 cameras."""
    rule, mu = MQ["default"], MQ_MUS["big"]
    h, h2 = handle("wide-above", "kd-bal", rule), None
    try:
        cost, _ = h.begin()
        h.linearize(1.0, 1.0)
        D0 = h.get_damping_diag()
        h.schur_assemble(mu)
        h.schur_reduce()
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        sc = h.backsub_wait()
        assert sc.status == 0 and sc.new_cost < cost
        cams, pts = h.get_params(1)
        h.accept()
        D1 = h.get_damping_diag()
        assert D1.tobytes() != D0.tobytes()
        h.linearize(1.0, 1.0)                               # (nothing left to do: the linearization came with the accept)
        assert h.get_damping_diag().tobytes() == D1.tobytes()
        got = full_try(h, mu)
        h2 = handle("wide-above", "kd-bal", rule)
        h2.set_params(cams, pts)
        h2.linearize(1.0, 1.0)
        assert h2.get_damping_diag().tobytes() == D1.tobytes()
        want = full_try(h2, mu)
        assert got[0] == want[0], "the reduce buffer after the accepted look-ahead"
        assert got[1] == want[1] and got[2] == want[2]
    finally:
        h.close()
        if h2 is not None:
            h2.close()
