"""The lean form of the linearization: K1 stores the Jacobian factors A | B | e, K2 and its reduce form S, e_a
and g_a from them.  Needs an MI355X.

One damping try (test_one_try): the standard route and the lean route from the same parameters, both judged by
tests/assembly_ref.py (extended precision) with the bounds tests/test_gpu_assembly_entrywise.py applies to the standard
route -- S (lower triangle), e_a, dp_b, the try's four scalars, the status word, through that module's fused_layer --
and, on the lean route's buffers alone: the upper triangle is the mirror of the lower one bit for bit, the padding is
the standard route's, g_a (what K3 reads: psba_get_gradient after the lean reduce) within the reference's envelope of
g, and dp_a by the backward error of the GPU's own system at ETA_MAX of tests/test_gpu_dense_solve.py.  No bound is
new.  The lean form is reached through psba_levmar only; psba_linearize_lean (a test hook) puts it behind a
psba_linearize, which is how a chosen mu and the coefficients (2, -2) reach it here.

Worst bound ratios measured on an MI355X over the eight shapes (standard | lean; 1.0 = the bound; the module prints
them per shape at its end, DESIGN 5e repeats them): S 6.4e-4 | 6.4e-4, e_a 1.0e-4 | 1.0e-4, dp_b 6.0e-4 | 6.0e-4,
dp_l2 4.3e-2 | 1.4e-2, gain_den 5.9e-5 | 6.0e-5, newp_l2 5.0e-2 | 5.1e-2, new_cost 1.3e-5 | 7.4e-6; lean alone: g_a
4.0e-4, dp_a's backward error 1.5e-2 of ETA_MAX.  What psba_levmar leaves behind (test_state_after_levmar, worst of
the three exits): g 8.1e-4 | 8.1e-4, S 6.6e-5 | 6.3e-5, e_a 2.9e-6 | 3.3e-6.

LM runs (test_levmar_*): psba_levmar lean and with PSBA_LEAN_LIN=0, same accept / reject sequence, each against the
CPU oracle at the tolerances of tests/test_gpu_parity.py (1e-9 per accepted cost, 1e-6 final); one run that starts far
from the solution at the default init_mu, so that the oracle rejects a try (why not a small init_mu: that test's
docstring).  State after the call (test_state_after_*): per exit of psba_levmar the handle answers psba_get_gradient,
psba_max_diag and psba_schur_assemble + the reduce buffer as a standard handle does -- the same error codes, and what
the call left behind is judged like any standard linearization at the handle's own final parameters: g, S and e_a by
the extended-precision reference with the bounds of tests/test_gpu_assembly_entrywise.py, max diag against the CPU
oracle at the 1e-12 of tests/test_gpu_parity.py.  Eligibility (test_disqualified_*): every disqualifier reports
"standard"."""
import numpy as np
import pytest

import assembly_ref as ar
import dense_ref as dr
import test_gpu_assembly_entrywise as tae
from oracle_lib import Oracle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ar.LD_OK, reason="needs an 80-bit long double")]

ETA_MAX = 1e-14  # tests/test_gpu_dense_solve.py: the backward error of a dense camera solve


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = {r: {q: v for (rr, q), v in tae.WORST.items() if rr == r} for r in sorted({r for r, _ in tae.WORST})}
    if rows:
        print("\nworst bound ratio per shape, route and quantity:\n" +
              "\n".join(f"  {r}: " + ", ".join(f"{q} {v:.2e}" for q, v in qs.items()) for r, qs in rows.items()))


def _subset(prob, keep):
    from psba_amd.capi import Problem
    keep = np.asarray(keep)
    out = Problem(prob)
    for k in ("impts", "iidx", "jidx"):
        out[k] = np.ascontiguousarray(np.asarray(prob[k])[keep])
    out["nO"] = int(keep.sum())
    return out


def _tiny():
    """Two cameras, three points, the last point seen by camera 0 only: its V has rank 2."""
    import psba_amd.synth as synth
    p = synth.make_problem(n_cams=2, n_pts=3, mean_track=2.0, seed=11, min_track=2, max_track=2)
    keep = np.ones(int(p["nO"]), dtype=bool)
    keep[-1] = False
    return _subset(p, keep)


def _synth(n_cams, n_pts, track, seed, **kw):
    import psba_amd.synth as synth
    return synth.make_problem(n_cams=n_cams, n_pts=n_pts, mean_track=track, seed=seed, **kw)


# id -> (problem, mu as a fraction of max diag, (coeff, coeff_g))
SHAPES = {
    "tiny-mu1e-3": ("tiny", 1e-3, (1.0, 1.0)),
    "tiny-mu1e-9": ("tiny", 1e-9, (1.0, 1.0)),
    "6cams": ("6cams", 1e-3, (1.0, 1.0)),    # the fused first diagonal block covers exactly cameras 0..5
    "7cams-synth": ("7cams-synth", 1e-3, (1.0, 1.0)),
    "7cams": ("7cams", 1e-3, (1.0, 1.0)),
    "54cams": ("54cams", 1e-3, (1.0, 1.0)),  # more than one LDS group
    # tracks of 40: every K1 wave boundary and every tile boundary has a point's run ending at it or crossing it
    "straddle": ("straddle", 1e-3, (1.0, 1.0)),
    "tr-coeff": ("7cams", 1e-3, (2.0, -2.0)),
}


def _problem(name, problems):
    if name == "tiny":
        return _tiny()
    if name == "6cams":
        return _synth(6, 40, 3.0, 6)
    if name == "7cams-synth":
        return _synth(7, 40, 3.0, 7)
    if name == "straddle":
        return _synth(48, 30, 40.0, 48, min_track=37, max_track=43)
    return problems[name]


def _handle(prob):
    import psba_amd
    h = psba_amd.Psba(0)
    h.upload_problem(prob)
    return h


def _buffers(h, nA):
    buf = h.get_reduce_buffer()
    n32 = (nA + 31) // 32 * 32
    return buf[:n32 * n32].reshape(n32, n32), buf[n32 * n32:n32 * n32 + n32]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_try(shape, problems):
    from psba_amd import capi
    name, frac, (coeff, coeff_g) = SHAPES[shape]
    prob = _problem(name, problems)
    nC, nA = int(prob["nC"]), 6 * int(prob["nC"])
    h = _handle(prob)
    try:
        assert h.schur_path() == 0
        h.linearize(coeff, coeff_g)
        JA, JB = h.compute_jacobiQT()
        ex = h.compute_exQT(capi.PARAMS_CUR)
        mu = frac * h.max_diag()
        # the standard route, then the lean route from the same parameters: the same judge, the same bounds
        tae.fused_layer(f"{shape} standard", h, prob, JA, JB, ex, mu, coeff, coeff_g, None, False, False)
        h.linearize(coeff, coeff_g)
        h.schur_assemble(mu)
        S_std, row_std = _buffers(h, nA)
        h.linearize(coeff, coeff_g)
        h.linearize_lean()
        sc, _ = tae.fused_layer(f"{shape} lean", h, prob, JA, JB, ex, mu, coeff, coeff_g, None, False, False,
                                linearize=False)
        assert sc.status == 0
        # the lean route's buffers: both triangles, the padding, g_a, dp_a
        h.schur_assemble(mu)
        S, row = _buffers(h, nA)
        assert np.array_equal(S[:nA, :nA], S[:nA, :nA].T), f"{shape}: the upper triangle is not the mirror of the lower"
        pad = np.ones(S.shape, dtype=bool)
        pad[:nA, :nA] = False
        assert tae.fr.same_bits(S[pad], S_std[pad]) and tae.fr.same_bits(row[nA:], row_std[nA:]), f"{shape}: padding"
        ref, _, _, gx, eg = tae._fused_reference(JA, JB, ex, prob, coeff, coeff_g, None, mu)
        tae.judge(f"{shape} lean", "ga", h.get_gradient()[:nA], gx[:nA], eg[:nA])
        assert h.schur_solve() == capi.PSBA_OK
        assert h.backsub(mu).status == 0
        dpa = h.get_dp()[:nA]
        eta = dr.backward_error(S[:nA, :nA].copy(), dpa, row[:nA].copy())
        tae.WORST[(f"{shape} lean", "dpa eta / ETA_MAX")] = eta / ETA_MAX
        assert eta <= ETA_MAX, f"{shape}: backward error of dp_a {eta:.3e}"
    finally:
        h.close()


def _lm(prob, lean, monkeypatch, **kw):
    """psba_levmar on a fresh handle, lean or with PSBA_LEAN_LIN=0 (read at upload); returns (handle, result, log)."""
    if lean:
        monkeypatch.delenv("PSBA_LEAN_LIN", raising=False)
    else:
        monkeypatch.setenv("PSBA_LEAN_LIN", "0")
    h = _handle(prob)
    res, log = h.levmar(**kw)
    assert h.lm_ran_lean() == lean
    return h, res, log


# iterations per problem: up to where the cost still moves by more than rounding.  Behind that (7cams: itno 15, 54cams:
# itno 19-20) the cost changes in its last two digits, rho is the quotient of two rounding errors, and the standard route
# and the CPU oracle themselves take different accept / reject decisions
LM_ITERS = {"7cams": 14, "54cams": 18}


@pytest.mark.parametrize("name", list(LM_ITERS))
def test_levmar_lean_and_standard_against_the_oracle(name, golden, problems, monkeypatch):
    g, prob = golden["problems"][name], problems[name]
    kw = dict(max_iter=LM_ITERS[name], tr_handoff=False)
    ores, olog = Oracle(prob).levmar(**kw)
    assert np.all(olog[:, 4] > 0) and len(olog) == LM_ITERS[name]
    for lean in (True, False):
        h, res, log = _lm(prob, lean, monkeypatch, **kw)
        h.close()
        assert np.array_equal(log[:, [0, 4]], olog[:, [0, 4]]), (lean, log[:, [0, 4]])
        for k, want in enumerate(g["err_after_itno"]):
            assert abs(log[k, 1] - want) <= 1e-9 * want, (lean, k, log[k, 1], want)
        assert np.all(np.abs(log[:, 1] - olog[:, 1]) <= 1e-9 * olog[:, 1]), (lean, log[:, 1], olog[:, 1])
        assert abs(res.final_err - ores.final_err) <= 1e-6 * ores.final_err
        assert res.flag == ores.flag and res.iters == ores.iters and res.tries == ores.tries


def test_levmar_with_a_rejected_try(problems, monkeypatch):
    """7cams with its cameras moved (sigma 0.3 on every pose coordinate, seed 7), seven iterations at the default
    init_mu: the oracle accepts five steps and rejects the sixth (rho = -15; checked here on the CPU), so a retry
    assembles once more from the lean records the fifth step's look-ahead left.  No decision of the run hangs on
    rounding (every |rho| >= 0.5), and the run keeps rounding small: the oracle's costs move by 4e-12 relative when the
    points are perturbed by 1e-13 relative (measured on the CPU).  The rejection comes from the far start and not from a
    too-small init_mu, because a small mu makes S ill-conditioned and the costs then miss the oracle's at 1e-9 on the
    standard route already: 54cams with moved cameras and init_mu = 1e-8 rejects its fifth step and follows the oracle
    try by try, but its costs sit 1e-10 (first step, a standard linearization in both forms) to 3e-9 (the rejected try)
    from the oracle's; 7cams with moved points and init_mu = 1e-10 takes 4e-9 to 6e-4 in one iteration, and two
    standard runs do not agree on it.  Both forms follow the oracle."""
    prob = dict(problems["7cams"])
    cams = np.asarray(prob["cams"], dtype=np.float64)
    prob["cams"] = cams + 0.3 * np.random.default_rng(7).standard_normal(cams.shape)
    kw = dict(max_iter=7, tr_handoff=False)
    ores, olog = Oracle(prob).levmar(**kw)
    assert np.all(olog[:5, 4] > 0) and olog[5, 4] == 0 and olog[5, 2] < -1.0 and olog[6, 4] > 0, \
        "the input does not make the oracle reject a try"
    assert np.all(np.abs(olog[:, 2]) >= 0.5)
    for lean in (True, False):
        h, res, log = _lm(prob, lean, monkeypatch, **kw)
        h.close()
        assert np.array_equal(log[:, [0, 4]], olog[:, [0, 4]]), (lean, log[:, [0, 4]], olog[:, [0, 4]])
        assert np.all(np.abs(log[:, 1] - olog[:, 1]) <= 1e-9 * olog[:, 1]), (lean, log[:, 1], olog[:, 1])
        assert abs(res.final_err - ores.final_err) <= 1e-6 * ores.final_err
        assert res.tries == ores.tries == len(olog)


def _answers(h, mu):
    """What the verbs behind psba_levmar answer: (value or error code) of psba_get_gradient, psba_max_diag and
    psba_schur_assemble + the reduce buffer."""
    from psba_amd.capi import PsbaError
    out = []
    for f in (h.get_gradient, h.max_diag, lambda: (h.schur_assemble(mu), h.get_reduce_buffer())[1]):
        try:
            out.append(f())
        except PsbaError as err:
            out.append(err.code)
    return out


EXITS = {
    "max_iter": dict(max_iter=4, tr_handoff=False),
    # met after the first accepted step, with the linearization of the new parameters queued ahead
    "stop_cost": dict(max_iter=50, tr_handoff=False, stop_cost=1e30),
    "tr_handoff": dict(max_iter=50, tr_handoff=True),
}


@pytest.mark.parametrize("exit_", list(EXITS))
def test_state_after_levmar(exit_, problems, monkeypatch):
    from psba_amd import capi
    prob = problems["54cams"]
    nA = 6 * int(prob["nC"])
    n32 = (nA + 31) // 32 * 32
    mu = 1.0
    got = {}
    for lean in (True, False):
        h, res, _ = _lm(prob, lean, monkeypatch, **EXITS[exit_])
        try:
            got[lean] = (res.flag, res.iters, _answers(h, 1.0))
            # psba_linearize with the loop's coefficients: spared where the call left a linearization queued ahead
            # and accepted (stop_cost, tr_handoff) -- the set the verbs then read is the one the call left behind
            h.linearize(1.0, 1.0)
            left = _answers(h, mu)
            assert not any(isinstance(a, int) for a in left)
            g, md, buf = left
            # judged at the handle's own parameters like any standard linearization: g, S and e_a entry by entry by
            # the extended-precision reference, max diag by the CPU oracle at the 1e-12 of tests/test_gpu_parity.py
            cams, pts = h.get_params()
            JA, JB = h.compute_jacobiQT()
            ex = h.compute_exQT(capi.PARAMS_CUR)
            ref, _, _, gx, eg = tae._fused_reference(JA, JB, ex, prob, 1.0, 1.0, None, mu)
            route = f"after {exit_} {'lean' if lean else 'standard'}"
            tae.judge(route, "g", g, gx[:g.size], eg[:g.size])
            S = buf[:n32 * n32].reshape(n32, n32)[:nA, :nA]
            blk, mask = ar.dense_to_blocks(S, ref["jk"], lower=True)
            tae.judge(route, "S", blk, ref["S"], ref["S_env"], mask)
            tae.judge(route, "ea", buf[n32 * n32:n32 * n32 + nA], ref["ea"], ref["ea_env"])
            at = dict(prob)
            at["cams"], at["pts"] = cams, pts
            want = Oracle(at).linearize()["maxdiag"]
            assert abs(md - want) <= 1e-12 * want, (route, md, want)
            if exit_ == "tr_handoff":
                assert res.flag == 2
                tres, _ = h.trust_region(max_iter=3, start_itno=res.iters)
                got[lean] += (tres.flag, tres.iters)
        finally:
            h.close()
    assert got[True][:2] == got[False][:2]
    for a, b in zip(got[True][2], got[False][2]):
        assert isinstance(a, int) == isinstance(b, int) and (not isinstance(a, int) or a == b), (exit_, a, b)
    assert got[True][3:] == got[False][3:]


def _std_after(h, what):
    h.levmar(max_iter=3, tr_handoff=False)
    assert not h.lm_ran_lean(), f"{what}: reported lean"


def test_eligible_handle_reports_lean(problems, monkeypatch):
    monkeypatch.delenv("PSBA_LEAN_LIN", raising=False)
    h = _handle(problems["7cams"])
    try:
        assert not h.lm_ran_lean()  # no psba_levmar yet
        h.levmar(max_iter=3, tr_handoff=False)
        assert h.lm_ran_lean()
    finally:
        h.close()


def test_mirror_verbs_refused_behind_the_hook(problems, monkeypatch):
    """The mirror verbs that assemble S dump Y and V^-1, which the lean route does not form: behind psba_linearize_lean
    they are refused instead of answering with stale buffers, and answer again behind the next psba_linearize."""
    from psba_amd.capi import PsbaError
    monkeypatch.delenv("PSBA_LEAN_LIN", raising=False)
    h = _handle(problems["7cams"])
    try:
        h.linearize(1.0, 1.0)
        h.linearize_lean()
        with pytest.raises(PsbaError):
            h.compute_Yblks()
        h.linearize(1.0, 1.0)
        assert h.compute_Yblks().size == 18 * int(problems["7cams"]["nO"])
    finally:
        h.close()


@pytest.mark.parametrize("why", ["lens", "loss", "fixed", "priors", "pcg", "read-w", "owner", "switch", "hook"])
def test_disqualified_handle_reports_standard(why, problems, monkeypatch):
    import psba_amd
    from psba_amd.capi import PsbaError
    prob = problems["7cams"]
    nC, nP = int(prob["nC"]), int(prob["nP"])
    env = {"read-w": "PSBA_BACK_READ_W", "owner": "PSBA_SCHUR_OWNER"}
    if why in env:
        monkeypatch.setenv(env[why], "1")
    if why in ("switch", "hook"):
        monkeypatch.setenv("PSBA_LEAN_LIN", "0")
    h = psba_amd.Psba(0)
    try:
        if why == "pcg":
            h.set_solver(1)
        if why == "priors":  # priors exist on the free-intrinsics models only: blocks of 11, never lean
            from psba_amd import capi
            h.set_camera_model(capi.CAMERA_FREE_K)
        h.upload_problem(prob)
        if why == "priors":
            cams, _ = h.get_params()
            h.set_priors(cam_mean=cams, cam_info=np.full(cams.shape, 1e-6))
        if why == "lens":
            h.set_distortion(np.full((nC, 5), 1e-3))
        if why == "loss":
            h.set_robust_loss(tae.LOSS_HUBER, 2.0)
        if why == "fixed":
            fc, fp = np.zeros(nC, dtype=np.uint8), np.zeros(nP, dtype=np.uint8)
            fc[0] = fp[0] = 1
            h.set_fixed(fc, fp)
        if why == "hook":  # the test hook refuses where psba_levmar would take the standard form
            h.linearize(1.0, 1.0)
            with pytest.raises(PsbaError):
                h.linearize_lean()
        _std_after(h, why)
    finally:
        h.close()
