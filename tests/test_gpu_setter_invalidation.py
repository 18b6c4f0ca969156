"""The invalidation rule of the per-problem setters as one table: every verb that changes the model or the
parameters drops what was derived from them, refuses while a damping try is in flight (psba_set_params and
psba_reset_params abandon the try instead) and discards a linearization queued ahead.  Each feature's own interface test
checks its own setter; this file checks all of them by the same rules, per camera model, with a no-op argument (None or
the current value) and with a real one.  Needs an MI355X.

One pair of handles per camera model serves every case: a new upload resets every setting and the state of the try.
The inputs are freekd_twin.tiny_problem() and test_freekd_twin.P7(), camera 1 given the intrinsics of camera 0 so that
the two can form a group.  Nothing here judges a number: the comparisons are refusals, getters and bit equality (the
free-intrinsics route sums in fixed order and uses no floating-point atomics)."""
import functools

import numpy as np
import pytest

from freekd_twin import BAL, start_kc, tiny_problem
from test_freekd_twin import P7

pytestmark = pytest.mark.gpu

NONE10 = (0,) * 10
REAL_MASK = (1, 1, 1, 0, 0, 1, 1, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def problem(name):
    p = dict({"tiny": tiny_problem, "P7": P7}[name]())
    K = np.array(p["K"], dtype=np.float64).reshape(p["nC"], 5).copy()
    K[1] = K[0]
    p["K"] = K
    return p


def kc0(p):
    kc = start_kc(p["nC"])
    kc[1] = kc[0]
    return kc


def flags(n, idx):
    f = np.zeros(n, dtype=np.uint8)
    f[idx] = 1
    return f


def moved(h):
    cams, pts = h.get_params(0)
    return cams * (1.0 + 1e-6), pts * (1.0 + 1e-6)


def groups_labels(p):
    g = np.arange(p["nC"], dtype=np.int32)
    g[1] = g[0]
    return g


class Setter:
    """noop / real: the call with a no-op and with a real argument, (handle, problem) -> None; getter: the setting as
    something == compares; prep: what the real call needs done before psba_linearize; moves_params: the verb clears
    the try's result as well, so psba_accept refuses after it"""

    def __init__(self, noop, real, getter, prep=None, moves_params=False):
        self.call = {"noop": noop, "real": real}
        self.getter, self.prep, self.moves_params = getter, prep, moves_params


def params_bytes(h):
    cams, pts = h.get_params(0)
    return cams.tobytes(), pts.tobytes()


SET_PARAMS = Setter(lambda h, p: h.set_params(*h.get_params(0)), lambda h, p: h.set_params(*moved(h)), params_bytes,
                    moves_params=True)
RESET_PARAMS = Setter(lambda h, p: h.reset_params(), lambda h, p: h.reset_params(), params_bytes,
                      prep=lambda h, p: h.set_params(*moved(h)), moves_params=True)


def _priors(h, p):
    cnp = h.camera_block()
    h.set_priors(np.zeros((p["nC"], cnp)), np.full((p["nC"], cnp), 1e-3), np.asarray(p["pts"]), np.ones((p["nP"], 3)))


def _free_setters():
    import psba_amd
    return {
        "set_held": Setter(lambda h, p: h.set_held(None, None),
                           lambda h, p: h.set_held(flags(p["nC"], [1]), flags(p["nP"], [1])), lambda h: h.held_counts()),
        "set_priors": Setter(lambda h, p: h.set_priors(), _priors, lambda h: h.prior_counts()),
        "set_damping": Setter(lambda h, p: h.set_damping(*h.damping()),
                              lambda h, p: h.set_damping(psba_amd.DAMPING_MARQUARDT, 1e-3, 1e8), lambda h: h.damping()),
        "set_params": SET_PARAMS, "reset_params": RESET_PARAMS}


def setters(model):
    import psba_amd
    if model == "fixed":
        return {
            "set_distortion": Setter(lambda h, p: h.set_distortion(None), lambda h, p: h.set_distortion(kc0(p)),
                                     lambda h: h.lens_model()),
            "set_obs_covariance": Setter(lambda h, p: h.set_obs_covariance(None),
                                         lambda h, p: h.set_obs_covariance(np.tile([2.0, 0.5, 0.5, 1.0], (p["nO"], 1))),
                                         lambda h: h.lens_model()),
            "set_robust_loss": Setter(lambda h, p: h.set_robust_loss(*h.robust_loss()),
                                      lambda h, p: h.set_robust_loss(psba_amd.LOSS_HUBER, 2.0), lambda h: h.robust_loss()),
            "set_fixed": Setter(lambda h, p: h.set_fixed(None, None),
                                lambda h, p: h.set_fixed(flags(p["nC"], [0]), flags(p["nP"], [0])), lambda h: h.fixed_counts()),
            "set_params": SET_PARAMS, "reset_params": RESET_PARAMS}
    s = _free_setters()
    if model == "kd":
        def groups(h):
            rep, n = h.intrinsics_groups()
            return rep.tobytes(), n
        s["set_intrinsics_mask"] = Setter(lambda h, p: h.set_intrinsics_mask(h.intrinsics_mask()),
                                          lambda h, p: h.set_intrinsics_mask(REAL_MASK), lambda h: h.intrinsics_mask())
        s["set_intrinsics_groups"] = Setter(lambda h, p: h.set_intrinsics_groups(None),
                                            lambda h, p: h.set_intrinsics_groups(groups_labels(p)), groups)
        # kc is part of the camera block: the verb moves the parameters, so psba_accept refuses after it, but unlike
        # psba_set_params it is refused while a try is in flight
        s["set_distortion"] = Setter(lambda h, p: h.set_distortion(kc0(p)), lambda h, p: h.set_distortion(2.0 * kc0(p)),
                                     lambda h: h.get_params(0)[0][:, 5:10].tobytes(), moves_params=True)
    return s


NAMES = {"fixed": ("set_distortion", "set_obs_covariance", "set_robust_loss", "set_fixed", "set_params", "reset_params"),
         "fk": ("set_held", "set_priors", "set_damping", "set_params", "reset_params"),
         "kd": ("set_held", "set_priors", "set_damping", "set_params", "reset_params", "set_intrinsics_mask",
                "set_intrinsics_groups", "set_distortion")}
CASES = [(m, s, a) for m in NAMES for s in NAMES[m] for a in ("noop", "real")]
IN_FLIGHT = [c for c in CASES if c[1] not in ("set_params", "reset_params")]
AHEAD = [c for c in CASES if c[0] != "fixed"]


@pytest.fixture(scope="module")
def handles():
    """model -> two handles of that camera model, made on first use and closed with the module"""
    import psba_amd
    made = {}

    def get(model):
        if model not in made:
            pair = psba_amd.Psba(0), psba_amd.Psba(0)
            for h in pair:
                h.set_camera_model({"fixed": psba_amd.CAMERA_FIXED_K, "fk": psba_amd.CAMERA_FREE_K,
                                    "kd": psba_amd.CAMERA_FREE_KD}[model])
            made[model] = pair
        assert sorted(NAMES[model]) == sorted(setters(model))
        return made[model]
    yield get
    for pair in made.values():
        for h in pair:
            h.close()


def baseline(h, model, p, mask=BAL):
    """a new upload (it resets every setting and the try's state), the starting distortion and the mask of the blocks of
    16, Marquardt's damping on the free models so that the diagonal exists"""
    import psba_amd
    h.upload_problem(p)
    if model == "kd":
        h.set_distortion(kc0(p))
        h.set_intrinsics_mask(mask)
    if model != "fixed":
        h.set_damping(psba_amd.DAMPING_MARQUARDT)


def refused(call, code, *words):
    import psba_amd
    with pytest.raises(psba_amd.PsbaError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def try_mu(h, model):
    return 1e-3 if model != "fixed" else 1e-3 * h.max_diag()   # Marquardt's mu is relative


def queue_try(h, model, ahead=False):
    """psba_linearize to psba_backsub_async (and psba_linearize_ahead): a try in flight"""
    h.linearize(1.0, 1.0)
    mu = try_mu(h, model)
    h.schur_assemble(mu)
    h.schur_reduce()
    h.schur_solve()
    h.backsub_async(mu)
    if ahead:
        h.linearize_ahead()


@pytest.mark.parametrize("name", ["tiny", "P7"])
@pytest.mark.parametrize("model,setter,arg", CASES)
def test_a_setter_drops_what_was_derived(handles, model, setter, arg, name):
    """psba_linearize, then the setter: psba_schur_assemble asks for a new psba_linearize, and the per-observation
    blocks, the damping diagonal (free models) and the covariance (fixed K) are gone"""
    from psba_amd import capi
    h, _ = handles(model)
    s, p = setters(model)[setter], problem(name)
    baseline(h, model, p)
    if arg == "real" and s.prep:
        s.prep(h, p)
    h.linearize(1.0, 1.0)
    mu = try_mu(h, model)
    if model == "fixed":
        assert h.covariance(mu) == capi.PSBA_OK
        h.camera_covariance()
    else:
        h.free_obs_blocks()
        h.get_damping_diag()
    s.call[arg](h, p)
    refused(lambda: h.schur_assemble(mu), -6, "psba_linearize")
    if model == "fixed":
        refused(h.camera_covariance, -6)
    else:
        refused(h.free_obs_blocks, -6)
        refused(h.get_damping_diag, -6)


@pytest.mark.parametrize("model,setter,arg", IN_FLIGHT)
def test_a_setter_is_refused_while_a_try_is_in_flight(handles, model, setter, arg):
    """between psba_backsub_async and psba_backsub_wait every setter but psba_set_params / psba_reset_params is
    refused, and the setting is what it was"""
    h, _ = handles(model)
    s, p = setters(model)[setter], problem("P7")
    baseline(h, model, p)
    before = s.getter(h)
    queue_try(h, model)
    refused(lambda: s.call[arg](h, p), -6, "in flight")
    assert h.backsub_wait().status == 0
    assert s.getter(h) == before


@pytest.mark.parametrize("ahead", [False, True])
@pytest.mark.parametrize("setter", ["set_params", "reset_params"])
@pytest.mark.parametrize("model", list(NAMES))
def test_moving_the_parameters_gives_up_a_try_in_flight(handles, model, setter, ahead):
    """psba_set_params and psba_reset_params are taken between psba_backsub_async and psba_backsub_wait, with or without
    a linearization queued ahead: nothing of the try is left to wait for or to accept, and the next try runs"""
    h, _ = handles(model)
    p = problem("P7")
    baseline(h, model, p)
    queue_try(h, model, ahead)
    setters(model)[setter].call["noop"](h, p)
    refused(h.backsub_wait, -6, "psba_backsub_async")
    refused(h.accept, -6, "psba_backsub")
    refused(lambda: h.schur_assemble(1e-3), -6, "psba_linearize")
    queue_try(h, model)
    assert h.backsub_wait().status == 0


@pytest.mark.parametrize("model,setter,arg", AHEAD)
def test_a_setter_discards_the_linearization_queued_ahead(handles, model, setter, arg):
    """a try with psba_linearize_ahead, psba_backsub_wait, the setter, psba_accept and psba_linearize: the blocks and
    the damping diagonal are bit for bit those of a handle given the same setting and the same parameters before its
    first psba_linearize.  (A verb that moves the parameters drops the try's result too: psba_accept refuses.)  With
    the groups set after the try the step must leave the intrinsics alone, or the members end up different and no
    fresh handle takes those parameters: that case runs with every intrinsic masked."""
    h, h2 = handles(model)
    s, p = setters(model)[setter], problem("P7")
    mask = NONE10 if (setter, arg) == ("set_intrinsics_groups", "real") else BAL
    baseline(h, model, p, mask)
    if arg == "real" and s.prep:
        s.prep(h, p)
    start = params_bytes(h)
    queue_try(h, model, ahead=True)
    sc = h.backsub_wait()
    assert sc.status == 0 and sc.dp_l2 > 0.0
    s.call[arg](h, p)
    if s.moves_params:
        refused(h.accept, -6, "psba_backsub")
    else:
        h.accept()
        assert params_bytes(h) != start
    h.linearize(1.0, 1.0)
    got = h.free_obs_blocks() + (h.get_damping_diag(),)
    cams, pts = h.get_params(0)
    baseline(h2, model, p, mask)
    s.call[arg](h2, p)
    h2.set_params(cams, pts)
    h2.linearize(1.0, 1.0)
    want = h2.free_obs_blocks() + (h2.get_damping_diag(),)
    for a, b, what in zip(got, want, ("W", "B", "e", "D")):
        assert np.array_equal(a, b), what
