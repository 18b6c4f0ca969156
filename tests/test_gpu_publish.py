"""The try-scalar handshake on the GPU (psba_amd/csrc/scal_publish.h), in two halves that need no timing:

  * the device half: psba_test_publish runs the publishing prologue alone, in workgroups of 64, 128 and 256 threads, on
    the edge blocks of test_publish_ref.py; the pinned words are the input bit for bit, the stamp is the next one, the
    check word is publish_ref's (stated independently, in numpy uint64) and the host's take accepts it;
  * the carried route: one damping try with backsub_async, linearize_ahead, backsub_wait on each kernel that carries
    the block (k_linearize2, k_linearize under PSBA_LIN_V1=1, k_free_linearize on blocks of 11 and 16, the lean form
    through psba_levmar); what backsub_wait returns is, bit for bit, the sum of the device's own block (fetched after
    the stream's end) over the partial sets 0 .. 15, and psba_publish_stats counts one take per carried try.  A failed
    factorization (NaN sums) and a NaN step come back the same way.  The event routes (PSBA_SCAL_KERNEL=1,
    PSBA_SCAL_MEMCPY=1) return the same and take nothing.

A NaN sum is compared as a NaN and not by its payload: when both operands of an addition are NaN the hardware returns
the payload of one of them, and which operand of a commutative addition comes first is the compiler's choice, in the
library and in numpy alike.  Needs an MI355X."""
import numpy as np
import pytest

import publish_ref as pr
from test_freekd_twin import P7

pytestmark = pytest.mark.gpu

E_STATE = -6
NOT_SPD = 1


def same_bits(got, want, label):
    """doubles equal bit for bit; NaN for NaN (module docstring)"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{label}: {got} / {want}"
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)), f"{label}: {got} / {want}"


def check_raw(raw, stamp, label):
    """raw pinned words: stamp, the reference's check word, accepted by the library's take and by the reference's"""
    from psba_amd import capi
    assert raw[pr.STAMP] == pr.bits(stamp), f"{label}: stamp {pr.doubles(raw[pr.STAMP:pr.STAMP + 1])[0]} for {stamp}"
    assert int(raw[pr.CHECK]) == pr.check(raw[:pr.WORDS], raw[pr.STAMP]), f"{label}: check word"
    ok, blk = capi.scal_block_take(raw, stamp)
    assert ok and np.array_equal(blk, raw[:pr.WORDS]), f"{label}: the host's take"
    assert pr.take(raw, stamp)[0] and not pr.take(raw, stamp + 1.0)[0], label


# ---- the device half -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threads", [64, 128, 256])
def test_device_prologue_against_the_independent_statement(threads):
    import psba_amd
    h = psba_amd.Psba(0)
    try:
        stamp = 0.0
        dev0 = h.test_publish(None, threads)          # the fresh handle's own block: zeros, under stamp 1
        stamp += 1.0
        check_raw(dev0, stamp, "the fresh block")
        assert not dev0[:pr.WORDS].any()
        prev = None
        for name, blk in pr.edge_blocks().items():
            raw = h.test_publish(blk, threads)
            stamp += 1.0
            assert np.array_equal(raw[:pr.WORDS], blk), f"{name}: the block's bits"
            check_raw(raw, stamp, name)
            if prev is not None:                      # nothing of the block published before is left behind
                differs = prev != blk
                assert np.all(raw[:pr.WORDS][differs] != prev[differs]), name
            prev = blk
        old, new = pr.two_blocks()                    # two blocks that differ in every word, one behind the other
        h.test_publish(old, threads)
        raw = h.test_publish(new, threads)
        stamp += 2.0
        assert np.all(raw[:pr.WORDS] != old) and np.array_equal(raw[:pr.WORDS], new)
        check_raw(raw, stamp, "new behind old")
        # a given block stood in for the launch only: the device's own block is back
        again = h.test_publish(None, threads)
        stamp += 1.0
        check_raw(again, stamp, "the device's block again")
        assert np.array_equal(again[:pr.WORDS], dev0[:pr.WORDS])
        assert h.publish_stats() == (0, 0)            # no try was carried
        with pytest.raises(psba_amd.PsbaError) as e:
            h.test_publish(None, 96)
        assert e.value.code == -1
    finally:
        h.close()


# ---- the carried route -----------------------------------------------------------------------------------------------

def open_route(route, problems):
    import psba_amd
    h = psba_amd.Psba(0)
    if route in ("free11", "free16"):
        from freekd_twin import start_kc
        p = P7()
        h.set_camera_model(psba_amd.CAMERA_FREE_KD if route == "free16" else psba_amd.CAMERA_FREE_K)
        h.upload_problem(p)
        if route == "free16":
            h.set_distortion(start_kc(p["nC"]))
        assert h.camera_block() == (16 if route == "free16" else 11) and h.schur_path() == 5
    else:
        h.upload_problem(problems["7cams"])
        assert h.camera_block() == 6
    return h


def carried_try(h, kind, carried=True):
    """one try through backsub_async, linearize_ahead, backsub_wait; the device's block after the stream's end"""
    cost0 = h.residual()
    h.linearize(1.0, 1.0)
    mu = -1e30 if kind == "not-spd" else 1e-3 * h.max_diag()
    h.schur_assemble(mu)
    h.schur_reduce()
    h.schur_solve()
    if kind == "nan-step":
        dp = h.get_dp()
        dp[:h.nA:7] = np.nan
        h.set_step(dp)
    takes, torn = h.publish_stats()
    h.backsub_async(mu)
    h.linearize_ahead()
    sc = h.backsub_wait()                              # (raises on "the try's scalars did not reach the host")
    t1 = h.publish_stats()
    assert t1[0] == takes + (1 if carried else 0) and t1[1] >= torn and t1[1] - torn <= 1
    raw = h.test_publish(None, 128)                    # waits for the stream; the device's own block
    assert int(raw[pr.CHECK]) == pr.check(raw[:pr.WORDS], raw[pr.STAMP])
    status, sums = pr.try_sums(raw[:pr.WORDS])
    got = np.array([sc.dp_l2, sc.gain_den, sc.new_cost, sc.newp_l2])
    print(f"{kind}: status {sc.status} sums {got} torn {t1[1] - torn}")
    assert sc.status == status
    same_bits(got, sums, kind)
    if kind == "plain":
        assert sc.status == 0 and np.all(np.isfinite(got)) and sc.new_cost < cost0
    elif kind == "not-spd":
        assert sc.status & NOT_SPD
    else:
        assert not (sc.status & NOT_SPD) and not (sc.new_cost < cost0)
    return sc


# (psba_set_step, which injects the NaN step, exists for six-parameter blocks only)
@pytest.mark.parametrize("route,kind", [(r, k) for r in ("lin2", "lin-v1", "free11", "free16")
                                        for k in ("plain", "not-spd", "nan-step") if k != "nan-step" or r.startswith("lin")])
def test_carried_try_returns_the_device_s_block(route, kind, problems, monkeypatch):
    import psba_amd
    if route == "lin-v1":
        monkeypatch.setenv("PSBA_LIN_V1", "1")
    h = open_route(route, problems)
    try:
        carried_try(h, kind)
        # the hook dropped the try's result, and the next try is carried like the first
        with pytest.raises(psba_amd.PsbaError) as e:
            h.accept()
        assert e.value.code == E_STATE
        carried_try(h, "plain")
    finally:
        h.close()


@pytest.mark.parametrize("env", ["PSBA_SCAL_KERNEL", "PSBA_SCAL_MEMCPY"])
@pytest.mark.parametrize("route", ["lin2", "free16"])
def test_event_routes_return_the_same_and_take_nothing(route, env, problems, monkeypatch):
    monkeypatch.setenv(env, "1")
    h = open_route(route, problems)
    try:
        for kind in ("plain", "not-spd"):
            carried_try(h, kind, carried=False)
        assert h.publish_stats() == (0, 0)
    finally:
        h.close()


def test_the_event_kernel_writes_the_same_format(problems, monkeypatch):
    """PSBA_SCAL_KERNEL=1: k_publish_scal is the shared prologue, so the pinned words behind a try carry the next stamp
    and the reference's check word; the hook's publish behind it carries the stamp after that"""
    monkeypatch.setenv("PSBA_SCAL_KERNEL", "1")
    h = open_route("lin2", problems)
    try:
        first = h.test_publish(None, 64)
        check_raw(first, 1.0, "the hook")
        carried_try(h, "plain", carried=False)        # the try's kernel took stamp 2, the hook inside carried_try 3
        check_raw(h.test_publish(None, 256), 4.0, "the hook behind the event kernel")
    finally:
        h.close()


def test_levmar_takes_one_block_per_look_ahead(problems):
    """psba_levmar (the lean look-ahead where the handle allows it): takes grows by the tries that queued a
    look-ahead, which is every try but those of the last iteration allowed"""
    import psba_amd
    for name, lean in (("7cams", None), ("54cams", True)):
        h = psba_amd.Psba(0)
        try:
            h.upload_problem(problems[name])
            max_iter = 4
            res, log = h.levmar(max_iter=max_iter, tr_handoff=False)
            assert res.iters == max_iter and res.n_log == res.tries   # no early end: every try wrote its row
            last = int(np.sum(log[:, 0] == max_iter - 1))
            takes, torn = h.publish_stats()
            print(f"{name}: tries {res.tries}, in the last iteration {last}, takes {takes}, torn {torn}, lean {h.lm_ran_lean()}")
            assert last >= 1 and takes == res.tries - last and 0 <= torn <= takes
            if lean is not None:
                assert h.lm_ran_lean() == lean
        finally:
            h.close()


# ---- state -----------------------------------------------------------------------------------------------------------

def test_the_hook_is_refused_while_a_try_is_in_flight(problems):
    import psba_amd
    h = open_route("lin2", problems)
    try:
        h.linearize(1.0, 1.0)
        mu = 1e-3 * h.max_diag()
        h.schur_assemble(mu)
        h.schur_reduce()
        h.schur_solve()
        h.backsub_async(mu)
        with pytest.raises(psba_amd.PsbaError) as e:
            h.test_publish(None, 128)
        assert e.value.code == E_STATE
        h.linearize_ahead()
        with pytest.raises(psba_amd.PsbaError) as e:
            h.test_publish(pr.edge_blocks()["ordinary"], 128)
        assert e.value.code == E_STATE
        sc = h.backsub_wait()                          # the refused calls changed nothing: the try is carried and taken
        assert sc.status == 0 and h.publish_stats()[0] == 1
        cost = sc.new_cost
        h.test_publish(pr.edge_blocks()["nan-payloads"], 128)
        with pytest.raises(psba_amd.PsbaError) as e:   # the try's result went with the hook
            h.accept()
        assert e.value.code == E_STATE
        # a new try from the same parameters: the same proposal, accepted this time
        h.linearize(1.0, 1.0)
        h.schur_assemble(mu)
        h.schur_reduce()
        h.schur_solve()
        h.backsub_async(mu)
        h.linearize_ahead()
        sc = h.backsub_wait()
        assert sc.status == 0 and abs(sc.new_cost - cost) <= 1e-12 * cost
        h.accept()
        assert abs(h.residual() - sc.new_cost) <= 1e-12 * cost
    finally:
        h.close()
