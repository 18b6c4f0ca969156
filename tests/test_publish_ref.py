"""The host half of the try-scalar handshake (psba_amd/csrc/scal_publish.h) without a GPU: the library's
check word and its take (psba_scal_block_check, psba_scal_block_take -- the function psba_backsub_wait applies to the
pinned block) against the independent statement in publish_ref.py.  Every comparison is on bit patterns.

The cases are built by publish_ref from a check function, so that a whole protocol -- writer and reader sharing one
check -- is judged by them: with the right check every verdict below is the expected one, and each of four wrong
checks (a plain XOR, the stamp left out, the last word left out, floating-point equality in place of bits) gets at
least one of them wrong."""
import numpy as np
import pytest

import publish_ref as pr

OLD_STAMP, NEW_STAMP = 6.0, 7.0


def cases(fault=None):
    """[(name, raw words, wanted stamp, accept?)] under the check `fault` selects"""
    out = []

    def add(name, words, stamp, chk, want, accept):
        raw = np.empty(pr.RAW, dtype=np.uint64)
        raw[:pr.WORDS] = words
        raw[pr.STAMP] = pr.bits(stamp)
        raw[pr.CHECK] = np.uint64(chk)
        out.append((name, raw, want, accept))

    def ck(words, stamp):
        return pr.check(words, stamp, fault)

    # complete blocks
    for name, blk in pr.edge_blocks().items():
        for stamp in (1.0, NEW_STAMP, 265000.0):
            add(f"complete {name} stamp {stamp}", blk, stamp, ck(blk, stamp), stamp, True)
    old, new = pr.two_blocks()
    add("complete old", old, OLD_STAMP, ck(old, OLD_STAMP), OLD_STAMP, True)
    add("complete new", new, NEW_STAMP, ck(new, NEW_STAMP), NEW_STAMP, True)
    # the captured situation and its relatives
    add("captured: new stamp and check over the old words", old, NEW_STAMP, ck(new, NEW_STAMP), NEW_STAMP, False)
    add("new stamp, old check, old words", old, NEW_STAMP, ck(old, OLD_STAMP), NEW_STAMP, False)
    add("new stamp, old check, new words", new, NEW_STAMP, ck(old, OLD_STAMP), NEW_STAMP, False)
    add("old stamp, new words and check", new, OLD_STAMP, ck(new, NEW_STAMP), NEW_STAMP, False)
    add("the previous publish, complete, when the next is wanted", old, OLD_STAMP, ck(old, OLD_STAMP), NEW_STAMP, False)
    # mixed blocks
    good = ck(new, NEW_STAMP)
    for k in range(pr.WORDS):
        mixed = new.copy()
        mixed[k] = old[k]
        add(f"one stale word, {k}", mixed, NEW_STAMP, good, NEW_STAMP, False)
    for k in range(1, pr.WORDS):
        mixed = new.copy()
        mixed[:k] = old[:k]
        add(f"stale prefix of {k}", mixed, NEW_STAMP, good, NEW_STAMP, False)
        mixed = new.copy()
        mixed[k:] = old[k:]
        add(f"stale suffix from {k}", mixed, NEW_STAMP, good, NEW_STAMP, False)
    for i, j in ((0, 1), (16, 20), (3, 103)):
        mixed = new.copy()
        mixed[i] ^= np.uint64(0x0000FFFF00000001)
        mixed[j] ^= np.uint64(0x0000FFFF00000001)
        add(f"words {i} and {j} stale by the same XOR mask", mixed, NEW_STAMP, good, NEW_STAMP, False)
    mixed = new.copy()
    mixed[[5, 9]] = mixed[[9, 5]]
    add("two words exchanged", mixed, NEW_STAMP, good, NEW_STAMP, False)
    for k in (2, 16, 103):
        z = new.copy()
        z[k] = np.uint64(0)                       # +0.0
        mz = z.copy()
        mz[k] = np.uint64(1 << 63)                # -0.0
        add(f"-0.0 for +0.0 in word {k}", mz, NEW_STAMP, ck(z, NEW_STAMP), NEW_STAMP, False)
        n1 = new.copy()
        n1[k] = np.uint64(0x7FF8000000000001)
        n2 = n1.copy()
        n2[k] = np.uint64(0x7FF8000000000002)
        add(f"another NaN payload in word {k}", n2, NEW_STAMP, ck(n1, NEW_STAMP), NEW_STAMP, False)
    return out


@pytest.fixture(scope="module")
def right_cases():
    return cases()


def test_reference_gives_the_expected_verdicts(right_cases):
    """the independent statement itself: complete blocks accepted, every stale or mixed block refused"""
    assert len(right_cases) > 300
    for name, raw, want, accept in right_cases:
        ok, copy = pr.take(raw, want)
        assert ok == accept, name
        assert np.array_equal(copy, raw), name


def test_library_take_gives_the_expected_verdicts(right_cases):
    """psba_scal_block_take on the same words: the same verdicts, and out holds the bits of the input block"""
    from psba_amd import capi
    for name, raw, want, accept in right_cases:
        ok, blk = capi.scal_block_take(raw, want)
        assert ok == accept, name
        assert np.array_equal(blk, raw[:pr.WORDS]), name


def test_library_check_word_is_the_reference_s(right_cases):
    """psba_scal_block_check against publish_ref.check on every block of the cases and on 1000 random bit patterns"""
    from psba_amd import capi
    for name, raw, _, _ in right_cases:
        stamp = pr.doubles(raw[pr.STAMP:pr.STAMP + 1])[0]
        assert int(capi.scal_block_check(raw[:pr.WORDS], stamp)) == pr.check(raw[:pr.WORDS], raw[pr.STAMP]), name
    rng = np.random.default_rng(1000)
    for k in range(1000):
        blk = rng.integers(0, 1 << 63, pr.WORDS, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, pr.WORDS, dtype=np.uint64)
        stamp = float(rng.integers(1, 1 << 40))
        want = pr.check(blk, stamp)
        assert int(capi.scal_block_check(blk, stamp)) == want, k
        raw = pr.make_raw(blk, stamp)
        assert int(raw[pr.CHECK]) == want
        ok, out = capi.scal_block_take(raw, stamp)
        assert ok and np.array_equal(out, blk), k


def test_take_refuses_every_single_bit_of_the_check_and_the_stamp():
    """a complete block with one bit of its check word or of its stamp flipped is refused (64 + 64 readings)"""
    from psba_amd import capi
    _, new = pr.two_blocks()
    raw = pr.make_raw(new, NEW_STAMP)
    assert capi.scal_block_take(raw, NEW_STAMP)[0]
    for word in (pr.STAMP, pr.CHECK):
        for b in range(64):
            bad = raw.copy()
            bad[word] ^= np.uint64(1 << b)
            assert not capi.scal_block_take(bad, NEW_STAMP)[0], (word, b)
            assert not pr.take(bad, NEW_STAMP)[0], (word, b)


@pytest.mark.parametrize("fault", ["xor", "no-stamp", "no-last", "float-eq"])
def test_injected_faults_fail_the_cases(fault, right_cases):
    """a protocol built on a wrong check gets verdicts wrong, and its check word is not the library's"""
    from psba_amd import capi
    wrong = [name for name, raw, want, accept in cases(fault) if pr.take(raw, want, fault)[0] != accept]
    print(f"{fault}: {len(wrong)} wrong verdicts, first: {wrong[:3]}")
    assert wrong, f"{fault} passed every case"
    differ = 0
    for name, raw, _, _ in right_cases[:40]:
        stamp = pr.doubles(raw[pr.STAMP:pr.STAMP + 1])[0]
        differ += int(capi.scal_block_check(raw[:pr.WORDS], stamp)) != pr.check(raw[:pr.WORDS], raw[pr.STAMP], fault)
    assert differ, f"{fault} has the library's check word"
