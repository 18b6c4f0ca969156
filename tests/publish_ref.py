"""The check word of the try's scalar block (psba_amd/csrc/scal_publish.h), stated a second time in numpy
uint64 from the header's comment -- nothing here calls the library.  The tests of both halves of the handshake compare
the library with this: test_publish_ref.py the host's take (no GPU), test_gpu_publish.py the device's prologue.

The pinned block is RAW = 106 words of 64 bits: words 0 .. 103 the device scalar block, word 104 the stamp, word 105
the check over words 0 .. 104:

    mix(pos, w):  z = w + (pos + 1) * 0x9E3779B97F4A7C15           (everything modulo 2^64, on bit patterns)
                  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
                  z = (z ^ (z >> 27)) * 0x94D049BB133111EB
                  mix = z ^ (z >> 31)
    check = sum over pos = 0 .. 104 of mix(pos, word pos)

and the host accepts a copy of the 106 words iff its stamp is the wanted one and its word 105 is the check of its
words 0 .. 104.

`fault` switches in a wrong variant of the check, for the tests that show that the cases can tell them apart:
"xor" a plain XOR of the words, "no-stamp" the stamp left out, "no-last" word 103 left out, "float-eq" words that count
as doubles do under ==, not as bits: -0.0 is +0.0 and a NaN is a NaN whatever its payload."""
import numpy as np

WORDS, STAMP, CHECK, RAW = 104, 104, 105, 106
SC_PART, SC_NPART, SC_STATUS_V, SC_STATUS_SPD = 16, 16, 80, 81   # slots of the block (psba_internal.h)
M64 = (1 << 64) - 1
GOLDEN, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def bits(x):
    """the bit patterns of doubles (or of words already) as uint64, copied"""
    a = np.array(x)
    if a.dtype != np.uint64:
        a = a.astype(np.float64).view(np.uint64)
    return a.copy()


def doubles(words):
    return np.ascontiguousarray(words, dtype=np.uint64).view(np.float64)


def mix(pos, w):
    z = (int(w) + (pos + 1) * GOLDEN) & M64
    z = ((z ^ (z >> 30)) * MUL1) & M64
    z = ((z ^ (z >> 27)) * MUL2) & M64
    return z ^ (z >> 31)


def check(words, stamp, fault=None):
    """check word (a Python int) of the 104 words `words` (uint64) under the stamp `stamp` (a double or a uint64)"""
    w = [int(v) for v in np.asarray(words, dtype=np.uint64).reshape(WORDS)]
    s = int(bits(stamp)) if not isinstance(stamp, (int, np.integer)) else int(stamp)
    if fault == "float-eq":
        d = doubles(np.array(w, dtype=np.uint64))
        w = [0x7FF8000000000000 if np.isnan(x) else 0 if x == 0.0 else v for v, x in zip(w, d)]
    if fault == "xor":
        c = s
        for v in w:
            c ^= v
        return c
    c = 0
    for pos, v in enumerate(w):
        if fault == "no-last" and pos == WORDS - 1:
            continue
        c = (c + mix(pos, v)) & M64
    if fault != "no-stamp":
        c = (c + mix(STAMP, s)) & M64
    return c


def make_raw(words, stamp, fault=None):
    """the 106 words a complete publish of `words` under `stamp` leaves in pinned memory"""
    raw = np.empty(RAW, dtype=np.uint64)
    raw[:WORDS] = np.asarray(words, dtype=np.uint64)
    raw[STAMP] = bits(stamp)
    raw[CHECK] = np.uint64(check(raw[:WORDS], raw[STAMP], fault))
    return raw


def take(raw, want_stamp, fault=None):
    """(accepted, copy) as the host decides it"""
    out = np.asarray(raw, dtype=np.uint64).copy()
    want = bits(want_stamp)
    c = np.uint64(check(out[:WORDS], out[STAMP], fault))
    return bool(out[STAMP] == want) and bool(out[CHECK] == c), out


def try_sums(words):
    """what psba_backsub_wait forms from an accepted block: the four sums over the partial sets 0 .. 15, in that order,
    starting from +0.0, and the status (bit 0 PSBA_NOT_SPD, bit 1 PSBA_SINGULAR_V)"""
    d = doubles(words)[:WORDS]
    sums = []
    with np.errstate(all="ignore"):
        for q in range(4):
            v = np.float64(0.0)
            for s in range(SC_NPART):
                v = v + d[SC_PART + 4 * s + q]
            sums.append(v)
    status = (1 if d[SC_STATUS_SPD] > 0.0 else 0) | (2 if d[SC_STATUS_V] > 0.0 else 0)
    return status, np.array(sums)


# ---- the blocks both test modules use --------------------------------------------------------------------------------

def edge_blocks():
    """name -> 104 words: ordinary sums, NaNs with different payloads, infinities / signed zeros / denormals, all-ones
    words, and a block whose partial sets are zero but for set 0 (small problems touch few sets)"""
    rng = np.random.default_rng(20240607)
    out = {}
    out["ordinary"] = bits(rng.standard_normal(WORDS) * 10.0 ** rng.integers(-8, 9, WORDS))
    nan = np.full(WORDS, 0x7FF8000000000000, dtype=np.uint64)
    nan |= rng.integers(1, 1 << 51, WORDS, dtype=np.uint64)
    nan[::3] |= np.uint64(1 << 63)               # negative quiet NaNs
    nan[1::5] &= np.uint64(~(1 << 51) & M64)     # signalling ones (payload non-zero: still NaN)
    out["nan-payloads"] = nan
    sp = np.empty(WORDS, dtype=np.uint64)
    pats = [0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0x0000000000000000,
            0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF]
    for t in range(WORDS):
        sp[t] = pats[t % len(pats)]
    out["inf-zero-denormal"] = sp
    out["all-ones"] = np.full(WORDS, M64, dtype=np.uint64)
    z = np.zeros(WORDS)
    z[0], z[7] = 1234.5678, 9.87e5
    z[SC_PART:SC_PART + 4] = [3.25e-3, 1.5e-2, 1229.125, 8.1e6]
    out["zero-sets"] = bits(z)
    out["all-zero"] = np.zeros(WORDS, dtype=np.uint64)
    return out


def two_blocks():
    """(old, new): two blocks that differ in every word"""
    rng = np.random.default_rng(77)
    old = rng.integers(0, 1 << 63, WORDS, dtype=np.uint64) * np.uint64(2)
    new = old ^ rng.integers(1, 1 << 63, WORDS, dtype=np.uint64)
    assert np.all(old != new)
    return old, new
