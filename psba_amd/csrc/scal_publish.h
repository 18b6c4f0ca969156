// scal_publish.h -- how a try's scalar block travels from the device to pinned host memory, stated once for the
// kernels that write it and the host that reads it (psba_backsub_wait).
//
// The pinned block is PUB_RAW = 106 words of 64 bits:
//   words 0 .. 103   the device scalar block (NSCAL doubles), bit for bit
//   word 104         the stamp: the double the host waits for (psba_ctx::pub_seq), as its bit pattern
//   word 105         the check word over words 0 .. 104
//
// The check word, in unsigned 64-bit arithmetic (every sum and product modulo 2^64) on BIT PATTERNS -- a NaN's
// payload, the sign of a zero and a denormal count like any other bits; no floating-point operation touches a word:
//
//   mix(pos, w):  z = w + (pos + 1) * 0x9E3779B97F4A7C15
//                 z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//                 z = (z ^ (z >> 27)) * 0x94D049BB133111EB
//                 mix = z ^ (z >> 31)
//   check = mix(0, word 0) + mix(1, word 1) + ... + mix(103, word 103) + mix(104, stamp)
//
// (the finalizer of splitmix64 behind a per-position offset).  For a fixed position mix is a bijection of the word,
// so a block with exactly one wrong word -- or the right words under another stamp -- never has the right check; a
// block with several wrong words has it with probability 2^-64.  The offset makes the sum depend on where a word
// stands: two words that are stale by the same XOR difference, or two words exchanged, do not cancel as they would
// under a plain XOR of the words.  The terms are independent, so the device forms them one per lane and adds them
// with a wave reduction; a sum modulo 2^64 does not depend on the order.
//
// The protocol: the device writes words 0 .. 103, then (behind a system-scope fence and a barrier) the stamp and the
// check.  The host copies all 106 words into memory of its own and accepts the COPY iff its stamp is the wanted one and
// its check word is the check of its words 0 .. 104.  That needs no order between the device's writes as the host
// sees them: only that an aligned 8-byte word arrives whole, and that every word has arrived by the stream's end.  A
// copy with the wanted stamp and another check is a torn reading (the stamp overtook the block): the host
// reads again.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

namespace psba {

constexpr int PUB_WORDS = 104;           // = NSCAL (psba_internal.h asserts it)
constexpr int PUB_STAMP = PUB_WORDS;     // word of the stamp
constexpr int PUB_CHECK = PUB_WORDS + 1; // word of the check
constexpr int PUB_RAW = PUB_WORDS + 2;

__host__ __device__ inline unsigned long long pub_mix(int pos, unsigned long long w) {
  unsigned long long z = w + (unsigned long long)(pos + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

inline unsigned long long pub_bits(double v) {
  unsigned long long b;
  memcpy(&b, &v, sizeof b);
  return b;
}

// host: the check word of a block of PUB_WORDS words under a stamp
inline unsigned long long pub_check(const unsigned long long *words, unsigned long long stamp) {
  unsigned long long c = pub_mix(PUB_STAMP, stamp);
  for (int t = 0; t < PUB_WORDS; t++) c += pub_mix(t, words[t]);
  return c;
}

// host: take a block.  Copies the PUB_RAW words at raw (pinned memory the device may be writing: one 8-byte load per
// word) to out, and accepts the copy iff it carries the wanted stamp and its own check.  *stamped (may be null): the
// copy carried the wanted stamp, so a refusal is a torn reading.
inline bool pub_take(const volatile unsigned long long *raw, unsigned long long want_stamp, unsigned long long *out,
                     bool *stamped = nullptr) {
  for (int t = 0; t < PUB_RAW; t++) out[t] = raw[t];
  const bool st = out[PUB_STAMP] == want_stamp;
  if (stamped) *stamped = st;
  return st && out[PUB_CHECK] == pub_check(out, out[PUB_STAMP]);
}

#if defined(__HIPCC__)
// device: the whole prologue of a workgroup that publishes, called by every thread of a one-dimensional workgroup of
// 64, 128 or 256 threads (any multiple of 64).  Wave 0 copies src[0 .. PUB_WORDS) to dst and forms the check (two words
// per lane, one wave reduction; no LDS, so the callers' LDS budgets stand); behind the fence and the barrier thread 0
// writes the stamp and the check.  Words move as doubles through loads and stores only, which keep every bit.
__device__ __forceinline__ void scal_publish(const double *src, double *dst, double stamp) {
  unsigned long long acc = 0;
  if (threadIdx.x < 64) {
    for (int t = threadIdx.x; t <= PUB_WORDS; t += 64) {
      double w = stamp;
      if (t < PUB_WORDS) {
        w = src[t];
        dst[t] = w;
      }
      acc += pub_mix(t, (unsigned long long)__double_as_longlong(w));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    dst[PUB_STAMP] = stamp;
    dst[PUB_CHECK] = __longlong_as_double((long long)acc);
  }
}
#endif

}  // namespace psba
