// desc_canon.h — the super-k-mer descriptor's bit layout and its strand-canonical form.
//
// A descriptor carries the L = n + E - 1 bases of a super-k-mer (n edges of E symbols):
//   w0: bases [0,32); w1: bases [32,54) in bits 0..43 | n edges (6 bits) at 44 | 14 hash bits at 50
// with the bases past the last edge zeroed. The minimizer, and with it n and the hash bits, is
// the same on both strands, and every consumer canonicalises each edge it takes out of a
// descriptor, so a descriptor and its reverse complement stand for the same canonical edges:
// desc_canonical keeps the smaller of the two base strings, and the two collapse into one.
//
// Self-contained (no HIP header needed), so a plain host compiler can build it alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCAAT_DESC_HD __host__ __device__ __forceinline__
#else
#define MCAAT_DESC_HD inline
#endif

namespace mcaat {

constexpr int kDescBases = 54;
constexpr int kNShift = 44;
constexpr int kHShift = 50;
constexpr int kHBits = 14;

// A canonical descriptor never has w0 == ~0 (the tables' empty marker): an all-T first word
// needs L >= 32, and then the last 32 bases of the reverse complement are all A; for L < 64
// those overlap its first 32 bases, so its first word holds an A, is smaller, and is the one
// kept.
static_assert(kDescBases < 64, "a canonical descriptor's w0 is never all ones only while L < 64");

// A descriptor is live when it holds at least one edge; padding and zero-filled slots have n = 0.
MCAAT_DESC_HD bool desc_live(uint64_t w1) { return ((w1 >> kNShift) & 63) != 0; }

// The fine sub-partition of a descriptor inside its L1 bucket: the top l2_bits of the hash bits,
// which are the top bits of w1 (0 <= l2_bits <= kHBits; no bits: sub 0).
static_assert(kHShift + kHBits == 64, "the hash bits end at the top of w1");
MCAAT_DESC_HD uint32_t desc_sub(uint64_t w1, int l2_bits) {
    return l2_bits > 0 ? (uint32_t)(w1 >> (64 - l2_bits)) : 0u;
}

// reverse the 2-bit groups of a word: the hardware bit reverse plus one swap of adjacent bits
#if defined(__has_builtin)
#if __has_builtin(__builtin_bitreverse32)
#define MCAAT_DESC_BITREV 1
#endif
#endif
MCAAT_DESC_HD uint32_t desc_rev2_32(uint32_t x) {
#ifdef MCAAT_DESC_BITREV
    const uint32_t y = __builtin_bitreverse32(x);
    return ((y >> 1) & 0x55555555u) | ((y << 1) & 0xAAAAAAAAu);
#else
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}
// per 32-bit half, as rev2_dev in node_counter.hip
MCAAT_DESC_HD uint64_t desc_rev2_64(uint64_t x) {
    return ((uint64_t)desc_rev2_32((uint32_t)x) << 32) | desc_rev2_32((uint32_t)(x >> 32));
}

// The descriptor with its base string in canonical orientation: the smaller w0 wins, on equal
// w0 the smaller base bits of w1 (a palindrome keeps either). n and the hash bits pass through;
// a padding descriptor (n = 0) passes through unchanged. Needs n + E - 1 <= kDescBases.
MCAAT_DESC_HD void desc_canonical(uint64_t &w0, uint64_t &w1, int E) {
    constexpr uint64_t kBase1 = (1ULL << kNShift) - 1;  // base bits of w1
    const int n = (int)((w1 >> kNShift) & 63);
    const int L = n + E - 1;
    const uint64_t b1 = w1 & kBase1;
    // the 64-base field reversed and complemented: base j at base 63 - j; then base L-1 comes
    // down to base 0, which drops the complemented padding and leaves zeros above 2L
    const uint64_t hi = ~desc_rev2_64(w0), lo = ~desc_rev2_64(b1);
    const int s = 2 * (64 - L);  // 20 .. 126 for L in 1 .. kDescBases
    uint64_t r0, r1;
    if (s >= 64) {
        r0 = hi >> (s - 64);
        r1 = 0;
    } else {
        r0 = (lo >> s) | (hi << (64 - s));
        r1 = hi >> s;
    }
    const bool take = n != 0 && (r0 < w0 || (r0 == w0 && r1 < b1));
    if (take) {
        w0 = r0;
        w1 = (w1 & ~kBase1) | r1;
    }
}

}  // namespace mcaat
