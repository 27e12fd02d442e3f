// Stand-alone sweep of desc_live and desc_sub (mcaat_amd/csrc/desc_canon.h, that header only)
// against a bit-string model: w1 written out as 64 characters, n read from characters 44..49 and
// the sub from the top l2_bits characters. Built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_dead_slots.py; prints "desc_sub ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../mcaat_amd/csrc/desc_canon.h"

using mcaat::kHBits;
using mcaat::kHShift;
using mcaat::kNShift;

static uint64_t rng_state = 0xD1B54A32D192ED03ULL;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

// character j of the string is bit j of w1
static std::string bits(uint64_t w1) {
    std::string s(64, '0');
    for (int j = 0; j < 64; ++j)
        if ((w1 >> j) & 1) s[j] = '1';
    return s;
}
static uint32_t value(const std::string &s, int lo, int n) {  // characters [lo, lo + n), lowest first
    uint32_t v = 0;
    for (int j = n; j-- > 0;) v = 2 * v + (uint32_t)(s[lo + j] == '1');
    return v;
}

static long n_checked = 0;
static void check(uint64_t w1) {
    const std::string s = bits(w1);
    const bool live = value(s, kNShift, 6) != 0;
    if (mcaat::desc_live(w1) != live) {
        fprintf(stderr, "desc_sub: live differs (w1=%016llx)\n", (unsigned long long)w1);
        exit(1);
    }
    for (int l2 = 0; l2 <= kHBits; ++l2) {
        const uint32_t want = l2 ? value(s, 64 - l2, l2) : 0u;
        if (mcaat::desc_sub(w1, l2) != want || want >= (1u << l2)) {
            fprintf(stderr, "desc_sub: sub differs (w1=%016llx, l2_bits=%d)\n", (unsigned long long)w1, l2);
            exit(1);
        }
    }
    ++n_checked;
}

int main() {
    const uint64_t base_mask = (1ULL << kNShift) - 1, all_hash = ((1ULL << kHBits) - 1) << kHShift;
    const uint64_t ns[] = {0, 1, 27, 39, 63};
    for (uint64_t n : ns) {
        check(n << kNShift);                          // no hash bit, no base
        check((n << kNShift) | all_hash);             // all-ones hash bits
        check((n << kNShift) | all_hash | base_mask);
        check((n << kNShift) | base_mask);            // every base bit below n: none may leak into it
        for (int h = 0; h < kHBits; ++h) check((n << kNShift) | (1ULL << (kHShift + h)));
        for (int rep = 0; rep < 2000; ++rep) check((rnd() & ~(63ULL << kNShift)) | (n << kNShift));
    }
    for (int rep = 0; rep < 20000; ++rep) check(rnd());
    check(0);
    check(~0ULL);
    printf("desc_sub ok: %ld words\n", n_checked);
    return 0;
}
