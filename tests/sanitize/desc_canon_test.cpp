// Stand-alone sweep of desc_canonical (mcaat_amd/csrc/desc_canon.h, that header only) against a
// plain string model: reverse, complement, pack. Built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_desc_canonical.py; prints "desc_canon ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "../../mcaat_amd/csrc/desc_canon.h"

using mcaat::kDescBases;
using mcaat::kHShift;
using mcaat::kNShift;

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

static std::string rc(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}
// base j at bits 2j of the 108-bit field: {w0, base bits of w1}
static std::pair<uint64_t, uint64_t> pack(const std::string &s) {
    uint64_t w[2] = {0, 0};
    for (size_t j = 0; j < s.size(); ++j) {
        const uint64_t c = s[j] == 'A' ? 0 : s[j] == 'C' ? 1 : s[j] == 'G' ? 2 : 3;
        w[j >> 5] |= c << (2 * (j & 31));
    }
    return {w[0], w[1]};
}

static long n_checked = 0;
static void fail(const char *what, const std::string &s, int E) {
    fprintf(stderr, "desc_canon: %s (E=%d, s=%s)\n", what, E, s.c_str());
    exit(1);
}

static std::pair<uint64_t, uint64_t> canon(const std::string &s, int n, uint64_t hash, int E) {
    const auto p = pack(s);
    uint64_t w0 = p.first, w1 = p.second | ((uint64_t)n << kNShift) | (hash << kHShift);
    mcaat::desc_canonical(w0, w1, E);
    if ((w1 >> kNShift) != (((uint64_t)n) | (hash << (kHShift - kNShift)))) fail("n or hash bits changed", s, E);
    return {w0, w1 & ((1ULL << kNShift) - 1)};
}

static void check(const std::string &s, int E) {
    const int L = (int)s.size(), n = L - E + 1;
    const uint64_t hash = rnd() & 0x3FFF;
    const auto f = pack(s), r = pack(rc(s));
    const auto want = r < f ? r : f;  // smaller w0, then smaller base bits of w1
    const auto got = canon(s, n, hash, E), got_rc = canon(rc(s), n, hash, E);
    if (got != f && got != r) fail("neither the input nor its reverse complement", s, E);
    if (got != want) fail("not the smaller orientation", s, E);
    if (got != got_rc) fail("canon(s) != canon(rc(s))", s, E);
    if (got.first == ~0ULL) fail("w0 is all ones", s, E);
    if (L < 32 ? (got.first >> (2 * L)) != 0 || got.second != 0 : L < 64 && (got.second >> (2 * (L - 32))) != 0)
        fail("bits above 2L set", s, E);
    ++n_checked;
}

int main() {
    const int Es[] = {16, 24, 28, 31};
    for (int E : Es) {
        for (int n = 1; n <= kDescBases - E + 1; ++n) {
            const int L = n + E - 1;  // covers L = 32, 33 and 54 for every E here
            for (int rep = 0; rep < 24; ++rep) {
                std::string s(L, 'A');
                for (char &c : s) c = "ACGT"[rnd() & 3];
                check(s, E);
                if (rep < 4) {  // long single-base runs at either end
                    const int run = 1 + (int)(rnd() % L);
                    std::string t = s;
                    for (int j = 0; j < run; ++j) t[rep & 1 ? L - 1 - j : j] = rep & 2 ? 'T' : 'A';
                    check(t, E);
                }
            }
            check(std::string(L, 'T'), E);
            check(std::string(L, 'A'), E);
            if (L % 2 == 0) {  // equal to its own reverse complement
                std::string h(L / 2, 'A');
                for (char &c : h) c = "ACGT"[rnd() & 3];
                check(h + rc(h), E);
            }
        }
        // padding passes through, whatever its other bits
        uint64_t w0 = 0, w1 = 0;
        mcaat::desc_canonical(w0, w1, E);
        if (w0 != 0 || w1 != 0) fail("n = 0 changed", "", E);
        w0 = rnd(), w1 = (rnd() & ((1ULL << kNShift) - 1)) | (rnd() << kHShift);
        const uint64_t a0 = w0, a1 = w1;
        mcaat::desc_canonical(w0, w1, E);
        if (w0 != a0 || w1 != a1) fail("n = 0 changed", "", E);
    }
    printf("desc_canon ok: %ld strings\n", n_checked);
    return 0;
}
