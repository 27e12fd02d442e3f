// The sharded build's key-range rule (mcaat_amd/csrc/splits.h: shard_hist_bits, choose_splits) for
// every k in 2..30 and every world in 1..64 on seeded histograms (all-zero, one non-zero bin at
// either end, sparse and dense random); built with the sanitizer flags of this directory
// (tests/test_sanitizers.py), so a shift by a negative or too large amount aborts: that is what this
// program is for. Beside it, structural checks of what the build relies on: world-1 splits,
// ascending, multiples of 16 (edges sharing key >> 4 stay on one rank), none above the key space,
// each a bin edge. The "weight" check (the prefix of bins is the first to reach its share) sums and
// divides in the same double arithmetic as choose_splits, so it catches a wrong index, not a
// rounding error: the independent, exact-integer restatement of the rule is in
// tests/test_sharded_k_sweep.py.
#include <cstdio>
#include <random>

#include "../../mcaat_amd/csrc/splits.h"

static int fail(const char *what, int k, int world, int h) {
    std::printf("FAIL %s: k %d world %d hist %d\n", what, k, world, h);
    return 1;
}

int main() {
    std::mt19937_64 rng(7);
    for (int k = 2; k <= 30; ++k) {
        const int bits = mcaat::shard_hist_bits(k), key_bits = 2 * (k + 1);
        if (bits < 1 || bits > 12) return fail("bits", k, 0, 0);
        const int nb = 1 << bits, shift = key_bits - bits;  // the rule itself shifts by it first
        for (int h = 0; h < 5; ++h) {
            std::vector<uint64_t> hist(nb, 0);
            if (h == 1) hist[0] = 1 + rng() % 1000;
            if (h == 2) hist[nb - 1] = 1 + rng() % 1000;
            if (h == 3)
                for (int i = 0; i < nb; ++i) hist[i] = rng() % 8 == 0 ? rng() % 100000 : 0;
            if (h == 4)
                for (int i = 0; i < nb; ++i) hist[i] = rng() % (1ULL << 40);
            std::vector<double> cum(nb);
            double acc = 0;
            for (int i = 0; i < nb; ++i) cum[i] = acc += (double)hist[i];
            for (int world = 1; world <= 64; ++world) {
                const std::vector<uint64_t> s = mcaat::choose_splits(hist, world, key_bits);
                if ((int)s.size() != world - 1) return fail("count", k, world, h);
                uint64_t prev = 0;
                for (int o = 1; o < world; ++o) {
                    const uint64_t x = s[o - 1];
                    if (x < prev || x % 16 || x > (1ULL << key_bits) || x & ((1ULL << shift) - 1))
                        return fail("split", k, world, h);
                    const int b = (int)(x >> shift);  // owners 0..o-1 hold bins [0, b)
                    const double want = acc * o / world;
                    if (acc > 0 && x > prev && !(cum[b - 1] >= want && (b < 2 || cum[b - 2] < want)))
                        return fail("weight", k, world, h);
                    if (acc == 0 && b != nb) return fail("empty", k, world, h);
                    prev = x;
                }
            }
        }
    }
    std::printf("splits ok\n");
    return 0;
}
