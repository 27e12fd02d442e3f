// splits.h — how the sharded build cuts the BOSS key space into owner ranges.
//
// The ranks sum a histogram of the top shard_hist_bits(k) bits of the 2(k+1)-bit BOSS key and
// choose_splits cuts it into `world` contiguous owner ranges of about equal weight; a split is a
// histogram-bin edge, so a multiple of 2^(2(k+1) - bits).
//
// Edges sharing key >> 4 form a group (one node's edges); the sharded adjacency and the per-shard
// CycleFinder rest on groups not straddling ranks (shard_cf.hip), so a split must be a multiple of
// 16: the histogram never resolves the low 4 key bits, bits = min(12, 2(k-1)). At k >= 7 that is
// 12 bits; below, fewer (k = 2: 2 bits, four bins of one first symbol each), and the shift the
// histogram kernel receives, 2(k+1) - bits, is at least 4 at every k.
//
// Self-contained (no HIP header needed), so a plain host compiler can build it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mcaat {

constexpr int kShardHistBitsMax = 12;

inline int shard_hist_bits(int k) { return std::min(kShardHistBitsMax, 2 * (k - 1)); }

// world-1 ascending split points at histogram-bin edges with equal weight (owner o takes
// keys in [splits[o-1], splits[o])): owners 0..o-1 together end after the first bin whose
// running sum reaches total * o / world. hist has 2^bits bins, 0 < bits <= key_bits.
inline std::vector<uint64_t> choose_splits(const std::vector<uint64_t> &hist, int world, int key_bits) {
    const int nb = (int)hist.size();
    int bits = 0;
    while ((1 << bits) < nb) ++bits;
    const int shift = key_bits - bits;
    std::vector<double> cum(nb);
    double acc = 0;
    for (int i = 0; i < nb; ++i) cum[i] = acc += (double)hist[i];
    const double total = nb ? cum[nb - 1] : 0.0;
    std::vector<uint64_t> out;
    int prev = 0;
    for (int o = 1; o < world; ++o) {
        int b = nb;
        if (total > 0) b = (int)(std::lower_bound(cum.begin(), cum.end(), total * o / world) - cum.begin()) + 1;
        b = std::min(std::max(b, prev), nb);
        out.push_back((uint64_t)b << shift);
        prev = b;
    }
    return out;
}

}  // namespace mcaat
