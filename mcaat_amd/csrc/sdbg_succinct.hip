// sdbg_succinct.hip — the succinct (BOSS) view of a built graph, measured beside the
// 26-B/edge arrays the path runs on (BASELINE north_star: "succinct de Bruijn graph ...
// wavefront ballot/prefix-sum for SDBG rank/select and edge traversal"; SURVEY.md §8a5 sizes
// it at ~3 B/edge; VERDICT r5 item 5: measure it before building more on the wide layout).
//
// Edge space (our ids: BOSS-key rank): one nibble per edge, 16 per word:
//   bits 0-1 W (the outgoing symbol), bit 2 last (the last edge of its source node), bit 3 W-
//   (an earlier edge of the same (k-1)-suffix group carries the same W: same target).
// Node space U: the labels that are a source (have out-edges) or a target (have in-edges), in
// colex order. Our ids materialise no MEGAHIT $-dummies, so BOSS's F-array arithmetic needs two
// bits per node: sink (a target without out-edges; not a source) and hin (has in-edges). The
// r-th non-minus W = c edge (id order) points at the r-th node with hin among the nodes whose
// label ends with c (colex order of the targets follows the id order of their edges), so
//   forward(e)  = select_hin(hinstart[c] + rank_c(e) - 1)                      (U position)
//   its edges   = node s = u - rank_sink(u): (select_last(s - 1), select_last(s)]
//   backward(e) = u = select_nonsink(node of e); e* = select_c(rank_hin(u) - hinstart[c]),
//                 then the W- edges with W = c among the next 15 ids (the same suffix group)
// Rank samples: per 64-entry block a 16-bit count relative to its 65536-entry superblock (u64);
// select samples: the position of every 512th one, then a binary search over the blocks and a
// popcount scan of the block. In a scan a wave holds one 64-edge block, so the edges' ranks are
// ballots + mbcnt over the wave (k_sv_outdeg_wave).
// The view is test / measurement infrastructure of the path, not on it: mcaat_graph_succinct_check
// builds it from the graph's arrays, checks every edge's valid out- and in-neighbours against
// them, and times the same degree scans on both.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "cub_helpers.h"

namespace mcaat {

namespace {

constexpr int kB = 256;
constexpr uint64_t kRep = 0x1111111111111111ULL;
constexpr int kSamp = 9;  // select sample every 2^9 ones

struct SvView {
    uint64_t D = 0, nU = 0, nodes = 0, nsink = 0;
    const uint64_t *sym = nullptr;   // edge nibbles, 16 per word
    const uint16_t *eblk = nullptr;  // per 64-edge block, 5 kinds (W = 0..3 non-minus, last): ones before it in its superblock
    const uint64_t *esb = nullptr;   // per 65536-edge superblock, 5 kinds: ones before it
    const uint64_t *es[5] = {};      // per kind: position of the (512 j)-th one
    uint64_t ecount[5] = {};         // per kind: ones
    const uint64_t *sinkbm = nullptr, *hinbm = nullptr;  // U bitmaps
    const uint16_t *ublk = nullptr;  // per 64-node block: (sink, hin) ones before it in its superblock
    const uint64_t *usb = nullptr;   // per 65536-node superblock: (sink, hin)
    const uint64_t *us[2] = {};      // select samples: [0] non-sink nodes (select0 of sink), [1] hin
    uint64_t ucount[2] = {};         // non-sink nodes, hin nodes
    uint64_t hinstart[5] = {}, Estart[5] = {};
    const uint64_t *valid = nullptr;
};

// position of the n-th (0-based) set bit of m (popcount(m) > n): a binary search over the
// halves' popcounts, six steps whatever n is
__device__ __forceinline__ int select64(uint64_t m, uint32_t n) {
    int pos = 0;
    uint32_t c = (uint32_t)__popc((uint32_t)m);
    if (n >= c) {
        n -= c;
        pos = 32;
        m >>= 32;
    }
#pragma unroll
    for (int w = 16; w; w >>= 1) {
        c = (uint32_t)__popc((uint32_t)m & ((1u << w) - 1));
        if (n >= c) {
            n -= c;
            pos += w;
            m >>= w;
        }
    }
    return pos;
}
__device__ __forceinline__ uint32_t nib(const uint64_t *sym, uint64_t e) { return (uint32_t)(sym[e >> 4] >> (4 * (e & 15))) & 15; }
// bit 4i set where nibble i is a non-minus edge with W == c
__device__ __forceinline__ uint64_t match_c(uint64_t w, uint32_t c) {
    const uint64_t y = w ^ (kRep * c);
    return ~(y | (y >> 1)) & ~(w >> 3) & kRep;
}
__device__ __forceinline__ uint64_t match_kind(uint64_t w, int kind) { return kind == 4 ? (w >> 2) & kRep : match_c(w, (uint32_t)kind); }

__device__ __forceinline__ uint64_t e_before_block(const SvView &v, int kind, uint64_t b) {
    return v.esb[(b >> 10) * 5 + kind] + v.eblk[b * 5 + kind];
}
// ones of `kind` at edges [0, e] (inclusive)
__device__ __forceinline__ uint64_t e_rank_incl(const SvView &v, int kind, uint64_t e) {
    const uint64_t b = e >> 6;
    uint64_t r = e_before_block(v, kind, b);
    const uint64_t we = e >> 4;
    for (uint64_t w = b * 4; w < we; ++w) r += __popcll(match_kind(v.sym[w], kind));
    const int sh = 4 * (int)(e & 15) + 4;
    const uint64_t m = sh >= 64 ? ~0ULL : ((1ULL << sh) - 1);
    return r + __popcll(match_kind(v.sym[we], kind) & m);
}
// the edge of the j-th (0-based) one of `kind`
__device__ uint64_t e_select(const SvView &v, int kind, uint64_t j) {
    const uint64_t nb = (v.D + 63) >> 6;
    uint64_t lo = v.es[kind][j >> kSamp] >> 6;
    const uint64_t ns = (v.ecount[kind] + (1u << kSamp) - 1) >> kSamp;
    uint64_t hi = (j >> kSamp) + 1 < ns ? v.es[kind][(j >> kSamp) + 1] >> 6 : nb - 1;
    while (lo < hi) {  // the last block whose count before it is <= j
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (e_before_block(v, kind, mid) <= j) lo = mid;
        else hi = mid - 1;
    }
    uint64_t r = e_before_block(v, kind, lo);
    for (uint64_t w = lo * 4;; ++w) {
        uint64_t m = match_kind(v.sym[w], kind);
        const uint64_t pc = __popcll(m);
        if (r + pc > j) return w * 16 + (uint64_t)(select64(m, (uint32_t)(j - r)) >> 2);
        r += pc;
    }
}

__device__ __forceinline__ uint64_t u_word(const SvView &v, int kind, uint64_t w) {
    return kind == 0 ? ~v.sinkbm[w] : v.hinbm[w];  // kind 0: non-sink (sources), 1: hin
}
__device__ __forceinline__ uint64_t u_before_block(const SvView &v, int kind, uint64_t b) {
    // stored: sink ones (kind 0 derives non-sink = positions - sinks) and hin ones
    const uint64_t x = v.usb[(b >> 10) * 2 + kind] + v.ublk[b * 2 + kind];
    return kind == 0 ? b * 64 - x : x;
}
// ones of `kind` at U positions [0, u) (exclusive)
__device__ __forceinline__ uint64_t u_rank_excl(const SvView &v, int kind, uint64_t u) {
    const uint64_t b = u >> 6;
    uint64_t r = u_before_block(v, kind, b);
    if (u & 63) r += __popcll(u_word(v, kind, b) & ((1ULL << (u & 63)) - 1));
    return r;
}
__device__ uint64_t u_select(const SvView &v, int kind, uint64_t j) {
    const uint64_t nb = (v.nU + 63) >> 6;
    uint64_t lo = v.us[kind][j >> kSamp] >> 6;
    const uint64_t ns = (v.ucount[kind] + (1u << kSamp) - 1) >> kSamp;
    uint64_t hi = (j >> kSamp) + 1 < ns ? v.us[kind][(j >> kSamp) + 1] >> 6 : nb - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (u_before_block(v, kind, mid) <= j) lo = mid;
        else hi = mid - 1;
    }
    uint64_t m = u_word(v, kind, lo);
    if (lo == nb - 1 && (v.nU & 63)) m &= (1ULL << (v.nU & 63)) - 1;  // bits past nU (non-sink reads them as ones)
    return lo * 64 + (uint64_t)select64(m, (uint32_t)(j - u_before_block(v, kind, lo)));
}

// the edges [first, last] of the source node at U position u (not a sink)
__device__ __forceinline__ void sv_node_edges(const SvView &v, uint64_t u, uint64_t &first, uint64_t &last) {
    const uint64_t s = u_rank_excl(v, 0, u);  // source nodes before u = its node index
    last = e_select(v, 4, s);
    first = s ? e_select(v, 4, s - 1) + 1 : 0;
}
// U position of the target of e (every target has an in-edge: hin)
__device__ __forceinline__ uint64_t sv_target(const SvView &v, uint64_t e, uint32_t c, uint64_t rank_c) {
    (void)e;
    return u_select(v, 1, v.hinstart[c] + rank_c - 1);
}
// valid out-edges of e, DESCENDING ids (OutgoingEdges); rank_c: e's non-minus W rank
__device__ int sv_outgoing_r(const SvView &v, uint64_t e, uint32_t c, uint64_t rank_c, uint64_t *out) {
    const uint64_t u = sv_target(v, e, c, rank_c);
    if (bit_get(v.sinkbm, u)) return 0;
    uint64_t lo, hi;
    sv_node_edges(v, u, lo, hi);
    int n = 0;
    for (uint64_t x = hi + 1; x-- > lo;)
        if (bit_get(v.valid, x)) out[n++] = x;
    return n;
}
__device__ int sv_outgoing(const SvView &v, uint64_t e, uint64_t *out) {
    const uint32_t c = nib(v.sym, e) & 3;
    return sv_outgoing_r(v, e, c, e_rank_incl(v, c, e), out);
}
// valid in-edges of e, ASCENDING ids (IncomingEdges)
__device__ int sv_incoming(const SvView &v, uint64_t e, uint64_t *in) {
    const uint64_t s = e ? e_rank_incl(v, 4, e - 1) : 0;  // nodes ending before e = e's node index
    const uint64_t u = u_select(v, 0, s);
    if (!bit_get(v.hinbm, u)) return 0;
    uint32_t c = 0;
    while (c < 3 && v.Estart[c + 1] <= e) ++c;  // the last symbol of e's label
    const uint64_t r = u_rank_excl(v, 1, u) - v.hinstart[c];
    const uint64_t first = e_select(v, (int)c, r);
    int n = 0;
    if (bit_get(v.valid, first)) in[n++] = first;
    for (uint64_t x = first + 1; x < v.D && x <= first + 15; ++x) {
        const uint32_t q = nib(v.sym, x);
        if ((q & 3) != c) continue;
        if (!(q >> 3)) break;  // the next group's first W = c edge
        if (bit_get(v.valid, x)) in[n++] = x;
    }
    return n;
}

// ---------------------------------------------------------------- build
// nibbles: W, last (the next key's label differs), minus (an earlier edge of the suffix group
// carries the same W: at most 15 edges back)
__global__ void __launch_bounds__(kB) k_sv_sym(const uint64_t *key, uint64_t D, uint64_t *sym) {
    const uint64_t nw = (D + 15) >> 4, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += stride) {
        uint64_t word = kRep * 8;  // past D: minus set, W 0, last 0 (matches no kind)
        for (int i = 0; i < 16; ++i) {
            const uint64_t e = w * 16 + i;
            if (e >= D) break;
            const uint64_t K = key[e];
            const uint32_t W = (uint32_t)(K & 3);
            const uint32_t last = e + 1 == D || (key[e + 1] >> 2) != (K >> 2);
            uint32_t minus = 0;
            for (uint64_t j = 1; j <= 15 && j <= e; ++j) {
                const uint64_t P = key[e - j];
                if ((P >> 4) != (K >> 4)) break;
                if ((P & 3) == W) {
                    minus = 1;
                    break;
                }
            }
            word = (word & ~(0xFULL << (4 * i))) | ((uint64_t)(W | (last << 2) | (minus << 3)) << (4 * i));
        }
        sym[w] = word;
    }
}
// per 64-edge block: ones of each kind
__global__ void __launch_bounds__(kB) k_sv_eblk_raw(const uint64_t *sym, uint64_t nb, uint64_t nsw, uint32_t *raw) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride) {
        uint32_t c[5] = {0, 0, 0, 0, 0};
        for (uint64_t w = 4 * b; w < 4 * b + 4 && w < nsw; ++w) {
            const uint64_t x = sym[w];
            for (int k = 0; k < 5; ++k) c[k] += (uint32_t)__popcll(match_kind(x, k));
        }
        for (int k = 0; k < 5; ++k) raw[(uint64_t)k * nb + b] = c[k];
    }
}
// from the exclusive sums (abs[k * nb + b]): 16-bit block counts and superblock counts
__global__ void __launch_bounds__(kB) k_sv_pack(const uint64_t *abs, uint64_t nb, int kinds, uint16_t *blk, uint64_t *sb) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride)
        for (int k = 0; k < kinds; ++k) {
            const uint64_t a = abs[(uint64_t)k * nb + b], s = abs[(uint64_t)k * nb + (b & ~1023ULL)];
            blk[b * kinds + k] = (uint16_t)(a - s);
            if ((b & 1023) == 0) sb[(b >> 10) * kinds + k] = a;
        }
}
// select samples: the position of the (512 j)-th one of each kind, found in the block holding it
__global__ void __launch_bounds__(kB) k_sv_esamples(SvView v, uint64_t nb, uint64_t *s0, uint64_t *s1, uint64_t *s2,
                                                    uint64_t *s3, uint64_t *s4) {
    uint64_t *S[5] = {s0, s1, s2, s3, s4};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride)
        for (int k = 0; k < 5; ++k) {
            uint64_t r = e_before_block(v, k, b);
            const uint64_t want = (r + (1u << kSamp) - 1) & ~(uint64_t)((1u << kSamp) - 1);  // next multiple of 512 at or after r
            for (uint64_t w = 4 * b; w < 4 * b + 4 && w < (v.D + 15) / 16; ++w) {
                uint64_t m = match_kind(v.sym[w], k);
                const uint64_t pc = __popcll(m);
                if (want >= r && want < r + pc) S[k][want >> kSamp] = w * 16 + (uint64_t)(select64(m, (uint32_t)(want - r)) >> 2);
                r += pc;
            }
        }
}
// sinks: non-minus edges whose target has no out-edges, flagged per W (the sorted sink order is
// by W, then id: colex order of the target labels)
__global__ void __launch_bounds__(kB) k_sv_sink_flags(const uint64_t *sym, const uint64_t *out_info, uint64_t D, uint8_t *flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < D; e += stride) {
        const uint32_t q = nib(sym, e);
        flag[e] = !(q >> 3) && ((out_info[e] >> kIdxBits) & 0xF) == 0 ? (uint8_t)(1 + (q & 3)) : 0;
    }
}
__global__ void __launch_bounds__(kB) k_sv_sink_count(const uint8_t *flag, uint64_t n, unsigned long long *cnt) {
    __shared__ unsigned long long c4[4];
    if (threadIdx.x < 4) c4[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long m[4] = {0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (flag[i]) ++m[flag[i] - 1];
    for (int c = 0; c < 4; ++c)
        if (m[c]) atomicAdd(&c4[c], m[c]);
    __syncthreads();
    if (threadIdx.x < 4 && c4[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], c4[threadIdx.x]);
}
__global__ void __launch_bounds__(kB) k_sv_eq(const uint8_t *flag, uint64_t n, uint8_t v, uint8_t *out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = flag[i] == v;
}
// nodes whose last edge precedes q[c] (c = 0..4), and hin nodes before U position q[c]
__global__ void k_sv_nodes_before(SvView v, const uint64_t *q, uint64_t *r) {
    const int c = threadIdx.x;
    if (c <= 4) r[c] = q[c] ? e_rank_incl(v, 4, q[c] - 1) : 0;
}
__global__ void k_sv_hin_before(SvView v, const uint64_t *q, uint64_t *r) {
    const int c = threadIdx.x;
    if (c <= 4) r[c] = u_rank_excl(v, 1, q[c]);
}
__global__ void __launch_bounds__(kB) k_sv_iota(uint64_t *x, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = i;
}
// a_i = source nodes whose label precedes sink i's (target) label: the nodes entirely before the
// lower bound of its label in the keys
__global__ void __launch_bounds__(kB) k_sv_sink_pos(SvView v, const uint64_t *key, int k, const uint64_t *dir, int shift,
                                                    const uint64_t *sink_edge, uint64_t ns, uint64_t *a, uint32_t *cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += stride) {
        const uint64_t e = sink_edge[i];
        const uint64_t lsb = boss_to_lsb(key[e], k);
        const uint64_t q = (lsb >> 2) << 2;  // the target label as a BOSS key with W = 0
        const uint64_t p = q >> shift;
        uint64_t lo = dir[p], hi = dir[p + 1];
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (key[mid] < q) lo = mid + 1;
            else hi = mid;
        }
        const uint64_t nodes_before = lo ? e_rank_incl(v, 4, lo - 1) : 0;
        a[i] = nodes_before;
        atomicAdd(&cnt[nodes_before], 1u);
    }
}
__global__ void __launch_bounds__(kB) k_sv_mark_sinks(const uint64_t *a, uint64_t ns, uint64_t *sinkbm, uint64_t *hinbm) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += stride) {
        const uint64_t u = a[i] + i;
        atomicOr((unsigned long long *)&sinkbm[u >> 6], 1ULL << (u & 63));
        atomicOr((unsigned long long *)&hinbm[u >> 6], 1ULL << (u & 63));
    }
}
// node s (its last edge e) sits at U position s + sinks_before(s); its hin bit from in_info
__global__ void __launch_bounds__(kB) k_sv_mark_nodes(SvView v, const uint64_t *in_info, const uint32_t *sinks_incl,
                                                      uint64_t *hinbm) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < v.D; e += stride) {
        if (!((nib(v.sym, e) >> 2) & 1)) continue;  // one thread per node: its last edge
        if (!((in_info[e] >> kIdxBits) & 0xFFFF)) continue;
        const uint64_t s = e_rank_incl(v, 4, e) - 1;
        const uint64_t u = s + sinks_incl[s];
        atomicOr((unsigned long long *)&hinbm[u >> 6], 1ULL << (u & 63));
    }
}
__global__ void __launch_bounds__(kB) k_sv_ublk_raw(const uint64_t *sinkbm, const uint64_t *hinbm, uint64_t nb, uint32_t *raw) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride) {
        raw[b] = (uint32_t)__popcll(sinkbm[b]);
        raw[nb + b] = (uint32_t)__popcll(hinbm[b]);
    }
}
__global__ void __launch_bounds__(kB) k_sv_usamples(SvView v, uint64_t nb, uint64_t *s0, uint64_t *s1) {
    uint64_t *S[2] = {s0, s1};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride)
        for (int k = 0; k < 2; ++k) {
            const uint64_t r = u_before_block(v, k, b);
            uint64_t m = u_word(v, k, b);
            if (b == nb - 1 && (v.nU & 63)) m &= (1ULL << (v.nU & 63)) - 1;
            const uint64_t pc = __popcll(m);
            const uint64_t want = (r + (1u << kSamp) - 1) & ~(uint64_t)((1u << kSamp) - 1);
            if (want < r + pc) S[k][want >> kSamp] = b * 64 + (uint64_t)select64(m, (uint32_t)(want - r));
        }
}

// ---------------------------------------------------------------- checks and scans
__global__ void __launch_bounds__(kB) k_sv_check(GraphView g, SvView v, unsigned long long *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bo = 0, bi = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < g.D; e += stride) {
        uint64_t a[4], b[4], c[16], d[16];
        const int na = dev_outgoing(g, e, a), nb2 = sv_outgoing(v, e, b);
        bool ok = na == nb2;
        for (int i = 0; ok && i < na; ++i) ok = a[i] == b[i];
        bo += !ok;
        const int nc = dev_incoming(g, e, c), nd = sv_incoming(v, e, d);
        ok = nc == nd;
        for (int i = 0; ok && i < nc; ++i) ok = c[i] == d[i];
        bi += !ok;
    }
    if (bo) atomicAdd(&bad[0], bo);
    if (bi) atomicAdd(&bad[1], bi);
}
// the degree scans timed on both layouts: every valid edge's valid out-degree (tips: 0) or
// in-degree; a tips bitmap and a degree sum, so the two layouts' outputs can be compared
template <bool IN>
__global__ void __launch_bounds__(kB) k_deg_info(GraphView g, uint64_t *tips, unsigned long long *sum) {
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (g.D + 63) / 64, wstride = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long s = 0;
    for (uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nw; w += wstride) {
        const uint64_t e = w * 64 + lane;
        bool t = false;
        if (e < g.D && bit_get(g.valid, e)) {
            uint64_t x[16];
            const int d = IN ? dev_incoming(g, e, x) : dev_outgoing(g, e, x);
            s += d;
            t = d == 0;
        }
        const unsigned long long m = __ballot(t);
        if (lane == 0) tips[w] = m;
    }
    block_add(sum, s);
}
// the same scan on the succinct view, one 64-edge block per wave: each edge's rank among the
// block's non-minus edges of its W is a ballot + mbcnt (the wavefront rank of north_star)
template <bool IN>
__global__ void __launch_bounds__(kB) k_deg_sv(SvView v, uint64_t *tips, unsigned long long *sum) {
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (v.D + 63) / 64, wstride = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long s = 0;
    for (uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nw; w += wstride) {
        const uint64_t e = w * 64 + lane;
        const bool in = e < v.D;
        const uint32_t q = in ? nib(v.sym, e) : 0xF;
        const uint32_t c = q & 3;
        const bool nm = in && !(q >> 3);
        uint64_t below = 0;
        for (uint32_t cc = 0; cc < 4; ++cc) {
            const unsigned long long m = __ballot(nm && c == cc);
            if (c == cc) below = (uint64_t)__popcll(m & (lane == 63 ? ~0ULL : ((1ULL << (lane + 1)) - 1)));
        }
        bool t = false;
        if (in && bit_get(v.valid, e)) {
            uint64_t x[16];
            int d;
            if (IN) {
                d = sv_incoming(v, e, x);
            } else {
                // rank_c(e) = non-minus W = c edges before the block + those of the block up to e (a
                // minus edge counts its group's non-minus one, before it in the block or earlier)
                const uint64_t rc = e_before_block(v, (int)c, w) + below;
                d = sv_outgoing_r(v, e, c, rc, x);
            }
            s += d;
            t = d == 0;
        }
        const unsigned long long m = __ballot(t);
        if (lane == 0) tips[w] = m;
    }
    block_add(sum, s);
}

// the out-degree scan with the selects streamed over the wave (the form a succinct CycleFinder
// scan would take): the non-minus edges of one W in a 64-edge block point at consecutive has-in
// nodes, so one select per W and wave finds the first target and every lane walks the has-in
// bitmap from there to its own; the targets' node indices are again consecutive, so one select
// of the `last` bits per W and wave, then a walk over the nibbles, gives each node's edges
__device__ __forceinline__ uint64_t nth_one_from(const uint64_t *bm, uint64_t from, uint64_t n) {
    uint64_t w = from >> 6, m = bm[w] & (~0ULL << (from & 63));
    for (;;) {
        const uint64_t pc = __popcll(m);
        if (n < pc) return w * 64 + (uint64_t)select64(m, (uint32_t)n);
        n -= pc;
        m = bm[++w];
    }
}
// position of the n-th (0-based) `last` edge at or after edge `from`
__device__ __forceinline__ uint64_t nth_last_from(const uint64_t *sym, uint64_t from, uint64_t n) {
    uint64_t w = from >> 4, m = (sym[w] >> 2) & kRep & (~0ULL << (4 * (from & 15)));
    for (;;) {
        const uint64_t pc = __popcll(m);
        if (n < pc) return w * 16 + (uint64_t)(select64(m, (uint32_t)n) >> 2);
        n -= pc;
        m = (sym[++w] >> 2) & kRep;
    }
}
__global__ void __launch_bounds__(kB) k_deg_sv_stream(SvView v, uint64_t *tips, unsigned long long *sum) {
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (v.D + 63) / 64, wstride = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long s = 0;
    for (uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nw; w += wstride) {
        const uint64_t e = w * 64 + lane;
        const bool in = e < v.D;
        const uint32_t q = in ? nib(v.sym, e) : 0xF;
        const uint32_t c = q & 3;
        const bool nm = in && !(q >> 3);
        const bool act = in && bit_get(v.valid, e);
        int d = 0;
        for (uint32_t cc = 0; cc < 4; ++cc) {
            const unsigned long long mc = __ballot(nm && c == cc);
            const unsigned long long need = __ballot(act && c == cc);
            if (!need) continue;
            const bool mine = act && c == cc;
            // hin rank of this lane's target, and the wave's smallest
            const uint64_t below = (uint64_t)__popcll(mc & (lane == 63 ? ~0ULL : ((1ULL << (lane + 1)) - 1)));
            const uint64_t t0 = v.hinstart[cc] + e_before_block(v, (int)cc, w);  // + below - 1
            const int l0 = __ffsll((long long)need) - 1;
            const uint64_t b0 = __shfl(below, l0);
            // the first lane's target by one select; the others walk the has-in bitmap from it
            uint64_t u0 = 0;
            if (lane == l0) u0 = u_select(v, 1, t0 + b0 - 1);
            u0 = __shfl(u0, l0);
            uint64_t u = 0;
            bool sink = true;
            uint64_t sidx = ~0ULL;
            if (mine) {
                u = below == b0 ? u0 : nth_one_from(v.hinbm, u0, below - b0);
                sink = bit_get(v.sinkbm, u);
                if (!sink) sidx = u_rank_excl(v, 0, u);
            }
            // the smallest node index among the lanes, its first edge by one select; each lane
            // then walks the last bits to its own node's edges
            uint64_t smin = sidx;
            for (int o = 32; o; o >>= 1) smin = min(smin, (uint64_t)__shfl_xor(smin, o));
            if (smin == ~0ULL) continue;  // every target a sink
            const int ls = __ffsll((long long)__ballot(sidx == smin)) - 1;
            uint64_t p0 = 0;
            if (lane == ls) p0 = smin ? e_select(v, 4, smin - 1) + 1 : 0;
            p0 = __shfl(p0, ls);
            if (mine && !sink) {
                const uint64_t first = sidx == smin ? p0 : nth_last_from(v.sym, p0, sidx - smin - 1) + 1;
                const uint64_t last = nth_last_from(v.sym, first, 0);
                for (uint64_t x = first; x <= last; ++x) d += bit_get(v.valid, x);
            }
        }
        s += d;
        const unsigned long long m = __ballot(act && d == 0);
        if (lane == 0) tips[w] = m;
    }
    block_add(sum, s);
}

struct SvBufs {
    DevBuf<uint64_t> sym, esb, es[5], sinkbm, hinbm, usb, us[2];
    DevBuf<uint16_t> eblk, ublk;
    uint64_t bytes() const {
        uint64_t b = sym.bytes() + esb.bytes() + eblk.bytes() + sinkbm.bytes() + hinbm.bytes() + usb.bytes() + ublk.bytes();
        for (auto &x : es) b += x.bytes();
        for (auto &x : us) b += x.bytes();
        return b;
    }
};

// The view's arrays, block by block: symbols -> edge-space rank structure and its samples ->
// Estart -> sinks (sorted by W, id) -> node-space bitmaps -> node-space rank structure and its
// samples -> hinstart. A block's scratch buffers go back to the arena where the block ends.
SvView build_view(mcaat_graph *g, SvBufs &B, uint64_t *n_sinks) {
    mcaat_ctx *ctx = g->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t D = g->D;
    const int k = g->k;
    auto grid = [&](uint64_t n) { return dim3(grid_for(n, kB, (unsigned)ctx->n_cu * 16)); };
    // the last entry of an exclusive scan plus the last value scanned: the total
    auto scan_total = [&](const uint64_t *abs, const uint32_t *raw, uint64_t n) {
        uint64_t a = 0;
        uint32_t r = 0;
        d2h(ctx, &a, abs + n - 1, 8);
        d2h(ctx, &r, raw + n - 1, 4);
        return a + r;
    };
    SvView v;
    v.D = D;
    v.valid = g->valid.p;

    // symbols: one nibble per edge
    const uint64_t nsw = (D + 15) / 16, nb = (D + 63) / 64;
    B.sym.alloc(4 * nb + 1);  // whole blocks (the scans read 4 words per block)
    HIP_OK(hipMemsetAsync(B.sym.p, 0x88, B.sym.bytes(), st));  // nibbles past D match no kind
    launch_at(st, grid(nsw), dim3(kB), k_sv_sym, g->key.p, D, B.sym.p);
    v.sym = B.sym.p;

    // edge-space rank structure: per-block counts of the five kinds, scanned and packed; samples
    B.eblk.alloc(5 * nb);
    B.esb.alloc(5 * ((nb + 1023) / 1024));
    {
        DevBuf<uint32_t> raw(5 * nb);
        DevBuf<uint64_t> abs(5 * nb);
        launch_at(st, grid(nb), dim3(kB), k_sv_eblk_raw, B.sym.p, nb, nsw, raw.p);
        for (int kd = 0; kd < 5; ++kd)
            excl_scan(st, (const uint32_t *)raw.p + (uint64_t)kd * nb, abs.p + (uint64_t)kd * nb, nb);
        launch_at(st, grid(nb), dim3(kB), k_sv_pack, abs.p, nb, 5, B.eblk.p, B.esb.p);
        for (int kd = 0; kd < 5; ++kd) v.ecount[kd] = scan_total(abs.p + (uint64_t)kd * nb, raw.p + (uint64_t)kd * nb, nb);
    }
    v.eblk = B.eblk.p;
    v.esb = B.esb.p;
    for (int kd = 0; kd < 5; ++kd) {
        B.es[kd].alloc((v.ecount[kd] >> kSamp) + 1);
        v.es[kd] = B.es[kd].p;
    }
    launch_at(st, grid(nb), dim3(kB), k_sv_esamples, v, nb, B.es[0].p, B.es[1].p, B.es[2].p, B.es[3].p, B.es[4].p);
    v.nodes = v.ecount[4];

    // Estart[c]: the first edge whose label ends with c (BOSS key c << 2k), a lower bound on the
    // host through single-key reads (five values)
    for (int c = 0; c < 5; ++c) {
        const uint64_t q = (uint64_t)c << (2 * k);
        uint64_t lo = 0, hi = D;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            uint64_t km = 0;
            d2h(ctx, &km, g->key.p + mid, 8);
            if (km < q) lo = mid + 1;
            else hi = mid;
        }
        v.Estart[c] = lo;
    }

    // sinks, sorted by (W, id): the sinks per W first, then each W's flagged ids (a counting
    // iterator: no id array)
    DevBuf<uint64_t> sink_edge;
    uint64_t ns = 0;
    std::vector<uint64_t> ns_c(4, 0);
    {
        DevBuf<uint8_t> flag(D ? D : 1);
        launch_at(st, grid(D), dim3(kB), k_sv_sink_flags, B.sym.p, g->out_info.p, D, flag.p);
        DevBuf<unsigned long long> cnt4(4), num(1);
        HIP_OK(hipMemsetAsync(cnt4.p, 0, 32, st));
        launch_at(st, grid(D), dim3(kB), k_sv_sink_count, flag.p, D, cnt4.p);
        unsigned long long hc4[4];
        d2h(ctx, hc4, cnt4.p, 32);
        DevBuf<uint8_t> f1(D ? D : 1);
        std::vector<DevBuf<uint64_t>> per(4);
        hipcub::CountingInputIterator<uint64_t> ids((uint64_t)0);
        for (int c = 0; c < 4; ++c) {
            ns_c[c] = hc4[c];
            per[c].alloc(hc4[c] ? hc4[c] : 1);
            ns += hc4[c];
            if (!hc4[c]) continue;
            launch_at(st, grid(D), dim3(kB), k_sv_eq, flag.p, D, c + 1, f1.p);
            with_cub_temp([&](void *t, size_t &tmp) {
                return hipcub::DeviceSelect::Flagged(t, tmp, ids, f1.p, per[c].p, num.p, (size_t)D, st);
            });
        }
        sink_edge.alloc(ns ? ns : 1);
        uint64_t o = 0;
        for (int c = 0; c < 4; ++c) {
            if (ns_c[c]) HIP_OK(hipMemcpyAsync(sink_edge.p + o, per[c].p, 8 * ns_c[c], hipMemcpyDeviceToDevice, st));
            o += ns_c[c];
        }
        HIP_OK(hipStreamSynchronize(st));
    }
    v.nsink = ns;
    v.nU = v.nodes + ns;

    // node-space bitmaps: the sinks' positions among the nodes, the nodes with an incoming edge
    const uint64_t nub = (v.nU + 63) / 64;
    B.sinkbm.alloc(nub + 1);
    B.hinbm.alloc(nub + 1);
    HIP_OK(hipMemsetAsync(B.sinkbm.p, 0, B.sinkbm.bytes(), st));
    HIP_OK(hipMemsetAsync(B.hinbm.p, 0, B.hinbm.bytes(), st));
    {
        DevBuf<uint64_t> a(ns ? ns : 1);
        DevBuf<uint32_t> cnt(v.nodes + 1), incl(v.nodes + 1);
        HIP_OK(hipMemsetAsync(cnt.p, 0, cnt.bytes(), st));
        if (ns) {
            launch_at(st, grid(ns), dim3(kB), k_sv_sink_pos, v, g->key.p, k, g->dir.p, g->dir_shift, sink_edge.p, ns, a.p, cnt.p);
            launch_at(st, grid(ns), dim3(kB), k_sv_mark_sinks, a.p, ns, B.sinkbm.p, B.hinbm.p);
        }
        with_cub_temp([&](void *t, size_t &tmp) {
            return hipcub::DeviceScan::InclusiveSum(t, tmp, cnt.p, incl.p, (size_t)(v.nodes + 1), st);
        });
        launch_at(st, grid(D), dim3(kB), k_sv_mark_nodes, v, g->in_info.p, incl.p, B.hinbm.p);
        HIP_OK(hipStreamSynchronize(st));
    }
    v.sinkbm = B.sinkbm.p;
    v.hinbm = B.hinbm.p;

    // node-space rank structure over the two bitmaps; samples
    B.ublk.alloc(2 * nub + 2);
    B.usb.alloc(2 * ((nub + 1023) / 1024) + 2);
    {
        DevBuf<uint32_t> raw(2 * nub + 2);
        DevBuf<uint64_t> abs(2 * nub + 2);
        launch_at(st, grid(nub), dim3(kB), k_sv_ublk_raw, B.sinkbm.p, B.hinbm.p, nub, raw.p);
        for (int kd = 0; kd < 2; ++kd)
            excl_scan(st, (const uint32_t *)raw.p + (uint64_t)kd * nub, abs.p + (uint64_t)kd * nub, nub);
        launch_at(st, grid(nub), dim3(kB), k_sv_pack, abs.p, nub, 2, B.ublk.p, B.usb.p);
        v.ucount[1] = scan_total(abs.p + nub, raw.p + nub, nub);  // nodes with an incoming edge
    }
    v.ublk = B.ublk.p;
    v.usb = B.usb.p;
    v.ucount[0] = v.nodes;
    for (int kd = 0; kd < 2; ++kd) {
        B.us[kd].alloc((v.ucount[kd] >> kSamp) + 1);
        v.us[kd] = B.us[kd].p;
    }
    launch_at(st, grid(nub), dim3(kB), k_sv_usamples, v, nub, B.us[0].p, B.us[1].p);

    // hinstart[c]: hin nodes before Ustart[c], the first U position whose label ends with c
    // (nodes whose label ends before c, plus the sinks of the W < c edges)
    {
        DevBuf<uint64_t> q(8), res(8);
        h2d(ctx, q.p, v.Estart, 40);
        launch_at(st, dim3(1), dim3(64), k_sv_nodes_before, v, q.p, res.p);
        std::vector<uint64_t> nbc(5), ustart(5);
        d2h(ctx, nbc.data(), res.p, 40);
        uint64_t sb = 0;
        for (int c = 0; c <= 4; ++c) {
            ustart[c] = nbc[c] + sb;
            if (c < 4) sb += ns_c[c];
        }
        h2d(ctx, q.p, ustart.data(), 40);
        launch_at(st, dim3(1), dim3(64), k_sv_hin_before, v, q.p, res.p);
        d2h(ctx, v.hinstart, res.p, 40);
    }
    *n_sinks = ns;
    return v;
}

}  // namespace

void graph_succinct_check(mcaat_graph *g, bool check, uint64_t *out, double *ms) {
    mcaat_ctx *ctx = g->ctx;
    hipStream_t st = ctx->stream;
    if (g->sharded) throw Error(MCAAT_E_INVALID, "succinct view: unshard the graph first");
    if (g->gid.n) throw Error(MCAAT_E_INVALID, "succinct view: not on a region replica");
    const uint64_t D = g->D;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    for (int i = 0; i < 6; ++i) ms[i] = 0;
    if (!D) return;
    HIP_OK(hipStreamSynchronize(st));
    hipEvent_t a = event_get(ctx), b = event_get(ctx);
    auto elapsed = [&]() {
        float t = 0;
        HIP_OK(hipEventSynchronize(b));
        HIP_OK(hipEventElapsedTime(&t, a, b));
        return (double)t;
    };
    SvBufs B;
    uint64_t ns = 0;
    HIP_OK(hipEventRecord(a, st));
    const SvView v = build_view(g, B, &ns);
    HIP_OK(hipEventRecord(b, st));
    ms[0] = elapsed();
    out[0] = B.bytes();
    out[1] = 8 * D * 3;  // key + out_info + in_info (mult and valid are shared)
    out[4] = v.nU;
    out[5] = ns;
    const GraphView gv = g->view();
    if (check) {
        DevBuf<unsigned long long> bad(2);
        HIP_OK(hipMemsetAsync(bad.p, 0, 16, st));
        launch_at(st, dim3(grid_for(D, kB, (unsigned)ctx->n_cu * 16)), dim3(kB), k_sv_check, gv, v, bad.p);
        unsigned long long hb[2];
        d2h(ctx, hb, bad.p, 16);
        out[2] = hb[0];
        out[3] = hb[1];
    }
    // the degree scans, timed (second run of each: the first loads code and warms the TLB)
    const uint64_t nw = (D + 63) / 64;
    DevBuf<uint64_t> t1(nw), t2(nw);
    DevBuf<unsigned long long> s(4);
    const dim3 gw(grid_for(nw * 64, kB, (unsigned)ctx->n_cu * 16));
    auto run = [&](auto kern, auto view, uint64_t *tips, unsigned long long *sum) {
        double best = 1e30;
        for (int rep = 0; rep < 2; ++rep) {
            HIP_OK(hipMemsetAsync(sum, 0, 8, st));
            HIP_OK(hipEventRecord(a, st));
            launch_at(st, gw, dim3(kB), kern, view, tips, sum);
            HIP_OK(hipEventRecord(b, st));
            best = std::min(best, elapsed());
        }
        return best;
    };
    bool same = true;
    {  // the out-degree scan with streamed selects (its output against the arrays' scan)
        run(k_deg_info<false>, gv, t1.p, s.p);
        ms[5] = run(k_deg_sv_stream, v, t2.p, s.p + 1);
        unsigned long long hs[2];
        d2h(ctx, hs, s.p, 16);
        std::vector<uint64_t> h1(nw), h2(nw);
        d2h(ctx, h1.data(), t1.p, 8 * nw);
        d2h(ctx, h2.data(), t2.p, 8 * nw);
        same = hs[0] == hs[1] && h1 == h2;
    }
    for (int dir = 0; dir < 2; ++dir) {
        ms[1 + 2 * dir] = dir ? run(k_deg_info<true>, gv, t1.p, s.p) : run(k_deg_info<false>, gv, t1.p, s.p);
        ms[2 + 2 * dir] = dir ? run(k_deg_sv<true>, v, t2.p, s.p + 1) : run(k_deg_sv<false>, v, t2.p, s.p + 1);
        unsigned long long hs[2];
        d2h(ctx, hs, s.p, 16);
        std::vector<uint64_t> h1(nw), h2(nw);
        d2h(ctx, h1.data(), t1.p, 8 * nw);
        d2h(ctx, h2.data(), t2.p, 8 * nw);
        same = same && hs[0] == hs[1] && h1 == h2;
        out[6 + dir] = hs[0];
    }
    if (!same) out[2] += 1ULL << 40;  // the scans disagree: flagged in the mismatch count
    event_put(ctx, a);
    event_put(ctx, b);
}

void preload_sdbg_succinct() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)k_sv_sym);
}

}  // namespace mcaat
