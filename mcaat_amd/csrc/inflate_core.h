// inflate_core.h — DEFLATE (RFC 1951) decoding of one gzip member into tokens, and CRC-32 by slices.
//
// The decoder of csrc/bgzf_inflate.hip, kept apart from the wave that runs it so that a plain
// host compiler can build and test it alone (tests/sanitize/inflate_core_test.cpp): no HIP
// types, no wave intrinsics. It turns the compressed bytes of one member into tokens (a literal
// byte, a match of length and distance, a run of stored bytes); whoever calls it executes them:
// the kernel with a 64-lane copy, the host test with a byte loop.
//
// Every check lives here, so an executor only ever sees tokens that are safe to execute:
//   - every input read lies inside [0, zlen);
//   - every output position lies inside [0, olen);
//   - every distance is at most the bytes produced so far (and at most 32768 by construction);
//   - reserved block types, length and distance codes, over-subscribed and incomplete code sets
//     (but for the one-code set of length 1 that DEFLATE allows, as zlib reads it), a repeat
//     with nothing to repeat or past the end, a missing end-of-block code and stored blocks
//     whose LEN / NLEN disagree are errors;
//   - at the end the produced length must equal olen and the input must be used up to its last
//     byte.
// The verdict is zlib's inflate() on the same bytes with an output buffer of exactly olen bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCAAT_INFL_HD __host__ __device__ inline
#else
#define MCAAT_INFL_HD inline
#endif

namespace mcaat {
namespace infl {

enum Status : uint32_t {
    kOk = 0,
    kErrBlockType = 1,  // block type 3
    kErrStored = 2,     // LEN != ~NLEN
    kErrCodeSet = 3,    // over-subscribed / incomplete code lengths, bad counts, bad repeat, no end-of-block
    kErrSymbol = 4,     // a code that is not assigned, or a reserved length / distance symbol
    kErrDistance = 5,   // a distance beyond the bytes produced so far
    kErrInput = 6,      // the compressed bytes end inside the stream
    kErrOutput = 7,     // the stream produces more than ISIZE bytes
    kErrLength = 8,     // the stream produced fewer than ISIZE bytes
    kErrTrailing = 9,   // compressed bytes left over after the final block
    kErrCrc = 10,       // CRC-32 of the produced bytes is not the trailer's
};

// token forms (32 bits)
constexpr uint32_t kTokMatch = 1u << 31;   // | length << 16 | (distance - 1)
constexpr uint32_t kTokStored = 1u << 30;  // | byte count; source: Decoder::stored_src; last of its batch
MCAAT_INFL_HD uint32_t tok_len(uint32_t t) {
    return (t & kTokMatch) ? (t >> 16) & 0x1FFu : (t & kTokStored) ? (t & 0xFFFFu) : 1u;
}
MCAAT_INFL_HD uint32_t tok_dist(uint32_t t) { return (t & 0x7FFFu) + 1; }

constexpr int kLitRoot = 10, kDistRoot = 8, kClRoot = 7;

// decode tables and work space of one decoder (3.7 KB: LDS in the kernel)
struct Tables {
    uint16_t lfast[1 << kLitRoot];  // symbol << 4 | code length, 0: longer than the root or unassigned
    uint16_t lsym[288];             // symbols in canonical order
    uint16_t lcount[16];            // codes per length
    uint16_t dfast[1 << kDistRoot];
    uint16_t dsym[32];
    uint16_t dcount[16];
    uint16_t work[16];
    uint8_t lens[320];
    uint8_t cl[20];
};

struct BitReader {
    const uint8_t *p;
    uint32_t n, pos;  // bytes in all, bytes loaded
    uint64_t buf;     // loaded and not consumed, low bit first; zero above cnt
    uint32_t cnt;
};

MCAAT_INFL_HD void br_init(BitReader &b, const uint8_t *p, uint32_t n) {
    b.p = p;
    b.n = n;
    b.pos = 0;
    b.buf = 0;
    b.cnt = 0;
}
// at least 33 bits afterwards unless the input ends first
MCAAT_INFL_HD void br_refill(BitReader &b) {
    if (b.cnt > 32) return;
    if (b.pos + 4 <= b.n) {
        const uint8_t *q = b.p + b.pos;
        const uint32_t w = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        b.buf |= (uint64_t)w << b.cnt;
        b.cnt += 32;
        b.pos += 4;
    } else {
        while (b.cnt <= 56 && b.pos < b.n) {
            b.buf |= (uint64_t)b.p[b.pos++] << b.cnt;
            b.cnt += 8;
        }
    }
}
MCAAT_INFL_HD void br_drop(BitReader &b, uint32_t k) {
    b.buf >>= k;
    b.cnt -= k;
}
// k <= 16 bits; false when the input ends first
MCAAT_INFL_HD bool br_take(BitReader &b, uint32_t k, uint32_t &v) {
    if (k > b.cnt) return false;
    v = (uint32_t)b.buf & ((1u << k) - 1);
    br_drop(b, k);
    return true;
}
// bytes of input used, a partly used byte counted whole
MCAAT_INFL_HD uint32_t br_bytes_used(const BitReader &b) { return b.pos - b.cnt / 8; }

MCAAT_INFL_HD uint32_t rev_bits(uint32_t c, int len) {
    c = ((c & 0x5555u) << 1) | ((c >> 1) & 0x5555u);
    c = ((c & 0x3333u) << 2) | ((c >> 2) & 0x3333u);
    c = ((c & 0x0F0Fu) << 4) | ((c >> 4) & 0x0F0Fu);
    c = ((c & 0x00FFu) << 8) | ((c >> 8) & 0x00FFu);
    return c >> (16 - len);
}

// Canonical code of n symbols with the lengths given (0: unused). Returns the unused code
// space: 0 complete, > 0 incomplete, < 0 over-subscribed (the tables are then not built).
// maxlen: the longest code length in use.
MCAAT_INFL_HD int build_code(const uint8_t *lens, int n, uint16_t *fast, int root, uint16_t *sym, uint16_t *count,
                             uint16_t *work, int &maxlen) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) count[lens[s]]++;
    maxlen = 0;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        if (count[l]) maxlen = l;
        left <<= 1;
        left -= count[l];
        if (left < 0) return left;
    }
    // symbols in canonical order
    work[1] = 0;
    for (int l = 1; l < 15; ++l) work[l + 1] = (uint16_t)(work[l] + count[l]);
    for (int s = 0; s < n; ++s)
        if (lens[s]) sym[work[lens[s]]++] = (uint16_t)s;
    // first-level table: every index whose low bits are a code of at most `root` bits
    const int size = 1 << root;
    for (int i = 0; i < size; ++i) fast[i] = 0;
    uint32_t code = 0;
    work[0] = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code + (l > 1 ? count[l - 1] : 0)) << 1;
        work[l] = (uint16_t)code;  // 15-bit codes at most: the set is not over-subscribed
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        if (!l || l > root) continue;
        const uint32_t c = work[l]++;
        for (uint32_t j = rev_bits(c, l); j < (uint32_t)size; j += 1u << l) fast[j] = (uint16_t)((s << 4) | l);
    }
    return left;
}

// One symbol: >= 0 the symbol, -1 no such code, -2 the input ends inside the code.
MCAAT_INFL_HD int decode_sym(BitReader &b, const uint16_t *fast, int root, const uint16_t *sym, const uint16_t *count) {
    const uint32_t v = (uint32_t)b.buf;
    const uint32_t e = fast[v & ((1u << root) - 1)];
    if (e) {
        const uint32_t l = e & 15;
        if (l > b.cnt) return -2;
        br_drop(b, l);
        return (int)(e >> 4);
    }
    // overflow path: walk the canonical code length by length
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        if (l > b.cnt) return -2;
        code |= (int)((v >> (l - 1)) & 1);
        const int c = count[l];
        if (code - c < first) {
            br_drop(b, l);
            return sym[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

struct Decoder {
    BitReader br;
    uint32_t olen;      // ISIZE: the bytes the member must produce
    uint32_t produced;  // bytes the tokens handed out so far produce
    uint32_t stored_src;  // input offset of the bytes of the stored token handed out last
    uint32_t err;       // Status
    uint8_t state;      // kHeader, kHuff, kDone
    uint8_t final_block;
};
enum : uint8_t { kHeader = 0, kHuff = 1, kDone = 2 };

MCAAT_INFL_HD void decoder_init(Decoder &d, const uint8_t *z, uint32_t zlen, uint32_t olen) {
    br_init(d.br, z, zlen);
    d.olen = olen;
    d.produced = 0;
    d.stored_src = 0;
    d.err = kOk;
    d.state = kHeader;
    d.final_block = 0;
}
MCAAT_INFL_HD bool decoder_done(const Decoder &d) { return d.state == kDone; }

MCAAT_INFL_HD uint32_t fail(Decoder &d, uint32_t e) {
    d.err = e;
    d.state = kDone;
    return e;
}

// the two codes of a fixed block
MCAAT_INFL_HD uint32_t fixed_tables(Tables &t) {
    int s = 0, mx;
    for (; s < 144; ++s) t.lens[s] = 8;
    for (; s < 256; ++s) t.lens[s] = 9;
    for (; s < 280; ++s) t.lens[s] = 7;
    for (; s < 288; ++s) t.lens[s] = 8;
    build_code(t.lens, 288, t.lfast, kLitRoot, t.lsym, t.lcount, t.work, mx);
    for (s = 0; s < 32; ++s) t.lens[s] = 5;
    build_code(t.lens, 32, t.dfast, kDistRoot, t.dsym, t.dcount, t.work, mx);
    return kOk;
}

// the code lengths and the two codes of a dynamic block
MCAAT_INFL_HD uint32_t dynamic_tables(Decoder &d, Tables &t) {
    BitReader &b = d.br;
    uint32_t nlen, ndist, ncode;
    br_refill(b);
    if (!br_take(b, 5, nlen) || !br_take(b, 5, ndist) || !br_take(b, 4, ncode)) return kErrInput;
    nlen += 257;
    ndist += 1;
    ncode += 4;
    if (nlen > 286 || ndist > 30) return kErrCodeSet;
    for (int i = 0; i < 19; ++i) t.cl[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) {
        // the order of the code length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const uint32_t at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 7 + ((i - 2) >> 1);
        uint32_t v;
        br_refill(b);
        if (!br_take(b, 3, v)) return kErrInput;
        t.cl[at] = (uint8_t)v;
    }
    int mx;
    if (build_code(t.cl, 19, t.lfast, kClRoot, t.lsym, t.lcount, t.work, mx) != 0) return kErrCodeSet;
    const uint32_t total = nlen + ndist;
    uint32_t idx = 0;
    while (idx < total) {
        br_refill(b);
        const int s = decode_sym(b, t.lfast, kClRoot, t.lsym, t.lcount);
        if (s < 0) return s == -2 ? kErrInput : kErrSymbol;
        if (s < 16) {
            t.lens[idx++] = (uint8_t)s;
            continue;
        }
        uint32_t prev = 0, rep = 0;
        if (s == 16) {
            if (idx == 0) return kErrCodeSet;
            prev = t.lens[idx - 1];
            if (!br_take(b, 2, rep)) return kErrInput;
            rep += 3;
        } else if (s == 17) {
            if (!br_take(b, 3, rep)) return kErrInput;
            rep += 3;
        } else {
            if (!br_take(b, 7, rep)) return kErrInput;
            rep += 11;
        }
        if (idx + rep > total) return kErrCodeSet;
        while (rep--) t.lens[idx++] = (uint8_t)prev;
    }
    if (t.lens[256] == 0) return kErrCodeSet;  // no end-of-block code
    int left = build_code(t.lens, (int)nlen, t.lfast, kLitRoot, t.lsym, t.lcount, t.work, mx);
    if (left < 0 || (left > 0 && mx != 1)) return kErrCodeSet;
    left = build_code(t.lens + nlen, (int)ndist, t.dfast, kDistRoot, t.dsym, t.dcount, t.work, mx);
    if (left < 0 || (left > 0 && mx > 1)) return kErrCodeSet;  // no distance code at all is allowed
    return kOk;
}

// Up to cap tokens into tok[]; returns how many. Call until decoder_done(); d.err then says how
// the stream ended. Tokens handed out before an error are valid and may be executed or not.
MCAAT_INFL_HD int next_tokens(Decoder &d, Tables &t, uint32_t *tok, int cap) {
    BitReader &b = d.br;
    int n = 0;
    while (n < cap && d.state != kDone) {
        if (d.state == kHeader) {
            if (d.final_block) {  // the end of the stream
                d.state = kDone;
                if (d.produced != d.olen) d.err = kErrLength;
                else if (br_bytes_used(b) != b.n) d.err = kErrTrailing;
                break;
            }
            uint32_t fin, type;
            br_refill(b);
            if (!br_take(b, 1, fin) || !br_take(b, 2, type)) { fail(d, kErrInput); break; }
            d.final_block = (uint8_t)fin;
            if (type == 3) { fail(d, kErrBlockType); break; }
            if (type == 0) {
                uint32_t len, nlen;
                br_drop(b, b.cnt & 7);
                br_refill(b);
                if (!br_take(b, 16, len) || !br_take(b, 16, nlen)) { fail(d, kErrInput); break; }
                if ((len ^ 0xFFFFu) != nlen) { fail(d, kErrStored); break; }
                // whole bytes are loaded beyond the header: hand them back
                b.pos -= b.cnt / 8;
                b.buf = 0;
                b.cnt = 0;
                if (len > b.n - b.pos) { fail(d, kErrInput); break; }
                if (len > d.olen - d.produced) { fail(d, kErrOutput); break; }
                d.stored_src = b.pos;
                b.pos += len;
                d.produced += len;
                if (len) {
                    tok[n++] = kTokStored | len;
                    break;  // the last token of its batch
                }
                continue;
            }
            const uint32_t e = type == 1 ? fixed_tables(t) : dynamic_tables(d, t);
            if (e != kOk) { fail(d, e); break; }
            d.state = kHuff;
        }
        // ---- symbols of a fixed or dynamic block
        br_refill(b);
        const int s = decode_sym(b, t.lfast, kLitRoot, t.lsym, t.lcount);
        if (s < 0) { fail(d, s == -2 ? kErrInput : kErrSymbol); break; }
        if (s < 256) {
            if (d.produced >= d.olen) { fail(d, kErrOutput); break; }
            tok[n++] = (uint32_t)s;
            d.produced += 1;
            continue;
        }
        if (s == 256) {
            d.state = kHeader;
            continue;
        }
        if (s >= 286) { fail(d, kErrSymbol); break; }
        const uint32_t k = (uint32_t)s - 257;
        uint32_t len = 258, ext = 0, x = 0;
        if (k < 8) {
            len = 3 + k;
        } else if (k < 28) {
            ext = (k >> 2) - 1;
            len = 3 + ((4 + (k & 3)) << ext);
        }
        if (!br_take(b, ext, x)) { fail(d, kErrInput); break; }
        len += x;
        br_refill(b);
        const int ds = decode_sym(b, t.dfast, kDistRoot, t.dsym, t.dcount);
        if (ds < 0) { fail(d, ds == -2 ? kErrInput : kErrSymbol); break; }
        if (ds >= 30) { fail(d, kErrSymbol); break; }
        uint32_t dist = 1 + (uint32_t)ds;
        ext = 0;
        x = 0;
        if (ds >= 4) {
            ext = ((uint32_t)ds >> 1) - 1;
            dist = 1 + ((2 + ((uint32_t)ds & 1)) << ext);
        }
        if (!br_take(b, ext, x)) { fail(d, kErrInput); break; }
        dist += x;
        if (dist > d.produced) { fail(d, kErrDistance); break; }
        if (len > d.olen - d.produced) { fail(d, kErrOutput); break; }
        tok[n++] = kTokMatch | (len << 16) | (dist - 1);
        d.produced += len;
    }
    return n;
}

// ---- CRC-32 (the gzip polynomial, reflected) by slices ----------------------------------------
// A lane takes the CRC of its slice; the slices' CRCs are merged as zlib's crc32_combine merges
// two: crc(A ++ B) = crc(A) * x^(8 |B|) mod P  xor  crc(B), so over many slices the whole CRC is
// the xor of every slice's CRC shifted by the bytes that follow the slice.
constexpr uint32_t kCrcPoly = 0xEDB88320u;

MCAAT_INFL_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
    return c;
}
// CRC-32 of n bytes, as zlib's crc32(0, p, n); table: the 256 values of crc_table_entry
MCAAT_INFL_HD uint32_t crc_slice(const uint32_t *table, const uint8_t *p, uint32_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
// a * b mod P; bit 31 is x^0
MCAAT_INFL_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// crc of a slice as it counts in a text that goes on for `after` bytes behind the slice
MCAAT_INFL_HD uint32_t crc_shift(uint32_t crc, uint32_t after) {
    uint32_t r = 0x80000000u, base = 0x00800000u;  // x^0, x^8
    for (uint32_t n = after; n; n >>= 1) {
        if (n & 1) r = crc_mulmod(r, base);
        base = crc_mulmod(base, base);
    }
    return crc_mulmod(r, crc);
}

}  // namespace infl
}  // namespace mcaat
