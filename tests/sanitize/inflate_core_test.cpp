// Stand-alone check of mcaat_amd/csrc/inflate_core.h against zlib, meant to be built with
// -fsanitize=address,undefined: round trips over every block type and the copy edge cases, the
// CRC merge, and a sweep of mutated streams whose verdict must be zlib's. Buffers are allocated
// at exactly their lengths, so a read past the compressed bytes or a write past ISIZE is a
// sanitizer report. Prints "inflate_core ok" and returns 0 when everything holds.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../mcaat_amd/csrc/inflate_core.h"

using namespace mcaat::infl;

static int g_fail = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (g_fail++ < 20) {                       \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                   \
                printf("\n");                          \
            }                                          \
        }                                              \
    } while (0)

struct Setting {
    const char *name;
    int level, strategy, mem;
};
static const Setting kSettings[] = {{"stored", 0, Z_DEFAULT_STRATEGY, 8}, {"l1", 1, Z_DEFAULT_STRATEGY, 8},
                                    {"l6", 6, Z_DEFAULT_STRATEGY, 8},     {"l9", 9, Z_DEFAULT_STRATEGY, 8},
                                    {"fixed", 6, Z_FIXED, 8},             {"mem1", 6, Z_DEFAULT_STRATEGY, 1}};
static const int kNSettings = sizeof kSettings / sizeof kSettings[0];

static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t> &text, const Setting &s) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, s.level, Z_DEFLATED, -15, s.mem, s.strategy) != Z_OK) abort();
    std::vector<uint8_t> out(deflateBound(&z, (uLong)text.size()) + 64);
    uint8_t dummy = 0;
    z.next_in = text.empty() ? &dummy : const_cast<uint8_t *>(text.data());
    z.avail_in = (uInt)text.size();
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

// exact-size heap copy: any overrun is an AddressSanitizer report
struct Exact {
    uint8_t *p;
    size_t n;
    explicit Exact(size_t n_) : p(new uint8_t[n_]), n(n_) {}
    Exact(const uint8_t *src, size_t n_) : p(new uint8_t[n_]), n(n_) {
        if (n_) memcpy(p, src, n_);
    }
    ~Exact() { delete[] p; }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

// zlib's verdict: the stream ends, gives exactly isize bytes and leaves no input
static bool zlib_inflate(const uint8_t *in, size_t n, uint8_t *out, size_t isize) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) abort();
    uint8_t dummy = 0;
    z.next_in = n ? const_cast<uint8_t *>(in) : &dummy;
    z.avail_in = (uInt)n;
    z.next_out = isize ? out : &dummy;
    z.avail_out = (uInt)isize;
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.total_out == isize && z.avail_in == 0;
    inflateEnd(&z);
    return ok;
}

// the core with the trivial executor
static uint32_t core_inflate(const uint8_t *in, size_t n, uint8_t *out, size_t isize) {
    static Tables t;
    Decoder d;
    decoder_init(d, in, (uint32_t)n, (uint32_t)isize);
    uint32_t tok[64];
    uint32_t pos = 0;
    while (!decoder_done(d)) {
        const int m = next_tokens(d, t, tok, 64);
        for (int i = 0; i < m; ++i) {
            const uint32_t k = tok[i], len = tok_len(k);
            if (k & kTokMatch) {
                const uint32_t dist = tok_dist(k), start = pos - dist;
                for (uint32_t j = 0; j < len; ++j) out[pos + j] = out[start + j % dist];
            } else if (k & kTokStored) {
                memcpy(out + pos, in + d.stored_src, len);
            } else {
                out[pos] = (uint8_t)k;
            }
            pos += len;
        }
    }
    if (d.err == kOk && pos != isize) return 1000;  // cannot happen: the decoder checked it
    return d.err;
}

static uint32_t g_table[256];

// CRC by 64 slices with the bounds given (bounds[0] = 0 .. bounds[64] = n)
static uint32_t crc_by_slices(const uint8_t *p, const uint32_t *bounds) {
    uint32_t crc = 0;
    const uint32_t n = bounds[64];
    for (int l = 0; l < 64; ++l)
        crc ^= crc_shift(crc_slice(g_table, p + bounds[l], bounds[l + 1] - bounds[l]), n - bounds[l + 1]);
    return crc;
}
static uint32_t crc_even(const uint8_t *p, uint32_t n) {
    uint32_t b[65];
    const uint32_t per = (n + 63) / 64;
    for (int l = 0; l <= 64; ++l) b[l] = std::min<uint32_t>(n, (uint32_t)l * per);
    return crc_by_slices(p, b);
}

static std::vector<uint8_t> fastq_like(std::mt19937 &rng, size_t n) {
    std::string s;
    int id = 0;
    while (s.size() < n) {
        const int L = 30 + (int)(rng() % 200);
        s += "@read" + std::to_string(id++) + " x\n";
        for (int i = 0; i < L; ++i) s += "ACGTN"[rng() % 100 == 0 ? 4 : rng() % 4];
        s += "\n+\n";
        const char q = (char)('#' + rng() % 40);
        for (int i = 0; i < L; ++i) s += rng() % 8 ? q : (char)('#' + rng() % 40);
        s += "\n";
    }
    s.resize(n);
    return std::vector<uint8_t>(s.begin(), s.end());
}
static std::vector<uint8_t> fasta_like(std::mt19937 &rng, size_t n) {
    std::string s;
    int id = 0;
    while (s.size() < n) {
        s += ">contig" + std::to_string(id++) + "\n";
        const int lines = 1 + (int)(rng() % 40);
        const std::string unit = "ACGTTGCAAGGCTTAACCGT";
        for (int l = 0; l < lines; ++l) {
            for (int i = 0; i < 60; ++i) s += rng() % 5 ? unit[(size_t)(i + l) % unit.size()] : "ACGT"[rng() % 4];
            s += "\n";
        }
    }
    s.resize(n);
    return std::vector<uint8_t>(s.begin(), s.end());
}

static void round_trip(const std::vector<uint8_t> &text, const Setting &s, const char *what) {
    const std::vector<uint8_t> z = deflate_raw(text, s);
    Exact in(z.data(), z.size()), want(text.size()), got(text.size());
    CHECK(zlib_inflate(in.p, in.n, want.p, want.n), "%s/%s n=%zu: zlib rejects its own stream", what, s.name, text.size());
    const uint32_t e = core_inflate(in.p, in.n, got.p, got.n);
    CHECK(e == kOk, "%s/%s n=%zu: core status %u", what, s.name, text.size(), e);
    CHECK(text.empty() || memcmp(got.p, text.data(), text.size()) == 0, "%s/%s n=%zu: bytes differ", what, s.name,
          text.size());
    const uint32_t zc = (uint32_t)crc32(crc32(0, nullptr, 0), want.p, (uInt)want.n);
    CHECK(crc_even(got.p, (uint32_t)got.n) == zc, "%s/%s n=%zu: crc differs", what, s.name, text.size());
}

// is there a match token with these properties in the stream? (the hand-built texts must force them)
struct Seen {
    bool d1_258 = false, d32768 = false, ends_last = false;
};
static void scan_tokens(const std::vector<uint8_t> &z, size_t isize, Seen &seen) {
    static Tables t;
    Decoder d;
    decoder_init(d, z.data(), (uint32_t)z.size(), (uint32_t)isize);
    uint32_t tok[64], pos = 0;
    while (!decoder_done(d)) {
        const int m = next_tokens(d, t, tok, 64);
        for (int i = 0; i < m; ++i) {
            const uint32_t len = tok_len(tok[i]);
            if (tok[i] & kTokMatch) {
                if (tok_dist(tok[i]) == 1 && len == 258) seen.d1_258 = true;
                if (tok_dist(tok[i]) == 32768) seen.d32768 = true;
                if (pos + len == isize) seen.ends_last = true;
            }
            pos += len;
        }
    }
}

int main() {
    for (uint32_t i = 0; i < 256; ++i) g_table[i] = crc_table_entry(i);
    std::mt19937 rng(20240611);

    // ---- round trips
    const size_t sizes[] = {0, 1, 2, 63, 64, 65, 257, 258, 259, 4096, 65280};
    for (size_t n : sizes)
        for (int si = 0; si < kNSettings; ++si) {
            round_trip(fastq_like(rng, n), kSettings[si], "fastq");
            round_trip(fasta_like(rng, n), kSettings[si], "fasta");
        }
    {
        Seen seen;
        // one byte 600 times: dist 1, len 258, then a remainder; the match ends the text
        std::vector<uint8_t> run(600, 'I');
        // 1 KiB of noise, noise to 32768, the first 1 KiB again: distance 32768 exactly
        std::vector<uint8_t> far(40960);
        for (auto &c : far) c = (uint8_t)rng();
        memcpy(far.data() + 32768, far.data(), 1024);
        // a match that ends on the last output byte
        std::vector<uint8_t> tail(300);
        for (auto &c : tail) c = (uint8_t)rng();
        memcpy(tail.data() + 200, tail.data() + 20, 100);
        for (int si = 0; si < kNSettings; ++si) {
            round_trip(run, kSettings[si], "run");
            round_trip(far, kSettings[si], "far");
            round_trip(tail, kSettings[si], "tail");
            if (kSettings[si].level == 0) continue;
            scan_tokens(deflate_raw(run, kSettings[si]), run.size(), seen);
            scan_tokens(deflate_raw(far, kSettings[si]), far.size(), seen);
            scan_tokens(deflate_raw(tail, kSettings[si]), tail.size(), seen);
        }
        // zlib's deflate never looks back further than 32768 - 262, so the stream with the
        // longest distance is written by hand: a stored block of 32768 bytes, then a fixed block
        // with (len 258, dist 32768), (len 3, dist 32768) and the end-of-block code
        {
            std::vector<uint8_t> text(32768 + 261);
            for (size_t i = 0; i < 32768; ++i) text[i] = (uint8_t)rng();
            for (size_t i = 32768; i < text.size(); ++i) text[i] = text[i - 32768];
            std::vector<uint8_t> z = {0x00, 0x00, 0x80, 0xFF, 0x7F};
            z.insert(z.end(), text.begin(), text.begin() + 32768);
            uint64_t acc = 0;
            int nb = 0;
            auto put = [&](uint32_t v, int n, bool msb_first) {
                for (int i = 0; i < n; ++i) {
                    const uint32_t bit = msb_first ? (v >> (n - 1 - i)) & 1 : (v >> i) & 1;
                    acc |= (uint64_t)bit << nb;
                    if (++nb == 8) {
                        z.push_back((uint8_t)acc);
                        acc = 0;
                        nb = 0;
                    }
                }
            };
            put(1, 1, false);         // BFINAL
            put(1, 2, false);         // fixed codes
            put(0xC0 + 5, 8, true);   // 285: length 258
            put(29, 5, true);         // distances 24577..32768
            put(8191, 13, false);
            put(0x01, 7, true);       // 257: length 3
            put(29, 5, true);
            put(8191, 13, false);
            put(0, 7, true);          // end of block
            if (nb) z.push_back((uint8_t)acc);
            Exact in(z.data(), z.size()), want(text.size()), got(text.size());
            CHECK(zlib_inflate(in.p, in.n, want.p, want.n), "hand-built stream: zlib rejects it");
            CHECK(memcmp(want.p, text.data(), text.size()) == 0, "hand-built stream: not the text meant");
            const uint32_t e = core_inflate(in.p, in.n, got.p, got.n);
            CHECK(e == kOk && memcmp(got.p, text.data(), text.size()) == 0, "hand-built stream: core status %u", e);
            scan_tokens(z, text.size(), seen);
        }
        CHECK(seen.d1_258, "no dist 1 / len 258 match was produced");
        CHECK(seen.d32768, "no match at distance 32768 was produced");
        CHECK(seen.ends_last, "no match ended on the last byte");
    }

    // ---- CRC merge: 64 slices of unequal length (empty ones included) of a 4099-byte buffer
    {
        std::vector<uint8_t> buf(4099);
        for (auto &c : buf) c = (uint8_t)rng();
        const uint32_t want = (uint32_t)crc32(crc32(0, nullptr, 0), buf.data(), (uInt)buf.size());
        CHECK(crc_even(buf.data(), 4099) == want, "crc: even slices");
        for (int round = 0; round < 400; ++round) {
            uint32_t b[65];
            b[0] = 0;
            b[64] = 4099;
            for (int l = 1; l < 64; ++l) b[l] = rng() % 4100;
            if (round % 4 == 0)
                for (int l = 2; l < 64; l += 3) b[l] = b[l - 1];  // empty slices
            if (round == 1)
                for (int l = 1; l < 64; ++l) b[l] = 0;  // everything in the last slice
            if (round == 2)
                for (int l = 1; l < 64; ++l) b[l] = 4099;  // everything in the first
            std::sort(b, b + 65);
            CHECK(crc_by_slices(buf.data(), b) == want, "crc: split round %d", round);
        }
        // a suffix split at every byte: crc(A ++ B) from the two halves
        for (uint32_t cut = 0; cut <= 4099; cut += 1) {
            const uint32_t a = crc_slice(g_table, buf.data(), cut), c = crc_slice(g_table, buf.data() + cut, 4099 - cut);
            CHECK((crc_shift(a, 4099 - cut) ^ c) == want, "crc: cut %u", cut);
        }
    }

    // ---- mutation sweep: the verdict on a damaged stream is zlib's
    int accepted = 0, rejected = 0;
    int pair_count[kNSettings][3] = {};
    for (int m = 0; m < 2000; ++m) {
        const size_t n = 1 + rng() % 4000;
        // setting, kind and text are dealt independently: every kind meets every setting (18
        // pairs, 111 or 112 mutations each), the text type comes from the generator
        const Setting &s = kSettings[m % kNSettings];
        const int kind = (m / kNSettings) % 3;
        pair_count[m % kNSettings][kind]++;
        const std::vector<uint8_t> text = (rng() & 1) ? fasta_like(rng, n) : fastq_like(rng, n);
        std::vector<uint8_t> z = deflate_raw(text, s);
        if (kind == 0) {
            const size_t bit = rng() % (z.size() * 8);
            z[bit / 8] ^= (uint8_t)(1u << (bit % 8));
        } else if (kind == 1) {
            z[rng() % z.size()] = (uint8_t)rng();
        } else {
            z.resize(rng() % z.size());
        }
        Exact in(z.data(), z.size()), want(n), got(n);
        memset(want.p, 0, n);
        memset(got.p, 0, n);
        const bool zok = zlib_inflate(in.p, in.n, want.p, n);
        const uint32_t e = core_inflate(in.p, in.n, got.p, n);
        (zok ? accepted : rejected)++;
        CHECK(zok == (e == kOk), "mutation %d (%s kind %d n=%zu): zlib %s, core status %u", m, s.name, kind, n,
              zok ? "accepts" : "rejects", e);
        if (zok && e == kOk) {
            CHECK(memcmp(want.p, got.p, n) == 0, "mutation %d: accepted bytes differ", m);
            const uint32_t zc = (uint32_t)crc32(crc32(0, nullptr, 0), want.p, (uInt)n);
            CHECK(crc_even(got.p, (uint32_t)n) == zc, "mutation %d: crc differs", m);
            // the CRC is what tells a damaged but well-formed stream from the original
            const uint32_t oc = (uint32_t)crc32(crc32(0, nullptr, 0), text.data(), (uInt)n);
            CHECK((zc == oc) == (memcmp(want.p, text.data(), n) == 0), "mutation %d: crc blind to a change", m);
        }
    }
    printf("mutations: zlib accepted %d, rejected %d\n", accepted, rejected);
    CHECK(accepted >= 200 && rejected >= 200, "vacuous sweep: %d accepted, %d rejected", accepted, rejected);
    for (int si = 0; si < kNSettings; ++si)
        for (int k = 0; k < 3; ++k)
            CHECK(pair_count[si][k] >= 100, "setting %s met kind %d only %d times", kSettings[si].name, k, pair_count[si][k]);

    if (g_fail) {
        printf("inflate_core FAILED: %d checks\n", g_fail);
        return 1;
    }
    printf("inflate_core ok\n");
    return 0;
}
