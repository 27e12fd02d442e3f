// bgzf_inflate.hip — block-gzip (BGZF, htslib's bgzip) input inflated on the GPU.
//
// A BGZF file is a run of independent gzip members of at most 64 KiB of text each; a member's
// compressed length is in its header (extra subfield 'BC': BSIZE) and its text length in its
// trailer (ISIZE), so the members of a chunk and where their text goes are known without
// decoding anything. The host walks the members (BgzfReader), the compressed bytes cross PCIe,
// and k_bgzf_inflate decodes one member per wave into the text buffer the FASTQ / FASTA
// parsers read (fastq_ingest.hip).
//
//  k_bgzf_inflate  one wave per member, four members per workgroup. Lane 0 runs the token
//                  decoder of inflate_core.h (bit reader, canonical Huffman tables in LDS with
//                  a 10-bit first level, every bounds and validity check) and fills a batch of
//                  64 tokens in LDS; the wave then executes the batch: positions by a prefix
//                  sum over the token lengths, all literals at once (one byte per lane), the
//                  matches in order as 64-lane copies with source start + (i mod dist), which is
//                  right for overlapping matches. A match reads the member's own earlier output
//                  in global memory: stores are fenced (workgroup scope) before a match reads
//                  bytes written since the last fence. After the last block: ISIZE, the input
//                  used up, and CRC-32 over the produced bytes by lane slices merged with the
//                  x^(8n) mod P shift. One status word per member; the smallest failing index
//                  is reduced into one word the host reads per chunk.
//  k_bgzf_tail     one wave at the end of a file: trims trailing blank bytes, adds the final
//                  newline and the zero padding, as ChunkIo::prepare does on the host for
//                  uploaded text, and reports the chunk's length.
//
// Input the walk does not take declines (BgzfDecline): the ingest starts again with the host
// inflate stream. Corrupt data inside a member is an error, as it is for the host stream.
#include <zlib.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>

#include "inflate_core.h"
#include "internal.h"

namespace mcaat {
namespace {

constexpr int kWavesPerBlock = 4;

struct WaveLds {
    infl::Tables t;
    uint32_t tok[64];
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_bgzf_inflate(const uint8_t *z, const BgzfMember *tab, uint32_t n,
                                                                      uint8_t *out, uint32_t *status,
                                                                      uint32_t *first_bad) {
    __shared__ WaveLds lds[kWavesPerBlock];
    __shared__ uint32_t crc_tab[256];
    crc_tab[threadIdx.x] = infl::crc_table_entry(threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WaveLds &L = lds[wv];
    for (uint32_t m = blockIdx.x * kWavesPerBlock + wv; m < n; m += gridDim.x * kWavesPerBlock) {
        const uint32_t zoff = __builtin_amdgcn_readfirstlane(tab[m].zoff);
        const uint32_t zlen = __builtin_amdgcn_readfirstlane(tab[m].zlen);
        const uint32_t ooff = __builtin_amdgcn_readfirstlane(tab[m].ooff);
        const uint32_t olen = __builtin_amdgcn_readfirstlane(tab[m].olen);
        const uint8_t *in = z + zoff;
        uint8_t *o = out + ooff;
        infl::Decoder d;
        infl::decoder_init(d, in, zlen, olen);
        uint32_t pos = 0;     // bytes the executed tokens produced
        uint32_t synced = 0;  // o[0, synced) is written and visible to every lane
        for (;;) {
            uint32_t nt = 0, done = 0, ssrc = 0;
            if (lane == 0) {
                nt = (uint32_t)infl::next_tokens(d, L.t, L.tok, 64);
                done = infl::decoder_done(d) ? 1u : 0u;
                ssrc = d.stored_src;
            }
            nt = __builtin_amdgcn_readfirstlane(nt);
            done = __builtin_amdgcn_readfirstlane(done);
            ssrc = __builtin_amdgcn_readfirstlane(ssrc);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // ---- the batch: every token passed the decoder's checks
            const uint32_t t = lane < nt ? L.tok[lane] : 0u;
            const uint32_t mylen = lane < nt ? infl::tok_len(t) : 0u;
            uint32_t inc = mylen;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const uint32_t v = __shfl_up(inc, s);
                if ((int)lane >= s) inc += v;
            }
            const uint32_t excl = inc - mylen;
            const uint32_t total = __builtin_amdgcn_readlane(inc, 63);
            const bool copy = lane < nt && (t & (infl::kTokMatch | infl::kTokStored)) != 0;
            if (lane < nt && !copy) o[pos + excl] = (uint8_t)t;
            uint64_t mask = __ballot(copy);
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                const uint32_t tl = __builtin_amdgcn_readlane(t, l);
                const uint32_t p = pos + __builtin_amdgcn_readlane(excl, l);
                const uint32_t len = infl::tok_len(tl);
                if (tl & infl::kTokStored) {
                    for (uint32_t i = lane; i < len; i += 64) o[p + i] = in[ssrc + i];
                    continue;
                }
                const uint32_t dist = infl::tok_dist(tl), start = p - dist;
                if (start + (len < dist ? len : dist) > synced) {
                    __threadfence_block();  // the source holds bytes stored since the last fence
                    synced = p;
                }
                if (dist >= len) {
                    for (uint32_t i = lane; i < len; i += 64) o[p + i] = o[start + i];
                } else {
                    for (uint32_t i = lane; i < len; i += 64) o[p + i] = o[start + i % dist];
                }
            }
            pos += total;
            __builtin_amdgcn_wave_barrier();
            if (done) break;
        }
        uint32_t err = __builtin_amdgcn_readfirstlane(d.err);
        if (err == infl::kOk) {
            // CRC-32 over the produced bytes: a slice per lane, shifted by what follows it
            __threadfence_block();
            const uint32_t per = (olen + 63) / 64;
            const uint32_t a = min(olen, lane * per), b = min(olen, a + per);
            uint32_t c = infl::crc_slice(crc_tab, o + a, b - a);
            c = infl::crc_shift(c, olen - b);
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) c ^= __shfl_xor(c, s);
            const uint8_t *tr = in + zlen;  // the member's trailer: CRC-32, ISIZE
            const uint32_t want = (uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
            if (__builtin_amdgcn_readfirstlane(c) != __builtin_amdgcn_readfirstlane(want)) err = infl::kErrCrc;
        }
        if (lane == 0) {
            status[m] = err;
            if (err != infl::kOk) atomicMin(first_bad, m);
        }
    }
}

__device__ __forceinline__ bool blank(uint8_t c) { return c == '\n' || c == '\r' || c == ' ' || c == '\t'; }

// one wave; out_total[0]: the chunk's length after the trim and the final newline
__global__ __launch_bounds__(64) void k_bgzf_tail(uint8_t *text, uint32_t total, int trim, uint32_t *out_total) {
    const uint32_t lane = threadIdx.x;
    uint32_t t = total;
    if (trim) {
        while (t) {
            const bool solid = lane < t && !blank(text[t - 1 - lane]);
            const uint64_t mask = __ballot(solid);
            if (mask) {
                t -= (uint32_t)__builtin_ctzll(mask);
                break;
            }
            t = t > 64 ? t - 64 : 0;
        }
    }
    if (t && (trim || text[t - 1] != '\n')) {
        if (lane == 0) text[t] = '\n';
        ++t;
    }
    const uint32_t padded = (t + 63) / 64 * 64 + 64;
    for (uint32_t i = t + lane; i < padded; i += 64) text[i] = 0;
    if (lane == 0) out_total[0] = t;
}

uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }

// the BSIZE of the gzip member header at h (avail bytes readable): -1 no BGZF header, -2 more
// bytes needed (need says how many). FLG must be FEXTRA alone, as bgzip and every BGZF writer
// set it: a member that also carries FNAME, FCOMMENT or FHCRC is a valid gzip member but is not
// taken here (the file keeps the host inflate stream)
int bgzf_header(const uint8_t *h, size_t avail, size_t &need, uint32_t &xlen) {
    need = 12;
    if (avail < need) return -2;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4) return -1;  // CM 8, FEXTRA alone
    xlen = le16(h + 10);
    need = 12 + (size_t)xlen;
    if (avail < need) return -2;
    for (uint32_t i = 0; i + 4 <= xlen;) {  // subfield by subfield
        const uint8_t *f = h + 12 + i;
        const uint32_t slen = le16(f + 2);
        if (f[0] == 'B' && f[1] == 'C' && slen == 2 && i + 6 <= xlen) return (int)le16(f + 4);
        i += 4 + slen;
    }
    return -1;
}

}  // namespace

const char *bgzf_status_text(uint32_t s) {
    switch (s) {
        case infl::kErrBlockType: return "reserved DEFLATE block type";
        case infl::kErrStored: return "stored block lengths disagree";
        case infl::kErrCodeSet: return "invalid code lengths";
        case infl::kErrSymbol: return "invalid literal/length or distance code";
        case infl::kErrDistance: return "distance too far back";
        case infl::kErrInput: return "compressed data ends inside the stream";
        case infl::kErrOutput: return "more text than ISIZE";
        case infl::kErrLength: return "less text than ISIZE";
        case infl::kErrTrailing: return "unused bytes after the DEFLATE stream";
        case infl::kErrCrc: return "CRC mismatch";
        default: return "ok";
    }
}

bool is_bgzf_file(const char *path) {
    uint8_t h[12 + 65535];
    const int fd = open(path, O_RDONLY);
    if (fd < 0) throw Error(MCAAT_E_IO, std::string("cannot open ") + path);
    const ssize_t n = pread(fd, h, sizeof h, 0);
    close(fd);
    size_t need;
    uint32_t xlen;
    return n > 0 && bgzf_header(h, (size_t)n, need, xlen) >= 0;
}

BgzfReader::BgzfReader(const char *p) : path(p) {
    fd = open(p, O_RDONLY);
    if (fd < 0) throw Error(MCAAT_E_IO, std::string("cannot open ") + p);
    struct stat st;
    if (fstat(fd, &st) != 0) {
        close(fd);
        throw Error(MCAAT_E_IO, std::string("cannot stat ") + p);
    }
    fsize = (uint64_t)st.st_size;
    posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
}
BgzfReader::~BgzfReader() {
    if (fd >= 0) close(fd);
}

BgzfChunk BgzfReader::fill(uint8_t *dst, size_t CH, BgzfMember *tab, uint32_t *mstart, uint32_t max_members) {
    BgzfChunk ck;
    ck.file_off = off;
    ck.first_index = index;
    size_t have = 0, pos = 0;
    // at least `upto` bytes of the chunk in dst, unless the file or the chunk ends first
    auto ensure = [&](size_t upto) {
        while (have < upto && have < CH && off + have < fsize) {
            const size_t want = (size_t)std::min<uint64_t>(std::min<size_t>(kStep, CH - have), fsize - off - have);
            const ssize_t r = pread(fd, dst + have, want, (off_t)(off + have));
            if (r < 0) throw Error(MCAAT_E_IO, "read error in " + path);
            if (r == 0) throw BgzfDecline("file shrank: " + path);
            have += (size_t)r;
        }
        return have >= upto;
    };
    for (;;) {
        if (off + pos == fsize) {
            ck.eof = true;
            break;
        }
        size_t need = 12;
        uint32_t xlen = 0;
        int bsize;
        for (;;) {
            bsize = bgzf_header(dst + pos, have > pos ? have - pos : 0, need, xlen);
            if (bsize != -2) break;
            if (!ensure(pos + need)) break;
        }
        if (bsize == -2) {
            if (off + have == fsize) throw BgzfDecline("the file ends inside a member header: " + path);
            if (pos == 0) throw BgzfDecline("a member header larger than the chunk: " + path);
            break;  // the chunk is full
        }
        if (bsize < 0) throw BgzfDecline("a member without the BGZF subfield: " + path);
        const size_t msize = (size_t)bsize + 1;
        if (msize < (size_t)xlen + 20) throw BgzfDecline("BSIZE below the header and trailer: " + path);
        if (off + pos + msize > fsize) throw BgzfDecline("BSIZE points past the end of the file: " + path);
        if (msize > CH) throw BgzfDecline("a member larger than the chunk: " + path);
        if (pos + msize > CH) break;
        if (!ensure(pos + msize)) throw BgzfDecline("short read: " + path);
        const uint32_t isize = le32(dst + pos + msize - 4);
        // 64 KiB is the format's bound; the first member of a file is inflated up to that far
        // in front of the text buffer (leading blank bytes)
        if (isize > 65536 || isize > CH) throw BgzfDecline("a member with more text than a chunk holds: " + path);
        if (ck.text + isize > CH || ck.n_members == max_members) break;
        mstart[ck.n_members] = (uint32_t)pos;
        tab[ck.n_members++] = BgzfMember{(uint32_t)(pos + 12 + xlen), (uint32_t)(msize - xlen - 20), (uint32_t)ck.text, isize};
        ck.text += isize;
        pos += msize;
    }
    ck.zbytes = pos;
    off += pos;
    index += ck.n_members;
    return ck;
}

bool bgzf_host_inflate(const uint8_t *z, const BgzfMember &m, std::vector<uint8_t> &text) {
    text.resize(m.olen);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    uint8_t dummy = 0;
    zs.next_in = const_cast<uint8_t *>(z + m.zoff);
    zs.avail_in = m.zlen;
    zs.next_out = m.olen ? text.data() : &dummy;
    zs.avail_out = m.olen;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == m.olen && zs.avail_in == 0;
    inflateEnd(&zs);
    return ok && (uint32_t)crc32(crc32(0, nullptr, 0), text.data(), m.olen) == le32(z + m.zoff + m.zlen);
}

int bgzf_sniff(const char *path) {
    try {
        BgzfReader rd(path);
        std::vector<uint8_t> z(65536 + 64), text;
        for (;;) {
            BgzfMember m;
            uint32_t at;
            const BgzfChunk ck = rd.fill(z.data(), 65536, &m, &at, 1);
            if (ck.n_members) {
                if (!bgzf_host_inflate(z.data(), m, text)) return -2;
                for (uint8_t c : text)
                    if (c != '\n' && c != '\r' && c != ' ' && c != '\t') return c;
            }
            if (ck.eof) return -1;
        }
    } catch (const BgzfDecline &) {
        return -2;
    }
}

void bgzf_inflate_launch(hipStream_t s, const uint8_t *z, const BgzfMember *tab, uint32_t n, uint8_t *out,
                         uint32_t *status, uint32_t *first_bad) {
    if (!n) return;
    const unsigned blocks = std::min<unsigned>((n + kWavesPerBlock - 1) / kWavesPerBlock, 16384u);
    launch_at(s, dim3(blocks), dim3(64 * kWavesPerBlock), k_bgzf_inflate, z, tab, n, out, status, first_bad);
}

void bgzf_tail_launch(hipStream_t s, uint8_t *text, uint32_t total, bool trim, uint32_t *out_total) {
    launch_at(s, dim3(1), dim3(64), k_bgzf_tail, text, total, trim ? 1 : 0, out_total);
}

}  // namespace mcaat
