// fastq_ingest.hip — FASTQ(.gz/.bz2) -> 2-bit read library in HBM.
//
// Replaces SDBGBuild::BuildLib / SequenceLibCollection::Build (sdbg_build.cpp:82-115, the
// MEGAHIT buildlib step) for FASTQ inputs, and builds in the same pass the mapping view that
// get_reads re-parses the FASTQ for (reads.cpp:20-52, 88-130). The host only moves bytes: a
// reader task fills pinned chunks (zlib / libbz2 inflate .gz / .bz2; plain files are copied straight into
// the chunk by four pread() threads) while the GPU parses the previous chunk:
//
//  1. k_fq_nlcount   one lane per 64-byte segment (4 x 16-B loads): number of '\n' bytes
//                    (SWAR zero-byte count); exclusive scan -> line index per segment.
//  2. k_fq_nlpos     the same segments again: position of every '\n' (line starts).
//                    Records are 4 lines (header '@', sequence, '+', quality); the bytes
//                    after the last complete record carry over to the next chunk.
//  3. k_fq_records   one lane per record: header check, sequence bounds ('\r' stripped),
//                    ACGT base count and maximal-run count (counting view: non-ACGT symbols
//                    split a read), sequence length (mapping view); three exclusive scans.
//  4. k_fq_emit      one lane per record: packs the counting view (runs -> reads, global
//                    read offsets) and the mapping view (second file reversed and
//                    complemented; A/C/G -> 0/1/2, anything else -> 3, reads.cpp:44-52) into
//                    the growing device streams; words shared with a neighbouring record are
//                    merged with atomicOr, whole words are stored.
//
// Bytes per chunk byte (roofline, HBM): ~2.5 B read (two newline passes + the record
// passes) + 0.25 B per sequence byte written per view. The ingest is PCIe/host-read bound
// (text crosses PCIe once); the parse runs at HBM speed.
//
// FASTA (ingest_fasta) shares the source, the chunks, the copy stream and the newline passes
// (ChunkIo), and deals its work by line, not by record: a wrapped contig is one record of
// tens of thousands of lines.
//
//  3'. k_fa_lines    one lane per line: class (header '>' / sequence / empty), trimmed length,
//                    ACGT count, run starts, whether the first and the last symbol are ACGT;
//                    a sequence line that starts with '@' or '+' declines the input (kseq
//                    reads FASTQ grammar there: the host reader takes it).
//      scans         headers before a line (its record), the nearest non-empty line before it
//                    (max-scan), and after k_fa_link base, read and symbol offsets.
//      k_fa_link     a run open at a line's end continues in the record's next non-empty line
//                    (one read, also across empty lines; never across a header).
//  4'. k_fa_emit     one lane per line: both views packed as above; a record of a later file
//                    is reversed and complemented over the whole concatenated record, so a
//                    line writes backwards from its mirrored place in the record.
//
// A chunk is consumed up to the start of its last header line. Records above the carry
// reserve, FASTA mixed with FASTQ and kseq's FASTQ grammar inside a FASTA file stay on the
// host parser in capi.hip. A very long unwrapped line is parsed by one lane (correct, slow).
#include <hipcub/hipcub.hpp>
#include <zlib.h>

#include <algorithm>
#include <cstring>
#include <atomic>
#include <future>
#include <memory>
#include <string>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <thread>

#include "fasta_split.h"
#include "internal.h"

namespace mcaat {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kSeg = 64;  // bytes per lane in the newline passes

// zero-byte mask of a 32-bit word: bit 7 of each byte that is zero (exact, no carries)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t v) {
    const uint32_t y = (v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(y | v | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t nl_mask(uint32_t v) { return zero_bytes(v ^ 0x0A0A0A0Au); }

__global__ void k_fq_nlcount(const uint8_t *buf, uint32_t nseg, uint32_t *cnt) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += stride) {
        const uint4 *p = reinterpret_cast<const uint4 *>(buf + (size_t)s * kSeg);
        uint32_t c = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = p[q];
            c += __popc(nl_mask(v.x)) + __popc(nl_mask(v.y)) + __popc(nl_mask(v.z)) + __popc(nl_mask(v.w));
        }
        cnt[s] = c;
    }
}

__global__ void k_fq_nlpos(const uint8_t *buf, uint32_t nseg, const uint32_t *first, uint32_t *nl) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += stride) {
        const uint4 *p = reinterpret_cast<const uint4 *>(buf + (size_t)s * kSeg);
        uint32_t o = first[s];
        const uint32_t base = s * kSeg;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = p[q];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t m = nl_mask(w[j]);
                while (m) {
                    const int b = __builtin_ctz(m) >> 3;
                    nl[o++] = base + 16 * q + 4 * j + b;
                    m &= m - 1;
                }
            }
        }
    }
}

// counting-view code: A/C/G/T in either case, -1 splits the read (capi.hip Packer)
__device__ __forceinline__ int count_code(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}
// mapping-view code (k_mer_to_node_id, reads.cpp:44-52)
__device__ __forceinline__ uint32_t map_code(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }
// complement then code (reverse_pair_ends_sequence, reads.cpp:20-31: only A/C/G/T change)
__device__ __forceinline__ uint32_t map_code_rc(uint8_t c) { return c == 'T' ? 0 : c == 'G' ? 1 : c == 'C' ? 2 : 3; }

// a lane's sequential byte readers over the chunk (4-byte aligned loads instead of one load
// per byte; the chunk buffer is 256-B aligned and padded, so reading up to 3 bytes past the
// end is in bounds)
struct Fwd {
    const uint32_t *w;
    uint32_t cur;
    int avail;
    __device__ Fwd(const uint8_t *buf, uint32_t pos) {
        w = reinterpret_cast<const uint32_t *>(buf + (pos & ~3u));
        cur = *w++ >> (8 * (pos & 3));
        avail = 4 - (int)(pos & 3);
    }
    __device__ __forceinline__ uint8_t next() {
        if (!avail) {
            cur = *w++;
            avail = 4;
        }
        const uint8_t c = (uint8_t)cur;
        cur >>= 8;
        --avail;
        return c;
    }
};
struct Bwd {  // from pos downwards
    const uint32_t *w;
    uint32_t cur;
    int idx;
    __device__ Bwd(const uint8_t *buf, uint32_t pos) {
        w = reinterpret_cast<const uint32_t *>(buf + (pos & ~3u));
        cur = *w;
        idx = (int)(pos & 3);
    }
    __device__ __forceinline__ uint8_t next() {
        if (idx < 0) {
            cur = *--w;
            idx = 3;
        }
        return (uint8_t)(cur >> (8 * idx--));
    }
};

enum : uint32_t { kBadHeader = 1, kDiffer = 2 };

// per record: sequence start, length, counting-view bases and runs
__global__ void k_fq_records(const uint8_t *buf, const uint32_t *nl, uint32_t n_rec, uint32_t *sbeg, uint32_t *slen,
                             uint32_t *nbase, uint32_t *nrun, uint32_t *flags) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t fl = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += stride) {
        const uint32_t h = r ? nl[4 * r - 1] + 1 : 0;
        if (buf[h] != '@') fl |= kBadHeader;
        const uint32_t s = nl[4 * r] + 1;
        uint32_t e = nl[4 * r + 1];
        if (e > s && buf[e - 1] == '\r') --e;
        // '+' line, and a quality line as long as the sequence: otherwise not 4-line FASTQ
        // (wrapped lines), which the host kseq-style reader takes
        const uint32_t qs = nl[4 * r + 2] + 1;
        uint32_t qe = nl[4 * r + 3];
        if (qe > qs && buf[qe - 1] == '\r') --qe;
        if (buf[nl[4 * r + 1] + 1] != '+' || qe - qs != e - s) fl |= kBadHeader;
        uint32_t bases = 0, runs = 0;
        bool in = false, differ = false;
        Fwd rd(buf, s);
        for (uint32_t i = s; i < e; ++i) {
            const uint8_t c = rd.next();
            if (count_code(c) >= 0) {
                ++bases;
                runs += !in;
                in = true;
            } else {
                in = false;
            }
            differ |= c != 'A' && c != 'C' && c != 'G' && c != 'T';
        }
        // the mapping view equals the counting view only if this record is one ACGT run
        if (differ || runs != 1) fl |= kDiffer;
        sbeg[r] = s;
        slen[r] = e - s;
        nbase[r] = bases;
        nrun[r] = runs;
    }
    if (fl) atomicOr(flags, fl);
}

// appends 2-bit symbols at consecutive stream positions; a word this lane does not fill
// completely may be shared with another record and is merged with atomicOr
struct PackWriter {
    uint64_t *out;
    uint64_t pos;
    uint64_t acc = 0;
    bool partial;
    __device__ PackWriter(uint64_t *o, uint64_t p) : out(o), pos(p), partial((p & 31) != 0) {}
    __device__ __forceinline__ void put(uint32_t b) {
        acc |= (uint64_t)b << (2 * (pos & 31));
        if ((++pos & 31) == 0) {
            uint64_t *w = out + ((pos - 1) >> 5);
            if (partial) {
                if (acc) atomicOr((unsigned long long *)w, (unsigned long long)acc);
            } else {
                *w = acc;
            }
            acc = 0;
            partial = false;
        }
    }
    __device__ __forceinline__ void finish() {
        if ((pos & 31) && acc) atomicOr((unsigned long long *)(out + (pos >> 5)), (unsigned long long)acc);
    }
};

__global__ void k_fq_emit(const uint8_t *buf, uint32_t n_rec, const uint32_t *sbeg, const uint32_t *slen,
                          const uint32_t *boff, const uint32_t *roff, const uint32_t *qoff, uint64_t g_base,
                          uint64_t g_read, uint64_t g_qbase, uint64_t g_rec, int reverse, uint64_t *packed,
                          uint64_t *offsets, uint64_t *qpacked, uint64_t *qoffsets) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += stride) {
        const uint32_t sb = sbeg[r];
        const uint32_t L = slen[r];
        // counting view: maximal ACGT runs are reads
        PackWriter pw(packed, g_base + boff[r]);
        uint64_t ri = g_read + roff[r];
        bool in = false;
        Fwd rd(buf, sb);
        for (uint32_t i = 0; i < L; ++i) {
            const int b = count_code(rd.next());
            if (b >= 0) {
                pw.put((uint32_t)b);
                in = true;
            } else if (in) {
                offsets[1 + ri++] = pw.pos;
                in = false;
            }
        }
        if (in) offsets[1 + ri] = pw.pos;
        pw.finish();
        // mapping view: one entry per record
        if (qpacked) {
            PackWriter qw(qpacked, g_qbase + qoff[r]);
            if (!reverse) {
                Fwd rq(buf, sb);
                for (uint32_t i = 0; i < L; ++i) qw.put(map_code(rq.next()));
            } else if (L) {
                Bwd rq(buf, sb + L - 1);
                for (uint32_t i = 0; i < L; ++i) qw.put(map_code_rc(rq.next()));
            }
            qw.finish();
            qoffsets[1 + g_rec + r] = qw.pos;
        }
    }
}

// ---- FASTA: work dealt by line (a wrapped contig is one record of many thousand lines) ----

enum : uint32_t { kLHeader = 1, kLFirst = 2, kLLast = 4, kLCont = 8 };  // per-line flags

// per line: class (header / sequence / empty), trimmed length, ACGT count, run starts, whether
// its first and last symbols are ACGT. key[i] orders the non-empty lines for the max-scan that
// hands every line its nearest non-empty predecessor: (i + 1) << 1 | last-symbol-is-ACGT, 0 for
// an empty line. meta[0]: flags; meta[1], meta[2]: index + 1 and start of the last header line.
__global__ void k_fa_lines(const uint8_t *buf, const uint32_t *nl, uint32_t n_lines, uint32_t *len, uint32_t *nbase,
                           uint32_t *nrun, uint32_t *lflag, uint32_t *hflag, uint32_t *key, uint32_t *meta) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t fl = 0, h_idx = 0, h_pos = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride) {
        const uint32_t s = i ? nl[i - 1] + 1 : 0;
        uint32_t e = nl[i];
        if (e > s && buf[e - 1] == '\r') --e;
        const uint8_t c0 = buf[s];
        if (c0 == '>') {  // skipped whole: '>', '@' and '+' inside it mean nothing
            len[i] = nbase[i] = nrun[i] = 0;
            lflag[i] = kLHeader;
            hflag[i] = 1;
            key[i] = (i + 1) << 1;
            h_idx = i + 1;
            h_pos = s;
            continue;
        }
        // kseq starts a FASTQ-style record at '@' and a quality block at '+': not pure FASTA. A
        // chunk begins at a header line (line 0), or the file's first byte was no '>'.
        if (c0 == '@' || c0 == '+' || i == 0) fl |= kBadHeader;
        uint32_t bases = 0, runs = 0;
        bool in = false, first = false;
        Fwd rd(buf, s);
        for (uint32_t j = s; j < e; ++j) {
            const uint8_t c = rd.next();
            if (count_code(c) >= 0) {
                ++bases;
                runs += !in;
                in = true;
                first |= j == s;
            } else {
                in = false;
            }
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T') fl |= kDiffer;
        }
        len[i] = e - s;
        nbase[i] = bases;
        nrun[i] = runs;
        lflag[i] = (first ? kLFirst : 0) | (in ? kLLast : 0);
        hflag[i] = 0;
        key[i] = e > s ? ((i + 1) << 1) | (in ? 1u : 0u) : 0u;
    }
    if (fl) atomicOr(meta, fl);
    if (h_idx) {
        atomicMax(meta + 1, h_idx);
        atomicMax(meta + 2, h_pos);
    }
}

// A run that is open at the end of a record's line continues in the record's next non-empty
// line when that begins with an ACGT symbol: it is one read, so the continuing line has one run
// start less. Never across a header (a header's key has the ACGT bit clear). hdr[r] is the line
// of record r's header, hdr[n_rec] the line count.
__global__ void k_fa_link(uint32_t n_lines, const uint32_t *prev, const uint32_t *recx, uint32_t *nrun, uint32_t *lflag,
                          uint32_t *hdr) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n_lines; i += stride) {
        if (i == n_lines) {
            hdr[recx[i]] = i;
            continue;
        }
        const uint32_t lf = lflag[i];
        if (lf & kLHeader) {
            hdr[recx[i]] = i;
        } else if ((lf & kLFirst) && (prev[i] & 1)) {
            nrun[i] -= 1;
            lflag[i] = lf | kLCont;
        }
    }
}

// one lane per line. A sequence line packs its symbols into both views: the counting view at
// its base offset (a read's start offset is written where its run starts: offsets[i] is both
// the end of read i-1 and the start of read i; the host writes the last entry), the mapping
// view at its offset in the record, from the record's far end backwards when the file's records
// are reversed and complemented. A header line writes its record's end offset.
__global__ void k_fa_emit(const uint8_t *buf, const uint32_t *nl, uint32_t n_lines, const uint32_t *len,
                          const uint32_t *lflag, const uint32_t *recx, const uint32_t *hdr, const uint32_t *boff,
                          const uint32_t *roff, const uint32_t *qoff, uint64_t g_base, uint64_t g_read, uint64_t g_qbase,
                          uint64_t g_rec, int reverse, uint64_t *packed, uint64_t *offsets, uint64_t *qpacked,
                          uint64_t *qoffsets, uint32_t *meta) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t fl = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += stride) {
        const uint32_t lf = lflag[i];
        if (lf & kLHeader) {
            const uint32_t r = recx[i], next = hdr[r + 1];
            if (roff[next] - roff[i] != 1) fl |= kDiffer;  // not exactly one run
            qoffsets[1 + g_rec + r] = g_qbase + qoff[next];
            continue;
        }
        const uint32_t L = len[i];
        if (!L) continue;
        const uint32_t sb = nl[i - 1] + 1;  // line 0 is a header
        PackWriter pw(packed, g_base + boff[i]);
        uint64_t ri = g_read + roff[i];
        bool in = (lf & kLCont) != 0;
        Fwd rd(buf, sb);
        for (uint32_t j = 0; j < L; ++j) {
            const int b = count_code(rd.next());
            if (b >= 0) {
                if (!in) offsets[ri++] = pw.pos;
                in = true;
                pw.put((uint32_t)b);
            } else {
                in = false;
            }
        }
        pw.finish();
        if (!reverse) {
            PackWriter qw(qpacked, g_qbase + qoff[i]);
            Fwd rq(buf, sb);
            for (uint32_t j = 0; j < L; ++j) qw.put(map_code(rq.next()));
            qw.finish();
        } else {
            const uint32_t r = recx[i] - 1;  // headers before this line, less one
            const uint32_t r0 = qoff[hdr[r]], r1 = qoff[hdr[r + 1]];
            PackWriter qw(qpacked, g_qbase + r1 - (qoff[i] - r0) - L);
            Bwd rq(buf, sb + L - 1);
            for (uint32_t j = 0; j < L; ++j) qw.put(map_code_rc(rq.next()));
            qw.finish();
        }
    }
    if (fl) atomicOr(meta, fl);
}

__global__ void k_fq_fixed_len(const uint64_t *off, uint64_t n, uint64_t L, uint32_t *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool b = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) b |= off[i] != i * L;
    if (b) atomicOr(bad, 1u);
}

void scan_u32(mcaat_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n, DevBuf<uint8_t> &tmp) {
    size_t need = 0;
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (size_t)n, ctx->stream));
    if (need > tmp.bytes()) tmp.alloc(need);
    HIP_OK(hipcub::DeviceScan::ExclusiveSum(tmp.p, need, in, out, (size_t)n, ctx->stream));
}

// grows a zero-filled device stream, keeping its first `used` elements
void grow(mcaat_ctx *ctx, DevBuf<uint64_t> &b, uint64_t used, uint64_t need) {
    if (need <= b.n) return;
    DevBuf<uint64_t> nb(std::max<uint64_t>(need, b.n + b.n / 2));
    HIP_OK(hipMemsetAsync(nb.p, 0, nb.bytes(), ctx->stream));
    if (used) HIP_OK(hipMemcpyAsync(nb.p, b.p, 8 * used, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    b = std::move(nb);
}

// Source of input bytes: InStream for compressed files (one inflate stream), parallel pread()
// for plain files (one thread copies page-cache data at ~13 GB/s; eight reach ~38 GB/s end to end).
struct Source {
    std::unique_ptr<InStream> z;  // gzip / bzip2
    std::unique_ptr<BgzfReader> bgzf;  // block gzip: whole members, inflated on the device
    int fd = -1;
    uint64_t off = 0;
    const char *path;
    uint64_t end = ~0ULL;  // plain files: read [off, end) only (a rank's part of the file)
    // [begin, end) of a plain file; a compressed file is read whole (begin = 0, end = ~0)
    explicit Source(const char *p, uint64_t begin = 0, uint64_t end_ = ~0ULL, bool device_inflate = false)
        : off(begin), path(p), end(end_) {
        if (is_compressed_file(p)) {
            if (begin != 0 || end_ != ~0ULL) throw Error(MCAAT_E_INVALID, "a compressed input cannot be split");
            if (device_inflate && is_bgzf_file(p)) bgzf.reset(new BgzfReader(p));
            else z.reset(new InStream(p));
            return;
        }
        fd = open(p, O_RDONLY);
        if (fd < 0) throw Error(MCAAT_E_IO, std::string("cannot open ") + p);
        posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    }
    ~Source() {
        if (fd >= 0) close(fd);
    }
    Source(const Source &) = delete;
    Source &operator=(const Source &) = delete;
    size_t read(uint8_t *dst, size_t n) {
        if (z) return z->read(dst, n);
        n = (size_t)std::min<uint64_t>(n, end > off ? end - off : 0);
        if (!n) return 0;
        // 8 by default: the C3 FASTQ (92 GB in tmpfs) reads at 38 GB/s end to end with 8 or 16
        // threads, 12.6 GB/s with 4; MCAAT_FASTQ_THREADS overrides (1..32)
        static const int kThreads = [] {
            const char *e = getenv("MCAAT_FASTQ_THREADS");
            const int v = e ? atoi(e) : 8;
            return v < 1 ? 1 : v > 32 ? 32 : v;
        }();
        const size_t piece = (n + kThreads - 1) / kThreads;
        size_t got[32] = {};
        bool err[32] = {};
        auto job = [&](int t) {
            const size_t a = std::min(n, t * piece), b = std::min(n, a + piece);
            size_t g = 0;
            while (a + g < b) {
                const ssize_t r = pread(fd, dst + a + g, b - a - g, (off_t)(off + a + g));
                if (r < 0) { err[t] = true; break; }
                if (r == 0) break;
                g += (size_t)r;
            }
            got[t] = g;
        };
        std::thread th[31];
        for (int t = 1; t < kThreads; ++t) th[t - 1] = std::thread(job, t);
        job(0);
        for (int t = 1; t < kThreads; ++t) th[t - 1].join();
        size_t total = 0;
        for (int t = 0; t < kThreads; ++t) {
            if (err[t]) throw Error(MCAAT_E_IO, std::string("read error in ") + path);
            const size_t a = std::min(n, t * piece), b = std::min(n, a + piece);
            total += got[t];
            if (got[t] < b - a) break;  // end of file inside piece t: later pieces read nothing
        }
        off += total;
        return total;
    }
};

bool is_space(uint8_t c) { return c == '\n' || c == '\r' || c == ' ' || c == '\t'; }

}  // namespace

size_t fastq_chunk_bytes() {
    if (const char *e = getenv("MCAAT_FASTQ_CHUNK")) {
        const long long v = atoll(e);
        // chunk positions are 32-bit: keep chunk + carry reserve well below 4 GiB
        if (v >= 256) return (size_t)std::min<long long>(v, 1LL << 30);
    }
    return size_t(256) << 20;
}

namespace {

using Ranges = std::vector<std::pair<uint64_t, uint64_t>>;

// The two views of the read library as growing device streams, and what they hold so far.
struct Library {
    DevBuf<uint64_t> packed, offsets, qpacked, qoffsets;
    uint64_t n_bases = 0, n_reads = 0, q_bases = 0, n_rec = 0;
    std::vector<uint64_t> file_records;
    // stream capacity estimate from the input sizes (grown on demand)
    Library(mcaat_ctx *ctx, const char *const *files, int n_files, const Ranges *ranges) {
        uint64_t est = 0;
        for (int i = 0; i < n_files; ++i) {
            struct stat st;
            const std::string path(files[i]);
            const bool gz = (path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0) ||
                            (path.size() > 4 && path.compare(path.size() - 4, 4, ".bz2") == 0);
            if (stat(files[i], &st) == 0) {
                uint64_t sz = (uint64_t)st.st_size;
                if (ranges) sz = std::min(sz, (*ranges)[i].second) - std::min(sz, (*ranges)[i].first);
                est += sz * (gz ? 4 : 1);
            }
        }
        packed.alloc(est / 64 + 1024);
        offsets.alloc(est / 256 + 1024);
        qpacked.alloc(est / 64 + 1024);
        qoffsets.alloc(est / 256 + 1024);
        for (auto *b : {&packed, &offsets, &qpacked, &qoffsets}) HIP_OK(hipMemsetAsync(b->p, 0, b->bytes(), ctx->stream));
    }
    // room for cb bases in cr reads and cq symbols in nrec records more
    void reserve(mcaat_ctx *ctx, uint32_t cb, uint32_t cr, uint32_t cq, uint32_t nrec) {
        grow(ctx, packed, (n_bases + 31) / 32 + 1, (n_bases + cb + 31) / 32 + 17);
        grow(ctx, offsets, n_reads + 1, n_reads + cr + 2);
        grow(ctx, qpacked, (q_bases + 31) / 32 + 1, (q_bases + cq + 31) / 32 + 17);
        grow(ctx, qoffsets, n_rec + 1, n_rec + nrec + 2);
    }
};

// The host side of a chunked text ingest, shared by the FASTQ and the FASTA parser: two pinned
// chunks that a reader task fills, their device copies uploaded on a copy stream while the
// previous chunk is parsed, the newline passes, and the loop over files and chunks.
struct ChunkIo {
    mcaat_ctx *ctx;
    const size_t CH;   // new bytes per chunk
    const size_t R;    // carry reserve: the longest record that fits
    const size_t cap;  // bytes of a chunk buffer
    uint8_t *hb[2];
    DevBuf<uint8_t> dbufs[2];
    struct CopyStream {  // uploads overlap the parse of the previous chunk
        hipStream_t s = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};    // upload into dbufs[x] complete
        hipEvent_t done[2] = {nullptr, nullptr};  // the parse of dbufs[x] complete (buffer free)
        CopyStream() {
            HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            for (auto &e : ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            for (auto &e : done) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        ~CopyStream() {
            if (s) (void)hipStreamSynchronize(s);
            for (auto &e : ev)
                if (e) (void)hipEventDestroy(e);
            for (auto &e : done)
                if (e) (void)hipEventDestroy(e);
            if (s) (void)hipStreamDestroy(s);
        }
    } cs;
    DevBuf<uint32_t> cnt, first, nl;
    DevBuf<uint32_t> meta;
    DevBuf<uint8_t> tmp;
    uint32_t *hmeta = nullptr;  // pinned words for the counters read back per chunk

    // ---- block-gzip files (device_inflate): the reader fills hb[x] + R with whole members, they
    // are staged in zbuf[x] and k_bgzf_inflate writes their text behind the carry in dbufs[x].
    // A file's first member may begin with blank bytes that are not part of the chunk: it is
    // inflated up to kFront bytes in front of the text, so a chunk's text begins kFront bytes
    // into its buffer (uploaded text too: one layout).
    static constexpr size_t kFront = 65536;
    static constexpr uint32_t kMaxMembers = 1u << 16;  // per chunk: 1 MiB of table
    const bool device_inflate;                         // knob gz.gpu
    DevBuf<uint8_t> zbuf[2];
    DevBuf<BgzfMember> dtab[2];
    DevBuf<uint32_t> dstat[2];  // [0] smallest failing member, [1] text length at the end of the file, [2 + i] status
    BgzfMember *htab[2] = {nullptr, nullptr};  // pinned (ctx->bgzf_pinned)
    uint32_t *hstat = nullptr;                 // pinned (the same block): words [0], [1] of dstat[x] at hstat + 2 x
    std::vector<uint32_t> mstart[2];           // a member's offset in the chunk's compressed bytes
    struct Inflate {                           // the inflate of chunk x, queued and not yet waited for
        bool active = false, eof = false;
        std::unique_ptr<KernelTimer> kt;
        BgzfChunk ck;
        uint32_t dropped = 0;  // blank leading members the host inflated itself
    } inflate[2];
    uint8_t *text(int x) const { return dbufs[x].p + kFront; }

    explicit ChunkIo(mcaat_ctx *c, bool device_inflate_ = false)
        : ctx(c), CH(fastq_chunk_bytes()), R(std::max<size_t>(CH / 4, 4096)), cap(R + CH + 2 * kSeg),
          device_inflate(device_inflate_) {
        if (ctx->pinned_bytes < cap) {
            for (auto *&p : ctx->pinned) {
                if (p) (void)hipHostFree(p);
                p = nullptr;
            }
            ctx->pinned_bytes = 0;
            for (auto *&p : ctx->pinned) HIP_OK(hipHostMalloc((void **)&p, cap, hipHostMallocDefault));
            ctx->pinned_bytes = cap;
        }
        hb[0] = ctx->pinned[0];
        hb[1] = ctx->pinned[1];
        dbufs[0].alloc(kFront + cap);
        dbufs[1].alloc(kFront + cap);
        for (auto &e : cs.done) HIP_OK(hipEventRecord(e, ctx->stream));
        const uint64_t max_seg = cap / kSeg + 1;
        cnt.alloc(max_seg + 1);
        first.alloc(max_seg + 1);
        nl.alloc(cap + 16);  // every byte may be a newline
        meta.alloc(8);
        tmp.alloc(1 << 20);
        HIP_OK(hipHostMalloc((void **)&hmeta, 64, hipHostMallocDefault));
    }
    ~ChunkIo() {
        (void)hipStreamSynchronize(cs.s);  // an error unwinding: the staging buffers may be in use
        if (hmeta) (void)hipHostFree(hmeta);
    }
    ChunkIo(const ChunkIo &) = delete;
    ChunkIo &operator=(const ChunkIo &) = delete;

    // the staging buffers and tables of the device inflate, at the first block-gzip file. The
    // pinned tables and status words are one block kept in the context between calls (pinning
    // costs more than a small file's ingest); the device buffers come from the caching arena
    void ensure_inflate() {
        if (hstat) return;
        const size_t tab_bytes = sizeof(BgzfMember) * kMaxMembers;
        if (!ctx->bgzf_pinned) HIP_OK(hipHostMalloc((void **)&ctx->bgzf_pinned, 2 * tab_bytes + 64, hipHostMallocDefault));
        hstat = (uint32_t *)(ctx->bgzf_pinned + 2 * tab_bytes);
        for (int x = 0; x < 2; ++x) {
            htab[x] = (BgzfMember *)(ctx->bgzf_pinned + x * tab_bytes);
            mstart[x].resize(kMaxMembers);
            zbuf[x].alloc(CH + 64);
            dtab[x].alloc(kMaxMembers);
            dstat[x].alloc(kMaxMembers + 2);
        }
    }

    // Chunk x of a block-gzip file: the carry (carry_x bytes at carry_src, on the device) copied
    // to the front of the text, the members ck describes (compressed bytes in hb[x] + R, table
    // in htab[x]) staged and inflated behind it, all on the copy stream; cs.ev[x] marks
    // completion. The text is what the host path would have uploaded: leading blank bytes of
    // the file are left out (while `leading`, the host inflates members until it meets a solid
    // byte; wholly blank ones are dropped from the table, the next one is inflated that far in
    // front of the text), the file's tail is finished by k_bgzf_tail. total_x is final unless
    // the chunk ends the file: wait_inflate() then has the length.
    void prepare_inflate(int x, size_t carry_x, const uint8_t *carry_src, const BgzfChunk &ck, bool &leading,
                         bool trim_tail, size_t &total_x) {
        const uint8_t *zsrc = hb[x] + R;
        BgzfMember *tab = htab[x];
        uint32_t n = ck.n_members, lead = 0, dropped = 0;
        if (leading) {  // no solid byte of the file seen yet (a chunk of blank members: still none)
            std::vector<uint8_t> t;
            for (uint32_t i = 0; i < n && leading; ++i) {
                if (!bgzf_host_inflate(zsrc, tab[i], t)) break;  // corrupt: the kernel reports it
                uint32_t k = 0;
                while (k < tab[i].olen && is_space(t[k])) ++k;
                lead += k;
                if (k < tab[i].olen) leading = false;
                else dropped = i + 1;
            }
            if (dropped) {
                memmove(tab, tab + dropped, sizeof(BgzfMember) * (n - dropped));
                memmove(mstart[x].data(), mstart[x].data() + dropped, 4 * (size_t)(n - dropped));
                n -= dropped;
            }
        }
        total_x = carry_x + ck.text - lead;
        Inflate &in = inflate[x];
        in.active = true;
        in.eof = ck.eof;
        in.ck = ck;
        in.ck.n_members = n;
        in.dropped = dropped;
        // dbufs[x] is free once the kernels of the chunk it held last have run
        HIP_OK(hipStreamWaitEvent(cs.s, cs.done[x], 0));
        if (carry_x) HIP_OK(hipMemcpyAsync(text(x), carry_src, carry_x, hipMemcpyDeviceToDevice, cs.s));
        HIP_OK(hipMemsetAsync(dstat[x].p, 0xFF, 8, cs.s));
        if (n) {
            HIP_OK(hipMemcpyAsync(zbuf[x].p, zsrc, ck.zbytes, hipMemcpyHostToDevice, cs.s));
            HIP_OK(hipMemcpyAsync(dtab[x].p, tab, sizeof(BgzfMember) * n, hipMemcpyHostToDevice, cs.s));
            in.kt.reset(new KernelTimer(ctx, "bgzf_inflate", (double)ck.zbytes + (double)ck.text, cs.s));
            // member i's text at text + carry + ooff - lead (ooff counts from the chunk's first member)
            bgzf_inflate_launch(cs.s, zbuf[x].p, dtab[x].p, n, text(x) + carry_x - lead, dstat[x].p + 2, dstat[x].p);
            in.kt->mark();
        }
        if (ck.eof) {
            bgzf_tail_launch(cs.s, text(x), (uint32_t)total_x, trim_tail, dstat[x].p + 1);
        } else if (total_x) {
            const size_t padded = (total_x + kSeg - 1) / kSeg * kSeg + kSeg;
            HIP_OK(hipMemsetAsync(text(x) + total_x, 0, padded - total_x, cs.s));
        }
        HIP_OK(hipMemcpyAsync(hstat + 2 * x, dstat[x].p, 8, hipMemcpyDeviceToHost, cs.s));
        HIP_OK(hipEventRecord(cs.ev[x], cs.s));
    }

    // waits for the inflate of chunk x; corrupt data is an error that names the member. Returns
    // the chunk's text length (the tail kernel's at the end of the file)
    size_t wait_inflate(int x, size_t total, const char *path) {
        Inflate &in = inflate[x];
        if (!in.active) return total;
        in.active = false;
        HIP_OK(hipEventSynchronize(cs.ev[x]));
        if (in.kt) {
            in.kt->finish();
            in.kt.reset();
        }
        const uint32_t bad = hstat[2 * x];
        if (bad != ~0u) {
            uint32_t st = 0;
            if (bad < in.ck.n_members) HIP_OK(hipMemcpy(&st, dstat[x].p + 2 + bad, 4, hipMemcpyDeviceToHost));
            throw Error(MCAAT_E_IO, std::string("corrupt BGZF data in ") + path + ": member " +
                                        std::to_string(in.ck.first_index + in.dropped + bad) + " at offset " +
                                        std::to_string(in.ck.file_off + (bad < in.ck.n_members ? mstart[x][bad] : 0)) +
                                        ": " + bgzf_status_text(st));
        }
        return in.eof ? (size_t)hstat[2 * x + 1] : total;
    }

    // chunk x: host bytes [start, start+total) of hb[x] (carry + new data; blank bytes trimmed
    // at the file's start and, with trim_tail, at its end; a last line without its newline gets
    // one) uploaded on the copy stream into dbufs[x]; cs.ev[x] marks completion
    void prepare(int x, size_t carry_x, size_t n_x, bool eof_x, bool first_x, bool trim_tail, uint8_t *&start_x,
                 size_t &total_x) {
        start_x = hb[x] + R - carry_x;
        total_x = carry_x + n_x;
        if (first_x)  // leading blank lines
            while (total_x && is_space(*start_x)) ++start_x, --total_x;
        if (eof_x) {
            if (trim_tail)
                while (total_x && is_space(start_x[total_x - 1])) --total_x;
            if (total_x && (trim_tail || start_x[total_x - 1] != '\n')) start_x[total_x++] = '\n';
        }
        if (total_x) {
            const size_t padded = (total_x + kSeg - 1) / kSeg * kSeg + kSeg;
            // dbufs[x] is free once the kernels of the chunk it held last have run
            HIP_OK(hipStreamWaitEvent(cs.s, cs.done[x], 0));
            HIP_OK(hipMemcpyAsync(text(x), start_x, total_x, hipMemcpyHostToDevice, cs.s));
            HIP_OK(hipMemsetAsync(text(x) + total_x, 0, padded - total_x, cs.s));
            HIP_OK(hipEventRecord(cs.ev[x], cs.s));
        }
    }

    // the newline passes over chunk x once its upload is complete: nl[] holds the position of
    // every '\n'; their number is returned
    uint32_t newlines(int x, size_t total, const char *timer) {
        if (!total) return 0;
        const uint32_t nseg = (uint32_t)((total + kSeg - 1) / kSeg);
        HIP_OK(hipStreamWaitEvent(ctx->stream, cs.ev[x], 0));
        KernelTimer kt(ctx, timer, 2.0 * (double)total);
        HIP_OK(hipMemsetAsync(cnt.p + nseg, 0, 4, ctx->stream));
        launch_at(ctx->stream, dim3(grid_for(nseg, kBlock)), dim3(kBlock), k_fq_nlcount, text(x), nseg, cnt.p);
        scan_u32(ctx, cnt.p, first.p, (uint64_t)nseg + 1, tmp);
        launch_at(ctx->stream, dim3(grid_for(nseg, kBlock)), dim3(kBlock), k_fq_nlpos, text(x), nseg, first.p, nl.p);
        HIP_OK(hipMemcpyAsync(hmeta, first.p + nseg, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        kt.stop();
        return hmeta[0];
    }

    // Every file's chunks in turn. consume(fi, x, total, NL, eof) says how many bytes of chunk x
    // (NL whole lines in `total` bytes) hold whole records; the rest is carried into the next
    // chunk, which uploads while parse(fi, x, consumed) packs this one. file_records gets one
    // entry per file: the growth of n_rec while that file was read.
    template <class Consume, class Parse>
    void run(const char *what, const char *nl_timer, bool trim_tail, const char *const *files, int n_files,
             const Ranges *ranges, const uint64_t &n_rec, std::vector<uint64_t> &file_records, Consume consume,
             Parse parse) {
        const size_t chunk = CH;
        for (int fi = 0; fi < n_files; ++fi) {
            const uint64_t rec_before = n_rec;
            struct FileDone {  // records of this file, however the loop below is left
                std::vector<uint64_t> &v;
                const uint64_t &n, before;
                ~FileDone() { v.push_back(n - before); }
            } file_done{file_records, n_rec, rec_before};
            if (ranges && (*ranges)[fi].first >= (*ranges)[fi].second) continue;  // no part of this file
            Source src(files[fi], ranges ? (*ranges)[fi].first : 0, ranges ? (*ranges)[fi].second : ~0ULL,
                       device_inflate);
            if (src.bgzf) {
                run_bgzf(what, nl_timer, trim_tail, files[fi], fi, src, consume, parse);
                continue;
            }
            int cur = 0;
            size_t n = src.read(hb[cur] + R, chunk);
            bool eof = n < chunk;
            uint8_t *start = nullptr;
            size_t total = 0;
            prepare(cur, 0, n, eof, true, trim_tail, start, total);
            std::future<size_t> next;
            if (!eof) {
                uint8_t *dst = hb[cur ^ 1] + R;
                next = std::async(std::launch::async, [&src, dst, chunk] { return src.read(dst, chunk); });
            }
            for (;;) {
                const uint32_t NL = newlines(cur, total, nl_timer);
                const size_t consumed = consume(fi, cur, total, NL, eof);
                if (!eof && total - consumed > R)
                    throw FormatError(std::string(what) + " record longer than the chunk reserve (" + std::to_string(R) +
                                      " bytes): " + files[fi]);
                // ---- the next chunk: its carry is known now, so it uploads while this chunk's
                // records are parsed; this chunk's host buffer is free again for the reader
                const bool have_next = !eof;
                uint8_t *nstart = nullptr;
                size_t ntotal = 0;
                bool neof = true;
                if (have_next) {
                    const size_t nn = next.get();
                    neof = nn < chunk;
                    const size_t ncarry = total - consumed;
                    memcpy(hb[cur ^ 1] + R - ncarry, start + consumed, ncarry);
                    prepare(cur ^ 1, ncarry, nn, neof, false, trim_tail, nstart, ntotal);
                    if (!neof) {
                        uint8_t *dst = hb[cur] + R;
                        next = std::async(std::launch::async, [&src, dst, chunk] { return src.read(dst, chunk); });
                    }
                }
                parse(fi, cur, consumed);
                HIP_OK(hipEventRecord(cs.done[cur], ctx->stream));
                if (!have_next) break;
                cur ^= 1;
                start = nstart;
                total = ntotal;
                eof = neof;
            }
        }
        HIP_OK(hipStreamSynchronize(ctx->stream));
    }

    // One block-gzip file, chunk by chunk: run()'s loop with the text inflated on the device. The
    // carry goes from chunk to chunk on the device (after this chunk's newline pass, before the
    // next chunk's inflate, both on the copy stream), and the end of the file is the member
    // walk's flag: chunks of whole members have no fixed size.
    template <class Consume, class Parse>
    void run_bgzf(const char *what, const char *nl_timer, bool trim_tail, const char *path, int fi, Source &src,
                  Consume &consume, Parse &parse) {
        ensure_inflate();
        BgzfReader &rd = *src.bgzf;
        auto fill = [this, &rd](int x) { return rd.fill(hb[x] + R, CH, htab[x], mstart[x].data(), kMaxMembers); };
        int cur = 0;
        const BgzfChunk ck = fill(cur);
        bool eof = ck.eof;
        size_t total = 0;
        bool leading = true;  // the file's leading blank bytes are not yet behind us
        prepare_inflate(cur, 0, nullptr, ck, leading, trim_tail, total);
        std::future<BgzfChunk> next;
        if (!eof) next = std::async(std::launch::async, fill, cur ^ 1);
        for (;;) {
            total = wait_inflate(cur, total, path);
            const uint32_t NL = newlines(cur, total, nl_timer);
            const size_t consumed = consume(fi, cur, total, NL, eof);
            if (!eof && total - consumed > R)
                throw FormatError(std::string(what) + " record longer than the chunk reserve (" + std::to_string(R) +
                                  " bytes): " + path);
            const bool have_next = !eof;
            size_t ntotal = 0;
            bool neof = true;
            if (have_next) {
                const BgzfChunk nk = next.get();
                neof = nk.eof;
                prepare_inflate(cur ^ 1, total - consumed, text(cur) + consumed, nk, leading, trim_tail, ntotal);
                // this chunk's compressed bytes and table are on the device: its host buffers are free
                if (!neof) next = std::async(std::launch::async, fill, cur);
            }
            parse(fi, cur, consumed);
            HIP_OK(hipEventRecord(cs.done[cur], ctx->stream));
            if (!have_next) break;
            cur ^= 1;
            total = ntotal;
            eof = neof;
        }
    }

    // the finished streams as a read library; the mapping view is kept when it is `separate`
    void finish(Library &lib, bool separate, mcaat_reads *r) {
        r->ctx = ctx;
        r->n_reads = lib.n_reads;
        r->n_bases = lib.n_bases;
        r->n_words = (lib.n_bases + 31) / 32;
        r->fixed_len = 0;
        if (lib.n_reads > 0) {
            uint64_t L = 0;
            HIP_OK(hipMemcpy(&L, lib.offsets.p + 1, 8, hipMemcpyDeviceToHost));
            HIP_OK(hipMemsetAsync(meta.p, 0, 4, ctx->stream));
            launch_at(ctx->stream, dim3(grid_for(lib.n_reads + 1, kBlock)), dim3(kBlock), k_fq_fixed_len, lib.offsets.p,
                      lib.n_reads, L, meta.p);
            HIP_OK(hipMemcpyAsync(hmeta, meta.p, 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_OK(hipStreamSynchronize(ctx->stream));
            if (!hmeta[0] && L > 0) r->fixed_len = L;
        }
        r->packed = std::move(lib.packed);
        r->offsets = std::move(lib.offsets);
        r->n_records = lib.n_rec;
        r->file_records = lib.file_records;
        r->has_records = separate;
        if (r->has_records) {
            r->rec_packed = std::move(lib.qpacked);
            r->rec_offsets = std::move(lib.qoffsets);
        }
    }
};

}  // namespace

// All inputs are FASTQ (checked by the caller). Files are concatenated; records of files
// after the first are reversed and complemented in the mapping view (paired-end R2).
namespace {
void ingest_fastq_text(mcaat_ctx *ctx, const char *const *files, int n_files, mcaat_reads *r, const Ranges *ranges,
                       bool device_inflate) {
    Library lib(ctx, files, n_files, ranges);
    ChunkIo io(ctx, device_inflate);
    hipStream_t st = ctx->stream;
    uint32_t *const hmeta = io.hmeta;
    DevBuf<uint32_t> sbeg, slen, nbase, nrun, boff, roff, qoff;
    uint32_t flags_all = 0;
    uint32_t nrec = 0;  // records of the chunk at hand

    // records are 4 lines: the bytes after the last complete record carry over
    auto consume = [&](int fi, int, size_t, uint32_t NL, bool eof) -> size_t {
        nrec = NL / 4;
        if (eof && NL % 4)
            throw FormatError(std::string("not 4-line FASTQ (truncated record, blank or wrapped line): ") + files[fi]);
        if (!nrec) return 0;
        HIP_OK(hipMemcpyAsync(hmeta, io.nl.p + 4 * (uint64_t)nrec - 1, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return (size_t)hmeta[0] + 1;
    };
    auto parse = [&](int fi, int cur, size_t consumed) {
        if (!nrec) return;
        KernelTimer kt(ctx, "fq_records", (double)consumed + 16.0 * nrec);
        if (sbeg.n < (uint64_t)nrec + 1) {
            const uint64_t m = std::max<uint64_t>((uint64_t)nrec + 1, io.cap / 64);
            for (auto *b : {&sbeg, &slen, &nbase, &nrun, &boff, &roff, &qoff}) b->alloc(m);
        }
        HIP_OK(hipMemsetAsync(io.meta.p, 0, 4, st));
        for (auto *b : {&nbase, &nrun, &slen}) HIP_OK(hipMemsetAsync(b->p + nrec, 0, 4, st));
        launch_at(st, dim3(grid_for(nrec, kBlock)), dim3(kBlock), k_fq_records, io.text(cur), io.nl.p, nrec, sbeg.p,
                  slen.p, nbase.p, nrun.p, io.meta.p);
        scan_u32(ctx, nbase.p, boff.p, (uint64_t)nrec + 1, io.tmp);
        scan_u32(ctx, nrun.p, roff.p, (uint64_t)nrec + 1, io.tmp);
        scan_u32(ctx, slen.p, qoff.p, (uint64_t)nrec + 1, io.tmp);
        HIP_OK(hipMemcpyAsync(hmeta + 0, boff.p + nrec, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hmeta + 1, roff.p + nrec, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hmeta + 2, qoff.p + nrec, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hmeta + 3, io.meta.p, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        kt.stop();
        const uint32_t cb = hmeta[0], cr = hmeta[1], cq = hmeta[2], fl = hmeta[3];
        if (fl & kBadHeader) throw FormatError(std::string("not 4-line FASTQ (header or '+' line): ") + files[fi]);
        flags_all |= fl;
        if (fi > 0) flags_all |= kDiffer;  // second file: reverse-complemented records
        lib.reserve(ctx, cb, cr, cq, nrec);
        KernelTimer ke(ctx, "fq_emit", (double)consumed + 0.5 * (double)(cb + cq) + 8.0 * (cr + nrec));
        launch_at(st, dim3(grid_for(nrec, kBlock)), dim3(kBlock), k_fq_emit, io.text(cur), nrec, sbeg.p, slen.p, boff.p,
                  roff.p, qoff.p, lib.n_bases, lib.n_reads, lib.q_bases, lib.n_rec, fi > 0 ? 1 : 0, lib.packed.p,
                  lib.offsets.p, lib.qpacked.p, lib.qoffsets.p);
        ke.stop();
        lib.n_bases += cb;
        lib.n_reads += cr;
        lib.q_bases += cq;
        lib.n_rec += nrec;
    };
    io.run("FASTQ", "fq_parse", true, files, n_files, ranges, lib.n_rec, lib.file_records, consume, parse);
    io.finish(lib, (flags_all & kDiffer) != 0, r);
}
}  // namespace

void ingest_fastq(mcaat_ctx *ctx, const char *const *files, int n_files, mcaat_reads *r,
                  const std::vector<std::pair<uint64_t, uint64_t>> *ranges) {
    // plain files of well-formed upper-case ACGT records: packed by host threads (PCIe carries
    // 2 bits per base); any other input falls through to the text parser
    if (fastq_hostpack(ctx, files, n_files, ranges, r)) return;
    // block-gzip files are inflated on the device (knob gz.gpu). When the member walk declines
    // one (BgzfDecline), this ingest starts again from the first file with the host inflate
    // stream under the same parser: nothing of the first attempt is kept, r is written last.
    if (knob(ctx, "gz.gpu", 1) != 0) {
        try {
            ingest_fastq_text(ctx, files, n_files, r, ranges, true);
            return;
        } catch (const BgzfDecline &) {
        }
    }
    ingest_fastq_text(ctx, files, n_files, r, ranges, false);
}

// All inputs are FASTA (checked by the caller): records of a '>' header line and any number of
// sequence lines, read as the host kseq-style reader reads them (capi.hip read_fastx_host).
// Files are concatenated; records of files after the first are reversed and complemented, over
// the whole concatenated record, in the mapping view. A chunk is consumed up to the start of
// its last header line (the record that header opens may continue in the next chunk), so a
// chunk always begins at a header and no read crosses a chunk. A line that starts with '@' or
// '+' outside a header is FASTQ grammar under kseq: FormatError, and the caller reads the input
// again on the host, as it does for a record above the carry reserve.
namespace {
void ingest_fasta_text(mcaat_ctx *ctx, const char *const *files, int n_files, mcaat_reads *r, const Ranges *ranges,
                       bool device_inflate) {
    Library lib(ctx, files, n_files, ranges);
    ChunkIo io(ctx, device_inflate);
    hipStream_t st = ctx->stream;
    uint32_t *const hmeta = io.hmeta;
    // per line; recx: headers before the line; prev: key of the nearest non-empty line before it
    DevBuf<uint32_t> len, nbase, nrun, lflag, hflag, key, prev, recx, hdr, boff, roff, qoff;
    DevBuf<uint32_t> flags(1);  // kDiffer of all chunks (k_fa_lines keeps its own in io.meta)
    HIP_OK(hipMemsetAsync(flags.p, 0, 4, st));
    uint32_t flags_all = 0;
    uint32_t n_use = 0;  // lines of the chunk at hand that are consumed

    auto consume = [&](int fi, int cur, size_t total, uint32_t NL, bool eof) -> size_t {
        n_use = 0;
        if (!NL) return 0;
        if (len.n < (uint64_t)NL + 1) {
            const uint64_t m = std::max<uint64_t>((uint64_t)NL + 1, io.cap / 32);
            for (auto *b : {&len, &nbase, &nrun, &lflag, &hflag, &key, &prev, &recx, &hdr, &boff, &roff, &qoff}) b->alloc(m);
        }
        KernelTimer kt(ctx, "fa_lines", (double)total + 28.0 * NL);
        HIP_OK(hipMemsetAsync(io.meta.p, 0, 12, st));
        launch_at(st, dim3(grid_for(NL, kBlock)), dim3(kBlock), k_fa_lines, io.text(cur), io.nl.p, NL, len.p, nbase.p,
                  nrun.p, lflag.p, hflag.p, key.p, io.meta.p);
        HIP_OK(hipMemcpyAsync(hmeta, io.meta.p, 12, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        kt.stop();
        const uint32_t fl = hmeta[0], h_idx = hmeta[1], h_pos = hmeta[2];
        if (fl & kBadHeader)
            throw FormatError(std::string("not plain FASTA (a sequence line starts with '@' or '+'): ") + files[fi]);
        flags_all |= fl;
        n_use = eof ? NL : h_idx - 1;  // line 0 is a header: h_idx >= 1
        return eof ? total : (size_t)h_pos;
    };
    auto parse = [&](int fi, int cur, size_t consumed) {
        const uint32_t n = n_use;
        if (!n) return;
        KernelTimer kt(ctx, "fa_lines", 56.0 * n);
        scan_u32(ctx, hflag.p, recx.p, (uint64_t)n + 1, io.tmp);
        {
            size_t need = 0;
            HIP_OK(hipcub::DeviceScan::ExclusiveScan(nullptr, need, key.p, prev.p, hipcub::Max(), 0u, (size_t)n, st));
            if (need > io.tmp.bytes()) io.tmp.alloc(need);
            HIP_OK(hipcub::DeviceScan::ExclusiveScan(io.tmp.p, need, key.p, prev.p, hipcub::Max(), 0u, (size_t)n, st));
        }
        launch_at(st, dim3(grid_for((uint64_t)n + 1, kBlock)), dim3(kBlock), k_fa_link, n, prev.p, recx.p, nrun.p, lflag.p,
                  hdr.p);
        scan_u32(ctx, nbase.p, boff.p, (uint64_t)n + 1, io.tmp);
        scan_u32(ctx, nrun.p, roff.p, (uint64_t)n + 1, io.tmp);
        scan_u32(ctx, len.p, qoff.p, (uint64_t)n + 1, io.tmp);
        HIP_OK(hipMemcpyAsync(hmeta + 0, boff.p + n, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hmeta + 1, roff.p + n, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hmeta + 2, qoff.p + n, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hmeta + 3, recx.p + n, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        kt.stop();
        const uint32_t cb = hmeta[0], cr = hmeta[1], cq = hmeta[2], nrec = hmeta[3];
        if (fi > 0 && nrec) flags_all |= kDiffer;  // second file: reverse-complemented records
        lib.reserve(ctx, cb, cr, cq, nrec);
        KernelTimer ke(ctx, "fa_emit", (double)consumed + 0.5 * (double)(cb + cq) + 8.0 * (cr + nrec) + 40.0 * n);
        launch_at(st, dim3(grid_for(n, kBlock)), dim3(kBlock), k_fa_emit, io.text(cur), io.nl.p, n, len.p, lflag.p,
                  recx.p, hdr.p, boff.p, roff.p, qoff.p, lib.n_bases, lib.n_reads, lib.q_bases, lib.n_rec,
                  fi > 0 ? 1 : 0, lib.packed.p, lib.offsets.p, lib.qpacked.p, lib.qoffsets.p, flags.p);
        ke.stop();
        lib.n_bases += cb;
        lib.n_reads += cr;
        lib.q_bases += cq;
        lib.n_rec += nrec;
    };
    // blank lines are transparent in FASTA, so the file's tail is not trimmed: a last line of
    // blanks is a sequence line, as it is for kseq
    io.run("FASTA", "fa_parse", false, files, n_files, ranges, lib.n_rec, lib.file_records, consume, parse);
    // the end of the last read (k_fa_emit writes a read's start); any record not one ACGT run
    HIP_OK(hipMemcpyAsync(lib.offsets.p + lib.n_reads, &lib.n_bases, 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(hmeta, flags.p, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    flags_all |= hmeta[0];
    io.finish(lib, (flags_all & kDiffer) != 0, r);
}
}  // namespace

void ingest_fasta(mcaat_ctx *ctx, const char *const *files, int n_files, mcaat_reads *r,
                  const std::vector<std::pair<uint64_t, uint64_t>> *ranges) {
    // block-gzip files on the device, the host inflate stream when the walk declines: as ingest_fastq
    if (knob(ctx, "gz.gpu", 1) != 0) {
        try {
            ingest_fasta_text(ctx, files, n_files, r, ranges, true);
            return;
        } catch (const BgzfDecline &) {
        }
    }
    ingest_fasta_text(ctx, files, n_files, r, ranges, false);
}

}  // namespace mcaat

namespace mcaat {

// The counting view as 4-line FASTQ ("@r", sequence, "+", all-'I' qualities): record i
// starts at byte 2*offsets[i] + 7*i, so host threads format disjoint read ranges and pwrite
// them independently. Used to make FASTQ inputs of the synthetic configs (bench, tests).
void write_fastq(const mcaat_reads *r, const char *path, int threads) {
    std::vector<uint64_t> packed(r->n_words + 1, 0), offs(r->n_reads + 1);
    if (r->n_words) HIP_OK(hipMemcpy(packed.data(), r->packed.p, 8 * r->n_words, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs.data(), r->offsets.p, 8 * (r->n_reads + 1), hipMemcpyDeviceToHost));
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw Error(MCAAT_E_IO, std::string("cannot create ") + path);
    const uint64_t n = r->n_reads;
    const uint64_t total = 2 * (offs[n] - offs[0]) + 7 * n;
    if (ftruncate(fd, (off_t)total) != 0) {
        close(fd);
        throw Error(MCAAT_E_IO, std::string("cannot size ") + path);
    }
    if (threads < 1) threads = 1;
    std::atomic<bool> failed{false};
    auto work = [&](uint64_t a, uint64_t b) {
        std::vector<char> buf;
        buf.reserve(8u << 20);
        uint64_t pos = 2 * (offs[a] - offs[0]) + 7 * a;
        auto flush = [&]() {
            size_t done = 0;
            while (done < buf.size()) {
                const ssize_t w = pwrite(fd, buf.data() + done, buf.size() - done, (off_t)(pos + done));
                if (w <= 0) { failed = true; return; }
                done += (size_t)w;
            }
            pos += buf.size();
            buf.clear();
        };
        for (uint64_t i = a; i < b && !failed; ++i) {
            const uint64_t s = offs[i], L = offs[i + 1] - s;
            const size_t at = buf.size();
            buf.resize(at + 2 * L + 7);
            char *o = buf.data() + at;
            *o++ = '@'; *o++ = 'r'; *o++ = '\n';
            for (uint64_t j = 0; j < L; ++j) o[j] = "ACGT"[(packed[(s + j) >> 5] >> (2 * ((s + j) & 31))) & 3];
            o += L;
            *o++ = '\n'; *o++ = '+'; *o++ = '\n';
            memset(o, 'I', L);
            o[L] = '\n';
            if (buf.size() >= (8u << 20)) flush();
        }
        flush();
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) {
        const uint64_t a = n * t / threads, b = n * (t + 1) / threads;
        if (a < b) pool.emplace_back(work, a, b);
    }
    for (auto &th : pool) th.join();
    close(fd);
    if (failed) throw Error(MCAAT_E_IO, std::string("write failed: ") + path);
}

}  // namespace mcaat

namespace mcaat {

bool is_compressed_file(const char *path) {
    unsigned char m[4] = {0, 0, 0, 0};
    const int fd = open(path, O_RDONLY);
    if (fd < 0) throw Error(MCAAT_E_IO, std::string("cannot open ") + path);
    const ssize_t n = pread(fd, m, 4, 0);
    close(fd);
    const bool gz = n >= 2 && m[0] == 0x1f && m[1] == 0x8b;
    const bool bz = n >= 4 && m[0] == 'B' && m[1] == 'Z' && m[2] == 'h' && m[3] >= '1' && m[3] <= '9';
    return gz || bz;
}

// A line start q >= pos begins a record when line q starts with '@', line q+2 with '+', and
// lines q+1 and q+3 (sequence, quality) have the same length. A quality line that starts
// with '@' is followed by a header and a sequence line, never by '+', so it is not taken.
// The window grows until four whole lines follow a candidate (records up to 64 MiB).
uint64_t fastq_record_start(const char *path, uint64_t pos) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) throw Error(MCAAT_E_IO, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0) {
        close(fd);
        throw Error(MCAAT_E_IO, std::string("cannot stat ") + path);
    }
    const uint64_t size = (uint64_t)st.st_size;
    if (pos == 0 || pos >= size) {
        close(fd);
        return std::min(pos, size);
    }
    std::vector<uint8_t> buf;
    uint64_t result = size;
    // the window starts one byte early so a record starting exactly at pos is seen
    const uint64_t w0 = pos - 1;
    for (uint64_t win = 1 << 16;; win *= 2) {
        const uint64_t n = std::min<uint64_t>(win, size - w0);
        buf.resize(n);
        uint64_t got = 0;
        while (got < n) {
            const ssize_t r = pread(fd, buf.data() + got, n - got, (off_t)(w0 + got));
            if (r <= 0) break;
            got += (uint64_t)r;
        }
        buf.resize(got);
        const bool at_eof = w0 + got >= size;
        // line starts at or after pos (index 0 is byte pos - 1)
        std::vector<uint64_t> ls;
        for (uint64_t i = 0; i + 1 < got; ++i)
            if (buf[i] == '\n') ls.push_back(i + 1);
        auto line_len = [&](size_t li) -> int64_t {  // -1: line not complete in the window
            const uint64_t b = ls[li];
            const uint64_t e = li + 1 < ls.size() ? ls[li + 1] - 1 : (at_eof ? got : ~0ULL);
            if (e == ~0ULL) return -1;
            uint64_t len = e - b;
            if (len && buf[b + len - 1] == '\n') --len;
            if (len && buf[b + len - 1] == '\r') --len;
            return (int64_t)len;
        };
        bool undecided = false;
        for (size_t li = 0; li < ls.size(); ++li) {
            if (buf[ls[li]] != '@') continue;
            if (li + 3 >= ls.size()) {  // the record's four lines are not all in the window
                if (!at_eof) undecided = true;
                break;
            }
            if (buf[ls[li + 2]] != '+') continue;
            const int64_t a = line_len(li + 1), b = line_len(li + 3);
            if (a < 0 || b < 0) { undecided = true; break; }
            if (a != b) continue;
            result = w0 + ls[li];
            break;
        }
        if (result != size || !undecided || at_eof || win >= (64ULL << 20)) break;
    }
    close(fd);
    return result;
}

// The file is scanned window by window from pos - 1 (so a header starting exactly at pos is
// seen); whether a window begins a line is the last byte of the window before it.
uint64_t fasta_record_start(const char *path, uint64_t pos) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) throw Error(MCAAT_E_IO, std::string("cannot open ") + path);
    struct FdClose {
        int fd;
        ~FdClose() { close(fd); }
    } closer{fd};
    struct stat st;
    if (fstat(fd, &st) != 0) throw Error(MCAAT_E_IO, std::string("cannot stat ") + path);
    const uint64_t size = (uint64_t)st.st_size;
    if (pos == 0 || pos >= size) return std::min(pos, size);
    std::vector<uint8_t> buf(1 << 20);
    bool line_start = false;  // pos - 1 is returned only as a '\n' before a header at pos
    for (uint64_t at = pos - 1; at < size;) {
        const ssize_t got = pread(fd, buf.data(), (size_t)std::min<uint64_t>(buf.size(), size - at), (off_t)at);
        if (got < 0) throw Error(MCAAT_E_IO, std::string("read error in ") + path);
        if (got == 0) break;
        const size_t i = fasta_first_header(buf.data(), (size_t)got, line_start);
        if (i < (size_t)got) return at + i;
        line_start = buf[got - 1] == '\n';
        at += (uint64_t)got;
    }
    return size;
}

}  // namespace mcaat
