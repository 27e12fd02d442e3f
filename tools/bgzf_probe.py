"""Times mcaat_reads_from_fastx on one page-cached block-gzip (BGZF) FASTQ with the inflate on the
device (gz.gpu = 1) and on the host stream (gz.gpu = 0), alternated in one process (GPU box).

The file is written here with zlib, no bgzip binary needed: each member a raw deflate stream of
at most 65,280 text bytes behind an 18-byte header with the 'BC' subfield, CRC-32 and ISIZE behind
it, then the 28-byte EOF member. The reads are the ingest probe's (tools/ingest_probe.py), made
slab by slab. For scale the plain-text parser runs on the uncompressed copy (fq.hostpack = 0).

    python tools/bgzf_probe.py [n_reads] [--level 6] [--member 65280] [--calls 3] [--dir /tmp]
"""
import argparse
import concurrent.futures as cf
import dataclasses
import os
import struct
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import mcaat_amd as M  # noqa: E402

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = co.compress(data) + co.flush()
    head = struct.pack("<4BIBBH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(payload) + 25)
    return head + payload + struct.pack("<II", zlib.crc32(data), len(data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_reads", nargs="?", type=int, default=2_000_000)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--member", type=int, default=65280)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    a = ap.parse_args()

    spec = M.SynthSpec(**bench.CONFIGS["c3"]["spec"].__dict__)
    fd, plain = tempfile.mkstemp(suffix=".fq", dir=a.dir)
    os.close(fd)
    gz = plain + ".gz"
    t0 = time.perf_counter()
    slab = 1_000_000
    with open(plain, "wb") as fp, open(gz, "wb") as fz, cf.ThreadPoolExecutor(a.threads) as pool:
        rest = b""
        for i, first in enumerate(range(0, a.n_reads, slab)):
            rec, _ = bench.fastq_records(dataclasses.replace(spec, seed=spec.seed + i), min(slab, a.n_reads - first))
            data = rest + rec.tobytes()
            del rec
            fp.write(data[len(rest):])
            whole = len(data) // a.member * a.member if first + slab < a.n_reads else len(data)
            # zlib releases the interpreter lock while it compresses: members in parallel
            for m in pool.map(lambda p: member(data[p:p + a.member], a.level), range(0, whole, a.member)):
                fz.write(m)
            rest = data[whole:]
        fz.write(EOF_MEMBER)
    text, comp = os.path.getsize(plain), os.path.getsize(gz)
    print(f"{a.n_reads} reads: text {text / 1e6:.0f} MB, BGZF level {a.level} {comp / 1e6:.0f} MB "
          f"(ratio {text / comp:.2f}, members of {a.member}), written in {time.perf_counter() - t0:.0f} s", flush=True)

    def call(ctx, path, label, **knobs):
        with ctx.knobs(**knobs):
            ctx.reset_timing()
            t = time.perf_counter()
            r = M.Reads.from_fastx(ctx, [path])
            dt = time.perf_counter() - t
            ms, n, _ = ctx.kernel_timing("bgzf_inflate")
            info = r.info()
            r.free()
        print(f"{label:<22} wall {dt * 1e3:8.0f} ms  {text / dt / 1e9:6.2f} GB/s of text  "
              f"bgzf_inflate {ms * n:8.1f} ms in {n} launches  reads {info[0]}", flush=True)
        return dt

    try:
        with M.Context(0) as ctx:
            call(ctx, gz, "warm-up gz.gpu=1", gz__gpu=1)
            call(ctx, gz, "warm-up gz.gpu=0", gz__gpu=0)
            pairs = []
            for _ in range(a.calls):
                d = call(ctx, gz, "gz.gpu=1 (device)", gz__gpu=1)
                h = call(ctx, gz, "gz.gpu=0 (host stream)", gz__gpu=0)
                pairs.append((d, h))
            for _ in range(2):
                call(ctx, plain, "plain text parser", fq__hostpack=0)
            worst = max(d / h for d, h in pairs)
            print(f"device / host wall, worst pair: {worst:.3f} (the default stays gz.gpu = 1 at <= 0.5)")
    finally:
        os.unlink(plain)
        os.unlink(gz)


if __name__ == "__main__":
    main()
