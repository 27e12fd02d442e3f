"""Block-gzip (BGZF) FASTQ / FASTA inflated on the GPU (csrc/bgzf_inflate.hip, knob gz.gpu) under
the text parsers of csrc/fastq_ingest.hip, against the Python restatement of the read library
(oracle/fastx.py): bit-exact packed streams and offsets of both views, the record count and
`separate`. The files are written here with zlib: each member a raw deflate stream behind an
18-byte header with the 'BC' subfield, CRC-32 and ISIZE behind it, then the 28-byte EOF member.

Every positive case asserts that the device path ran (the bgzf_inflate timer counted launches),
every decline that it did not: a decline reads the same file through the host inflate stream.
Shapes: every DEFLATE block type, several blocks per member, members of 1 byte to the format's
65,280, stored members at the 16-bit BSIZE limit, EOF members mid-file / missing, chunks forced
down so records straddle members and chunks and the carry moves on the device, the text edges
the host path trims, the copy edge cases of the match executor, paired-end, FASTA, mixed plain
and BGZF inputs, corrupt members (one fresh process each) and the CLI.
"""
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from oracle import fastx as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mcaat_amd", "mcaat")
ALPHA = "ACGT" * 6 + "acgtNRY"
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

SETTINGS = {  # level, strategy, memLevel
    "stored": (0, zlib.Z_DEFAULT_STRATEGY, 8),
    "fixed": (6, zlib.Z_FIXED, 8),
    "l1": (1, zlib.Z_DEFAULT_STRATEGY, 8),
    "l6": (6, zlib.Z_DEFAULT_STRATEGY, 8),
    "l9": (9, zlib.Z_DEFAULT_STRATEGY, 8),
    "mem1": (6, zlib.Z_DEFAULT_STRATEGY, 1),  # several DEFLATE blocks per member
}


def _member(data, setting="l6", extra_before=b""):
    level, strategy, mem = SETTINGS[setting]
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    payload = co.compress(data) + co.flush()
    xlen = len(extra_before) + 6
    bsize = 12 + xlen + len(payload) + 8 - 1
    assert bsize < 65536
    head = struct.pack("<4BIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, xlen) + extra_before + struct.pack("<2BHH", 66, 67, 2, bsize)
    return head + payload + struct.pack("<II", zlib.crc32(data), len(data))


def _bgzf(data, sizes=65280, setting="l6", eof=True, eof_at=(), extra_before=b""):
    """data cut into members of `sizes` text bytes (a number, or a list that is cycled); an EOF
    member after every member index in eof_at, and `eof` of them at the end."""
    out, pos, i = bytearray(), 0, 0
    while pos < len(data):
        n = sizes if isinstance(sizes, int) else sizes[i % len(sizes)]
        out += _member(data[pos:pos + n], setting, extra_before)
        if i in eof_at:
            out += EOF_MEMBER
        pos += n
        i += 1
    out += EOF_MEMBER * int(eof)
    return bytes(out)


def _write_bgzf(path, text, **kw):
    blob = _bgzf(text.encode(), **kw)
    assert gzip.decompress(blob) == text.encode()  # what every gzip reader makes of the file
    with open(path, "wb") as f:
        f.write(blob)
    return str(path)


def _rand_records(rng, n, max_len=300):
    seqs = []
    for i in range(n):
        L = int(rng.integers(0, max_len)) if i % 17 else 0
        s = "".join(rng.choice(list(ALPHA if i % 5 == 0 else "ACGT"), size=L))
        seqs.append(s)
    if n and not seqs[-1]:
        seqs[-1] = "ACGTN"  # a text's blank tail is trimmed: its last record has a sequence
    return seqs


def _fastq_text(seqs, crlf=False, final_newline=True, lead="", trail=""):
    nl = "\r\n" if crlf else "\n"
    body = nl.join(f"@r{i} x{nl}{s}{nl}+{nl}{'I' * len(s)}" for i, s in enumerate(seqs))
    return lead + body + (nl if final_newline else "") + trail


def _fasta_text(seqs, width=60):
    lines = []
    for i, s in enumerate(seqs):
        lines.append(f">c{i} x>y")
        lines += [s[p:p + width] for p in range(0, len(s), width)]
    return "\n".join(lines) + "\n"


def _set_chunk(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("MCAAT_FASTQ_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("MCAAT_FASTQ_CHUNK", raising=False)


def _inflated_on_device(ctx):
    return ctx.kernel_timing("bgzf_inflate")[1] > 0


def _check(ctx, files, texts, device=True, fasta=False):
    """The library of `files` equals the restatement's of `texts`; the device inflate ran or not."""
    import mcaat_amd as M

    per_file = [(FX.kseq_sequences if fasta else FX.fastq_sequences)(t) for t in texts]
    want_p, want_o = FX.pack_bases(FX.counting_view([s for f in per_file for s in f]))
    want_qp, want_qo = FX.pack_codes(FX.mapping_view(per_file))
    ctx.reset_timing()
    reads = M.Reads.from_fastx(ctx, files)
    assert _inflated_on_device(ctx) == device
    p, o = reads.download()
    assert np.array_equal(o, want_o)
    nw = (int(want_o[-1]) + 31) // 32
    assert np.array_equal(p[:nw], want_p[:nw])
    qp, qo = reads.download_records()
    assert np.array_equal(qo, want_qo)
    nq = (int(want_qo[-1]) + 31) // 32
    assert np.array_equal(qp[:nq], want_qp[:nq])
    n_rec, separate = reads.records_info()
    assert n_rec == sum(len(f) for f in per_file)
    one_run = all(len(s) > 0 and set(s) <= set("ACGT") for f in per_file for s in f)
    assert separate == (any(len(f) > 0 for f in per_file[1:]) or not one_run)
    reads.free()


_TEXT400 = []


def _text400():
    if not _TEXT400:
        _TEXT400.append(_fastq_text(_rand_records(np.random.default_rng(2024), 400)))
    return _TEXT400[0]


# ---- the writer (CPU): its files are gzip files, members as laid out ------------------------------

def test_writer_makes_gzip_files_with_the_bc_subfield():
    text = _text400().encode()
    blob = _bgzf(text, sizes=777, eof_at=(3,), extra_before=b"XY\x03\x00abc")
    assert gzip.decompress(blob) == text
    assert blob[:4] == b"\x1f\x8b\x08\x04" and blob[10:12] == struct.pack("<H", 13) and blob[19:21] == b"BC"
    assert blob.endswith(EOF_MEMBER) and gzip.decompress(EOF_MEMBER) == b""
    stored = _member(text[:65280], "stored")
    assert 65300 < len(stored) <= 65536  # a stored member of the largest text is near the 16-bit limit


# ---- 1. every block type ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["stored", "fixed", "l1", "l9", "mem1"])
def test_every_block_type(gpu_ctx, tmp_path, monkeypatch, setting):
    _set_chunk(monkeypatch, 0)
    text = _text400()
    _check(gpu_ctx, [_write_bgzf(tmp_path / "a.fq.gz", text, setting=setting)], [text])


# ---- 2. member sizes -------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", ["1", "64", "777", "65280", "stored_60000", "stored_65280", "eof_mid", "no_eof",
                                  "bc_not_first"])
def test_member_sizes(gpu_ctx, tmp_path, monkeypatch, case):
    _set_chunk(monkeypatch, 0)
    text = _text400()
    kw = {"1": dict(sizes=1), "64": dict(sizes=64), "777": dict(sizes=777), "65280": dict(sizes=65280),
          "stored_60000": dict(sizes=60000, setting="stored"), "stored_65280": dict(sizes=65280, setting="stored"),
          "eof_mid": dict(sizes=5000, eof_at=(0, 7)), "no_eof": dict(sizes=5000, eof=False),
          "bc_not_first": dict(sizes=5000, extra_before=b"XY\x03\x00abc")}[case]
    _check(gpu_ctx, [_write_bgzf(tmp_path / "a.fq.gz", text, **kw)], [text])


# ---- 3. chunk logic --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [256, 1000, 4099])
def test_chunk_logic(gpu_ctx, tmp_path, monkeypatch, chunk):
    """Members of 100..700 text bytes under forced chunk sizes: records straddle members and
    chunks, the carry is copied on the device many times, chunks of one member. At 256 a
    member's text alone exceeds the chunk (the first one, 700 bytes): the walk declines before
    anything is launched and the host stream feeds the same parser."""
    _set_chunk(monkeypatch, chunk)
    rng = np.random.default_rng(31)
    sizes = [700] + [int(v) for v in rng.integers(100, 701, size=40)]
    assert max(sizes) > 256 and min(sizes) < 256
    text = _text400()
    _check(gpu_ctx, [_write_bgzf(tmp_path / "a.fq.gz", text, sizes=sizes)], [text], device=chunk != 256)


# ---- 4. text edges ---------------------------------------------------------------------------------

FASTQ_EDGES = {
    "leading_blank_lines": dict(lead="\n\n \r\n"),
    "leading_blank_members": dict(lead="\n" * 250),
    "trailing_blank_lines": dict(trail="\n\n \n"),
    "trailing_blanks_then_empty_members": dict(trail="\n \n"),  # written with 12 EOF members: see below
    "no_final_newline": dict(final_newline=False),
    "crlf": dict(crlf=True),
    "crlf_no_final_newline": dict(crlf=True, final_newline=False, lead="\r\n"),
}
FASTA_EDGES = {  # the tail cases of the FASTA ingest's edge texts
    "blank_tail_line": ">a\nACGT\n \n",  # a last line of blanks is a sequence line
    "header_last": ">a\nACGT\n>b",
    "header_only": ">a\n",
    "line_of_only_cr": ">a\r\nACG\r\n\r\nTT\r\n>b\r\n\r\n",
    "run_crosses_empty_line": ">a\nACG\n\n\nTTA\n\n>b\n\nGG\n",
    "leading_blank_lines": "\n\n>a\nACGT\nAC",
}


@pytest.mark.gpu
@pytest.mark.parametrize("member,chunk", [(65280, 0), (100, 256), (37, 1000)])
def test_text_edges(gpu_ctx, tmp_path, monkeypatch, member, chunk):
    """What ChunkIo::prepare trims and adds on the host for uploaded text, on inflated text: in
    one member and one chunk, and with small members and chunks, where blank members are dropped
    in front and the tail reaches back into the carry."""
    _set_chunk(monkeypatch, chunk)
    seqs = _rand_records(np.random.default_rng(8), 12, max_len=90)
    for name, kw in FASTQ_EDGES.items():
        text = _fastq_text(seqs, **kw)
        # 12 empty members are 336 compressed bytes: at chunk 256 the file's last chunk holds
        # nothing but empty members, and the blank tail to trim lies in the carry
        eof = 12 if name == "trailing_blanks_then_empty_members" else 1
        _check(gpu_ctx, [_write_bgzf(tmp_path / f"{name}.fq.gz", text, sizes=member, eof=eof)], [text])
    for name, text in FASTA_EDGES.items():
        _check(gpu_ctx, [_write_bgzf(tmp_path / f"{name}.fa.gz", text, sizes=member)], [text], fasta=True)


# ---- 5. the match executor's edge cases --------------------------------------------------------------

def _rec(rng, L):
    """A record of exactly 2 L + 7 bytes with random sequence and random qualities."""
    s = "".join(rng.choice(list("ACGT"), size=L))
    q = "".join(chr(int(c)) for c in rng.integers(35, 75, size=L))
    return f"@r\n{s}\n+\n{q}\n"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["run_of_one_byte", "max_distance", "one_wave_of_lanes"])
def test_copy_cases(gpu_ctx, tmp_path, monkeypatch, case):
    _set_chunk(monkeypatch, 0)
    rng = np.random.default_rng(77)
    if case == "run_of_one_byte":
        # quality lines of one character, 300 long: dist 1 / len 258, then a remainder
        text = _fastq_text(["".join(rng.choice(list("ACGT"), size=300)) for _ in range(20)])
    elif case == "max_distance":
        # 40 KiB that repeat their first 1 KiB at offset 32768: 4 records of 1024 bytes, 64 of
        # 31744, the first 4 again, then more records
        first = "".join(_rec(rng, L) for L in (124, 124, 125, 125))
        fill = "".join(_rec(rng, 244 + (i & 1)) for i in range(64))
        rest = "".join(_rec(rng, 200) for _ in range(18))
        text = first + fill + first + rest
        assert len(first) == 1024 and text[32768:33792] == text[:1024] and len(text) > 40000
    else:
        # a 64-byte record without a repeated trigram, twice: one match that spans exactly one
        # wave's worth of lanes
        unit = "@0123456789abcdefghijklmnop\nACGTTGCAAGTCCTGA\n+\nIHGFEDCBA@?>=<;:\n"
        assert len(unit) == 64
        text = unit + unit
    _check(gpu_ctx, [_write_bgzf(tmp_path / "a.fq.gz", text, setting="l9")], [text])


def _hand_built_distance_32768(data):
    """A DEFLATE stream for 32768 + 261 bytes whose tail repeats its head: one stored block of
    32768 bytes, then a fixed block with (length 258, distance 32768), (length 3, distance
    32768) and the end-of-block code. zlib's deflate never looks back further than 32768 - 262,
    so only a stream written by hand carries the longest distance."""
    assert len(data) == 32768 + 261 and data[32768:] == data[:261]
    out = bytearray(b"\x00\x00\x80\xff\x7f") + data[:32768]  # BFINAL 0, stored, LEN 32768, NLEN
    acc = nbits = 0

    def put(value, n, msb_first):
        nonlocal acc, nbits
        for i in range(n):
            bit = (value >> (n - 1 - i if msb_first else i)) & 1
            acc |= bit << nbits
            nbits += 1
            if nbits == 8:
                out.append(acc)
                acc = nbits = 0

    put(1, 1, False)  # BFINAL
    put(1, 2, False)  # fixed codes
    for length_code, bits in ((0xC5, 8), (0x01, 7)):  # 285: length 258; 257: length 3
        put(length_code, bits, True)
        put(29, 5, True)  # distances 24577..32768
        put(8191, 13, False)
    put(0, 7, True)  # end of block
    if nbits:
        out.append(acc)
    return bytes(out)


@pytest.mark.gpu
def test_match_at_distance_32768(gpu_ctx, tmp_path, monkeypatch):
    """The longest distance DEFLATE has, through the wave's match copy: the first member is the
    hand-built stream above (a stored block and a fixed block in one member), the second holds
    the rest of the text."""
    _set_chunk(monkeypatch, 0)
    rng = np.random.default_rng(78)
    first = "".join(_rec(rng, L) for L in (124, 124, 125, 125))
    fill = "".join(_rec(rng, 244 + (i & 1)) for i in range(64))
    text = first + fill + first
    data = text.encode()
    assert len(first + fill) == 32768
    head = data[:32768 + 261]
    payload = _hand_built_distance_32768(head)
    assert zlib.decompress(payload, -15) == head
    member = (struct.pack("<4BIBBH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(payload) + 25) + payload
              + struct.pack("<II", zlib.crc32(head), len(head)))
    blob = member + _member(data[len(head):]) + EOF_MEMBER
    assert gzip.decompress(blob) == data
    path = tmp_path / "a.fq.gz"
    path.write_bytes(blob)
    _check(gpu_ctx, [str(path)], [text])


# ---- 6. the layers above -----------------------------------------------------------------------------

@pytest.mark.gpu
def test_paired_end(gpu_ctx, tmp_path, monkeypatch):
    _set_chunk(monkeypatch, 4099)
    rng = np.random.default_rng(5)
    t1 = _fastq_text(_rand_records(rng, 300), crlf=True)
    t2 = _fastq_text(_rand_records(rng, 300), final_newline=False)
    files = [_write_bgzf(tmp_path / "r1.fq.gz", t1, sizes=1500), _write_bgzf(tmp_path / "r2.fq.gz", t2, sizes=901)]
    _check(gpu_ctx, files, [t1, t2])


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [0, 1000])
def test_fasta_wrapped_at_60(gpu_ctx, tmp_path, monkeypatch, chunk):
    _set_chunk(monkeypatch, chunk)
    rng = np.random.default_rng(6)
    text = _fasta_text(_rand_records(rng, 120))
    files = [_write_bgzf(tmp_path / "a.fa.gz", text, sizes=777), _write_bgzf(tmp_path / "b.fa.gz", text, sizes=300)]
    _check(gpu_ctx, files, [text, text], fasta=True)


@pytest.mark.gpu
def test_plain_and_bgzf_in_one_call(gpu_ctx, tmp_path, monkeypatch):
    _set_chunk(monkeypatch, 4099)
    rng = np.random.default_rng(9)
    t1, t2, t3 = (_fastq_text(_rand_records(rng, 100)) for _ in range(3))
    plain = tmp_path / "a.fq"
    plain.write_text(t1)
    single = tmp_path / "c.fq.gz"  # an ordinary gzip file beside them: the host stream
    with gzip.open(single, "wb") as f:
        f.write(t3.encode())
    files = [str(plain), _write_bgzf(tmp_path / "b.fq.gz", t2, sizes=1000), str(single)]
    _check(gpu_ctx, files, [t1, t2, t3])


@pytest.mark.gpu
def test_knob_off_matches_on(gpu_ctx, tmp_path, monkeypatch):
    import mcaat_amd as M

    _set_chunk(monkeypatch, 0)
    text = _text400()
    path = _write_bgzf(tmp_path / "a.fq.gz", text, sizes=4000)
    got = []
    for on in (1, 0):
        with gpu_ctx.knobs(gz__gpu=on):
            _check(gpu_ctx, [path], [text], device=bool(on))
            gpu_ctx.reset_timing()
            r = M.Reads.from_fastx(gpu_ctx, [path])
            assert _inflated_on_device(gpu_ctx) == bool(on)
            got.append((r.download(), r.download_records(), r.info(), r.records_info()))
            r.free()
    (p1, o1), (q1, qo1), i1, ri1 = got[0]
    (p0, o0), (q0, qo0), i0, ri0 = got[1]
    nw, nq = (int(o1[-1]) + 31) // 32, (int(qo1[-1]) + 31) // 32
    assert i1 == i0 and ri1 == ri0 and np.array_equal(o1, o0) and np.array_equal(qo1, qo0)
    assert np.array_equal(p1[:nw], p0[:nw]) and np.array_equal(q1[:nq], q0[:nq])


@pytest.mark.gpu
def test_single_member_gzip_takes_the_host_stream(gpu_ctx, tmp_path, monkeypatch):
    _set_chunk(monkeypatch, 0)
    text = _text400()
    path = tmp_path / "a.fq.gz"
    with gzip.open(path, "wb") as f:
        f.write(text.encode())
    _check(gpu_ctx, [str(path)], [text], device=False)


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["plain_gzip_member", "junk", "bsize_past_the_end"])
def test_a_later_member_that_is_not_bgzf_declines(gpu_ctx, tmp_path, monkeypatch, tail):
    """The walk meets it in the file's first chunk, before anything is launched: the host stream
    reads the whole file, as it did before."""
    import mcaat_amd as M

    _set_chunk(monkeypatch, 0)
    seqs = _rand_records(np.random.default_rng(12), 60)
    t1, t2 = _fastq_text(seqs[:40]), _fastq_text(seqs[40:])
    path = tmp_path / "a.fq.gz"
    if tail == "plain_gzip_member":
        path.write_bytes(_bgzf(t1.encode(), sizes=3000, eof=False) + gzip.compress(t2.encode()))
        _check(gpu_ctx, [str(path)], [t1 + t2], device=False)
        return
    blob = _bgzf((t1 + t2).encode(), sizes=3000)
    path.write_bytes(blob + b"junk" if tail == "junk" else blob[:-len(EOF_MEMBER) - 10])
    gpu_ctx.reset_timing()
    if tail == "junk":  # zlib's gzread ignores trailing garbage after a complete member
        _check(gpu_ctx, [str(path)], [t1 + t2], device=False)
    else:  # whatever the host stream makes of a file cut inside a member, it is the one that reads it
        try:
            M.Reads.from_fastx(gpu_ctx, [str(path)]).free()
        except RuntimeError:
            pass
        assert not _inflated_on_device(gpu_ctx)


# ---- 7. corrupt input: one process each ----------------------------------------------------------------

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import mcaat_amd as M
bad, good = sys.argv[2], sys.argv[3]
with M.Context(0) as ctx:
    try:
        M.Reads.from_fastx(ctx, [bad])
    except M.McaatError as e:
        print("ERROR", e)
    else:
        print("NO ERROR")
    ctx.reset_timing()
    r = M.Reads.from_fastx(ctx, [good])
    print("GOOD", r.records_info()[0], ctx.kernel_timing("bgzf_inflate")[1] > 0)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("damage", ["crc_bit", "isize_plus_one", "payload_bit"])
def test_corrupt_member_is_an_io_error(tmp_path, damage):
    """A flipped CRC bit in the second member, an ISIZE one too large in the second, one flipped
    payload bit in the third member's dynamic block: MCAAT_E_IO that names the file and the
    member, and the same context ingests a good file afterwards. Python's gzip refuses the same
    files."""
    seqs = _rand_records(np.random.default_rng(3), 80)
    text = _fastq_text(seqs).encode()
    members = [_member(text[p:p + 3000]) for p in range(0, len(text), 3000)]
    assert len(members) >= 4
    m = bytearray(members[2 if damage == "payload_bit" else 1])
    if damage == "crc_bit":
        m[-8] ^= 0x10
    elif damage == "isize_plus_one":
        m[-4:] = struct.pack("<I", struct.unpack("<I", m[-4:])[0] + 1)
    else:
        assert (m[18] >> 1) & 3 == 2  # a dynamic block
        m[18 + 200] ^= 0x04
    members[2 if damage == "payload_bit" else 1] = bytes(m)
    bad = tmp_path / "bad.fq.gz"
    bad.write_bytes(b"".join(members) + EOF_MEMBER)
    with pytest.raises((gzip.BadGzipFile, zlib.error, EOFError)):
        gzip.decompress(bad.read_bytes())
    good = tmp_path / "good.fq.gz"
    good.write_bytes(_bgzf(text, sizes=3000))
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(bad), str(good)], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = p.stdout.strip().split("\n")
    assert lines[0].startswith("ERROR mcaat error -4:"), lines  # MCAAT_E_IO
    assert str(bad) in lines[0] and f"member {2 if damage == 'payload_bit' else 1} " in lines[0], lines
    assert lines[1] == f"GOOD {len(seqs)} True", lines


# ---- 8. the CLI ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cli_reads_bgzf_like_the_plain_file(tmp_path):
    import mcaat_amd as M
    from tests.helpers import unpack_read

    packed, offs = M.synth_host(M.SynthSpec())  # C1 tiny, the CLI test's input
    text = "".join(f"@r{r}\n{s}\n+\n{'I' * len(s)}\n"
                   for r in range(len(offs) - 1) for s in [unpack_read(packed, int(offs[r]), int(offs[r + 1]))])
    plain = tmp_path / "reads.fq"
    plain.write_text(text)
    bgzf = _write_bgzf(tmp_path / "a.fq.gz", text)
    got = []
    for name, path in (("plain", str(plain)), ("bgzf", bgzf)):
        out = subprocess.run([CLI, "--input-files", path, "--output-folder", str(tmp_path / name), "--threads", "2",
                              "--ram", "2G"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        got.append((tmp_path / name / "CRISPR_Arrays.txt").read_text())
    assert got[0] == got[1] and "CRISPR" in got[0]
