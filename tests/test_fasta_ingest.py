"""GPU FASTA ingest (csrc/fastq_ingest.hip, ingest_fasta: multi-line records parsed by line on
the device and split over ranks) against the kseq restatement of the read library
(oracle/fastx.py kseq_sequences, then counting_view / mapping_view / pack_bases / pack_codes).

Bar: bit-exact packed words up to the last base, and both offset arrays. Records are wrapped at
widths around the 32-base word and the 64-byte segment, with empty lines inside them, headers
that hold '>', '@' and '+', LF and CRLF; the chunk size is forced down (MCAAT_FASTQ_CHUNK) so
records straddle chunks and the carry runs many times. kernel_timing("fa_emit") tells which
path ran (the device parser's emit kernel), as "fq_concat" does for the FASTQ host packer.
"""
import bz2
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

from oracle import fastx as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mcaat_amd", "mcaat")
ALPHA = "ACGT" * 6 + "acgtNRY"
WIDTHS = (1, 7, 31, 32, 33, 60, 64, 80)


def _rand_records(rng, n, max_len=300):
    seqs = []
    for i in range(n):
        L = int(rng.integers(0, max_len)) if i % 17 else 0
        s = "".join(rng.choice(list(ALPHA if i % 5 == 0 else "ACGT"), size=L))
        seqs.append(s)
    return seqs


def _fasta_text(seqs, rng, crlf=False, final_newline=True):
    """Headers '>r{i} x>y @z +w', each record wrapped at a width drawn from WIDTHS, an empty
    line after about 1 line in 9, two empty lines before and after the text."""
    nl = "\r\n" if crlf else "\n"
    lines = []
    for i, s in enumerate(seqs):
        lines.append(f">r{i} x>y @z +w")
        w = int(rng.choice(WIDTHS))
        for p in range(0, len(s), w):
            lines.append(s[p:p + w])
            if rng.integers(0, 9) == 0:
                lines.append("")
    body = nl.join(lines)
    return "\n\n" + body + (nl + "\n\n" if final_newline else "")


def _write(path, text, gz=False):
    data = text.encode()
    if gz == "bz2":  # two concatenated bzip2 streams (as pbzip2 writes), split mid-record
        h = len(data) // 2
        with open(path, "wb") as f:
            f.write(bz2.compress(data[:h]) + bz2.compress(data[h:]))
    elif gz:
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        with open(path, "wb") as f:
            f.write(data)
    return str(path)


def _set_chunk(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("MCAAT_FASTQ_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("MCAAT_FASTQ_CHUNK", raising=False)


def _want(per_file):
    want_p, want_o = FX.pack_bases(FX.counting_view([s for f in per_file for s in f]))
    want_qp, want_qo = FX.pack_codes(FX.mapping_view(per_file))
    return want_p, want_o, want_qp, want_qo


def _assert_library(reads, per_file):
    want_p, want_o, want_qp, want_qo = _want(per_file)
    p, o = reads.download()
    assert np.array_equal(o, want_o)
    nw = (int(want_o[-1]) + 31) // 32
    assert np.array_equal(p[:nw], want_p[:nw])
    qp, qo = reads.download_records()
    assert np.array_equal(qo, want_qo)
    nq = (int(want_qo[-1]) + 31) // 32
    assert np.array_equal(qp[:nq], want_qp[:nq])


def _separate(per_file):
    """The mapping view is kept apart when a record is not exactly one upper-case ACGT run, or
    a file after the first has a record."""
    one_run = all(len(s) > 0 and set(s) <= set("ACGT") for f in per_file for s in f)
    return any(len(f) > 0 for f in per_file[1:]) or not one_run


def _check(ctx, files, texts):
    import mcaat_amd as M

    per_file = [FX.kseq_sequences(t) for t in texts]
    reads = M.Reads.from_fastx(ctx, files)
    _assert_library(reads, per_file)
    return reads, per_file


def _device_path_ran(ctx):
    return ctx.kernel_timing("fa_emit")[1] > 0


@functools.lru_cache(maxsize=None)
def _case1_text(crlf, final_newline):
    rng = np.random.default_rng(101 + 2 * crlf + final_newline)
    return _fasta_text(_rand_records(rng, 400), rng, crlf=crlf, final_newline=final_newline)


# ---- the generator (CPU): its texts read back through the restatement as generated -------------

def test_generator_reads_back_through_kseq():
    rng = np.random.default_rng(1)
    seqs = _rand_records(rng, 400)
    for crlf in (False, True):
        for final_newline in (False, True):
            text = _fasta_text(seqs, rng, crlf=crlf, final_newline=final_newline)
            assert FX.kseq_sequences(text) == seqs
    assert any(s == "" for s in seqs) and any(set(s) - set("ACGT") for s in seqs)


# ---- 1. chunked single file ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("final_newline", [True, False])
@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("chunk", [256, 1000, 4099, 0])
def test_single_file_chunked(gpu_ctx, tmp_path, monkeypatch, chunk, crlf, final_newline):
    _set_chunk(monkeypatch, chunk)
    text = _case1_text(crlf, final_newline)
    gpu_ctx.reset_timing()
    reads, per_file = _check(gpu_ctx, [_write(tmp_path / "a.fa", text)], [text])
    assert _device_path_ran(gpu_ctx)
    assert reads.records_info() == (400, _separate(per_file))
    assert reads.file_records(0) == 400
    reads.free()


# ---- 2. hand-written edge texts -----------------------------------------------------------------

EDGE_TEXTS = {
    "run_crosses_line_break": ">a\nACG\nTTA\n>b\nGG\n",
    "n_first_and_last_of_a_line": ">a\nNACG\nTTAN\nNAC\nGT\nAN\nC\n",
    "run_crosses_empty_line": ">a\nACG\n\n\nTTA\n\n>b\n\nGG\n",
    "line_of_only_cr": ">a\r\nACG\r\n\r\nTT\r\n>b\r\n\r\n",
    "space_and_tab": ">a\nAC GT\nA\tC\n \nGG\n",
    "consecutive_headers": ">a\n>b\n>c\nACGT\n>d\n>e\n",
    "header_last": ">a\nACGT\n>b",
    "header_only": ">a\n",
    "lower_case_single_run": ">a\nacgt\nACGT\n",
    "blank_tail_line": ">a\nACGT\n \n",
    "line_64_and_65": ">a\n" + "ACGT" * 16 + "\n" + "ACGT" * 16 + "A\n>b\n" + "C" * 65 + "\n" + "G" * 64 + "\n" + "T" * 63
                      + "\n>c\n" + "AC" * 32 + "\n",
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGE_TEXTS))
def test_edge_texts(gpu_ctx, tmp_path, monkeypatch, name):
    _set_chunk(monkeypatch, 256)
    text = EDGE_TEXTS[name]
    files = [_write(tmp_path / "a.fa", text), _write(tmp_path / "b.fa", text)]  # b: reverse-complemented
    gpu_ctx.reset_timing()
    reads, per_file = _check(gpu_ctx, files, [text, text])
    assert _device_path_ran(gpu_ctx)
    assert reads.records_info() == (2 * len(per_file[0]), True)
    reads.free()
    reads, per_file = _check(gpu_ctx, files[:1], [text])
    assert reads.records_info() == (len(per_file[0]), _separate(per_file))
    reads.free()


@pytest.mark.gpu
def test_known_answers(gpu_ctx, tmp_path, monkeypatch):
    """The restatement's own reading of three of the texts, spelled out."""
    assert FX.kseq_sequences(EDGE_TEXTS["run_crosses_empty_line"]) == ["ACGTTA", "GG"]
    assert FX.counting_view(FX.kseq_sequences(EDGE_TEXTS["n_first_and_last_of_a_line"])) == ["ACGTTA", "ACGTA", "C"]
    assert FX.kseq_sequences(EDGE_TEXTS["consecutive_headers"]) == ["", "", "ACGT", "", ""]
    # a header-only record: no read in the counting view, one empty entry in the mapping view
    _set_chunk(monkeypatch, 256)
    text = EDGE_TEXTS["consecutive_headers"]
    reads, _ = _check(gpu_ctx, [_write(tmp_path / "a.fa", text)], [text])
    assert reads.info() == (1, 4) and reads.records_info() == (5, True)
    reads.free()


@pytest.mark.gpu
def test_record_above_the_reserve_goes_to_the_host_reader(gpu_ctx, tmp_path, monkeypatch):
    """6000 symbols at chunk 256 exceed the 4096-byte carry reserve: same library, host reader."""
    _set_chunk(monkeypatch, 256)
    rng = np.random.default_rng(4)
    big = "".join(rng.choice(list("ACGTN"), size=6000))
    text = ">s\nACGT\n>big\n" + "\n".join(big[p:p + 60] for p in range(0, 6000, 60)) + "\n>t\nGGA\n"
    reads, per_file = _check(gpu_ctx, [_write(tmp_path / "a.fa", text)], [text])
    assert per_file[0] == ["ACGT", big, "GGA"]
    reads.free()


# ---- 3. paired ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("gz", [False, True, "bz2"])
def test_paired_files(gpu_ctx, tmp_path, monkeypatch, gz):
    _set_chunk(monkeypatch, 777)
    rng = np.random.default_rng(5)
    t1 = _fasta_text(_rand_records(rng, 300), rng, crlf=True)
    t2 = _fasta_text(_rand_records(rng, 300), rng, final_newline=False)
    sfx = ".fa.bz2" if gz == "bz2" else ".fa.gz" if gz else ".fa"
    files = [_write(tmp_path / ("r1" + sfx), t1, gz), _write(tmp_path / ("r2" + sfx), t2, gz)]
    gpu_ctx.reset_timing()
    reads, _ = _check(gpu_ctx, files, [t1, t2])
    assert _device_path_ran(gpu_ctx)
    assert reads.records_info() == (600, True)
    assert [reads.file_records(f) for f in (0, 1)] == [300, 300]
    reads.free()


@pytest.mark.gpu
def test_empty_mate(gpu_ctx, tmp_path, monkeypatch):
    _set_chunk(monkeypatch, 777)
    rng = np.random.default_rng(6)
    seqs = ["".join(rng.choice(list("ACGT"), size=90)) for _ in range(50)]
    t1 = _fasta_text(seqs, rng)
    files = [_write(tmp_path / "r1.fa", t1), _write(tmp_path / "r2.fa", "")]
    gpu_ctx.reset_timing()
    reads, _ = _check(gpu_ctx, files, [t1, ""])
    assert _device_path_ran(gpu_ctx)
    assert reads.records_info() == (50, False)  # no record in the mate: the counting view serves
    assert [reads.file_records(f) for f in (0, 1)] == [50, 0]
    reads.free()


# ---- 4. declines --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [256, 0])
def test_fastq_grammar_inside_fasta_is_read_like_kseq(gpu_ctx, tmp_path, monkeypatch, chunk):
    """A sequence line that starts with '@' opens a record under kseq, one that starts with '+' a
    quality block: the device parser declines and the host reader gives the restatement's result."""
    _set_chunk(monkeypatch, chunk)
    rng = np.random.default_rng(8)
    good = _fasta_text(_rand_records(rng, 40), rng)
    at = ">a\nACGT\n@CGT\nAAAA\n>b\nTT\n"
    assert FX.kseq_sequences(at) == ["ACGT", "AAAA", "TT"]
    plus = ">a\nACGT\nAC\n+\nIIIIII\n>b\nTT\n"
    assert FX.kseq_sequences(plus) == ["ACGTAC", "TT"]
    fastq = "@q\nACGTN\n+\nIIIII\n"
    cases = {"at": [at], "plus": [plus], "late_at": [good + at], "late_plus": [good.rstrip("\n") + "\n" + plus],
             "mixed": [good, fastq], "mixed_first": [fastq, good]}
    for name, texts in cases.items():
        files = [_write(tmp_path / f"{name}{i}.fa", t) for i, t in enumerate(texts)]
        reads, _ = _check(gpu_ctx, files, texts)
        reads.free()


# ---- 5. fa.gpu = 0 equals fa.gpu = 1 ------------------------------------------------------------

@pytest.mark.gpu
def test_knob_off_matches_on(gpu_ctx, tmp_path, monkeypatch):
    import mcaat_amd as M

    _set_chunk(monkeypatch, 1000)
    path = _write(tmp_path / "a.fa", _case1_text(False, True))
    got = []
    for on in (1, 0):
        with gpu_ctx.knobs(fa__gpu=on):
            gpu_ctx.reset_timing()
            r = M.Reads.from_fastx(gpu_ctx, [path])
            assert _device_path_ran(gpu_ctx) == bool(on)
            got.append((r.download(), r.download_records(), r.info(), r.records_info()))
            r.free()
    (p1, o1), (q1, qo1), i1, s1 = got[0]
    (p0, o0), (q0, qo0), i0, s0 = got[1]
    nw, nq = (int(o1[-1]) + 31) // 32, (int(qo1[-1]) + 31) // 32
    assert i1 == i0 and s1 == s0
    assert np.array_equal(o1, o0) and np.array_equal(p1[:nw], p0[:nw])
    assert np.array_equal(qo1, qo0) and np.array_equal(q1[:nq], q0[:nq])


# ---- 6. fixed length ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_acgt_only_is_the_counting_view(gpu_ctx, tmp_path, monkeypatch):
    _set_chunk(monkeypatch, 2048)
    rng = np.random.default_rng(7)
    seqs = ["".join(rng.choice(list("ACGT"), size=150)) for _ in range(500)]
    text = "".join(f">r{i}\n{s}\n" for i, s in enumerate(seqs))
    gpu_ctx.reset_timing()
    reads, _ = _check(gpu_ctx, [_write(tmp_path / "a.fa", text)], [text])
    assert _device_path_ran(gpu_ctx)
    assert reads.info() == (500, 75000)
    assert reads.records_info() == (500, False)
    reads.free()


# ---- 7. parts -----------------------------------------------------------------------------------

N_PART_RECORDS = 200


@functools.lru_cache(maxsize=None)
def _parts_texts():
    rng = np.random.default_rng(13)
    return (_fasta_text(_rand_records(rng, N_PART_RECORDS), rng),
            _fasta_text(_rand_records(rng, N_PART_RECORDS // 2), rng, crlf=True, final_newline=False))


def _codes(packed, offs, lo, hi):
    """Records [lo, hi) of a mapping view: their lengths and their symbols."""
    idx = np.arange(int(offs[lo]), int(offs[hi]), dtype=np.uint64)
    sym = (packed[(idx >> np.uint64(5)).astype(np.int64)] >> (np.uint64(2) * (idx & np.uint64(31)))) & np.uint64(3)
    return np.diff(offs[lo:hi + 1].astype(np.int64)), sym


@pytest.mark.gpu
@pytest.mark.parametrize("n_files", [1, 2])
@pytest.mark.parametrize("n_parts", [2, 3, 8, N_PART_RECORDS + 57])
def test_parts_partition_the_records(gpu_ctx, tmp_path, monkeypatch, n_parts, n_files):
    """Per file, the parts' mapping-view records in part order are the whole file's records; the
    records per file and the bases add up (as tests/test_native_multi.py compares FASTQ parts)."""
    import mcaat_amd as M

    _set_chunk(monkeypatch, 4099)
    texts = list(_parts_texts()[:n_files])
    files = [_write(tmp_path / f"r{i}.fa", t) for i, t in enumerate(texts)]
    per_file = [FX.kseq_sequences(t) for t in texts]
    n_file = [len(f) for f in per_file]
    _, want_o, wrp, wro = _want(per_file)
    gpu_ctx.reset_timing()
    parts = [M.Reads.from_fastx_part(gpu_ctx, files, part, n_parts) for part in range(n_parts)]
    assert _device_path_ran(gpu_ctx)
    got_file = np.zeros(n_files, dtype=np.int64)
    views = []
    for pr in parts:
        nf = [pr.file_records(f) for f in range(n_files)]
        got_file += nf
        views.append((nf, *pr.download_records()))
    assert got_file.tolist() == n_file
    wl = 0
    for f in range(n_files):
        want_len, want_sym = _codes(wrp, wro, wl, wl + n_file[f])
        wl += n_file[f]
        lens, syms = [], []
        for nf, rp, ro in views:
            lo = sum(nf[:f])
            ln, sy = _codes(rp, ro, lo, lo + nf[f])
            lens.append(ln)
            syms.append(sy)
        assert np.array_equal(np.concatenate(lens), want_len), (n_parts, f)
        assert np.array_equal(np.concatenate(syms), want_sym), (n_parts, f)
    assert sum(pr.info()[1] for pr in parts) == int(want_o[-1])
    for pr in parts:
        pr.free()


@pytest.mark.gpu
def test_compressed_fasta_goes_whole_to_part_0(gpu_ctx, tmp_path, monkeypatch):
    import mcaat_amd as M

    _set_chunk(monkeypatch, 4099)
    text = _parts_texts()[0]
    files = [_write(tmp_path / "r.fa.gz", text, True)]
    per_file = [FX.kseq_sequences(text)]
    parts = [M.Reads.from_fastx_part(gpu_ctx, files, part, 3) for part in range(3)]
    assert [p.file_records(0) for p in parts] == [N_PART_RECORDS, 0, 0]
    _assert_library(parts[0], per_file)
    assert parts[1].info() == (0, 0) and parts[2].info() == (0, 0)
    for p in parts:
        p.free()


@pytest.mark.gpu
def test_parts_of_unsplittable_inputs_are_refused(gpu_ctx, tmp_path, monkeypatch):
    """A part that meets kseq's FASTQ grammar, or FASTA with the knob off, is an error (the
    caller reads the input whole), never a guess."""
    import mcaat_amd as M

    _set_chunk(monkeypatch, 4099)
    bad = _write(tmp_path / "bad.fa", ">a\nACGT\n@CGT\nAAAA\n>b\nTT\n")
    with pytest.raises(RuntimeError):
        M.Reads.from_fastx_part(gpu_ctx, [bad], 0, 2)
    good = _write(tmp_path / "good.fa", _parts_texts()[0])
    with gpu_ctx.knobs(fa__gpu=0):
        with pytest.raises(RuntimeError):
            M.Reads.from_fastx_part(gpu_ctx, [good], 0, 2)


# ---- 8. the CLI: FASTA over two ranks equals FASTQ on one GPU -------------------------------------

@pytest.mark.gpu
def test_cli_fasta_on_two_ranks_equals_fastq_on_one(tmp_path):
    import mcaat_amd as M
    from tests.helpers import unpack_read

    spec = M.SynthSpec()
    packed, offs = M.synth_host(spec)
    seqs = [unpack_read(packed, int(offs[i]), int(offs[i + 1])) for i in range(len(offs) - 1)]
    fa, fq = tmp_path / "x.fa", tmp_path / "x.fq"
    with open(fa, "w") as f:
        for i, s in enumerate(seqs):
            f.write(f">r{i}\n" + "".join(s[p:p + 60] + "\n" for p in range(0, len(s), 60)))
    with open(fq, "w") as f:
        for i, s in enumerate(seqs):
            f.write(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n")
    runs = {}
    for name, path, multi in (("fa", fa, ["--gpus", "2", "--comm", "shm"]), ("fq", fq, [])):
        out = subprocess.run([CLI, "-i", str(path), "--output-folder", str(tmp_path / name), "--threads", "2", "--ram",
                              "2G", *multi], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr + out.stdout[-2000:]
        runs[name] = ((tmp_path / name / "CRISPR_Arrays.txt").read_text(), out.stdout)
    assert "Inputs read whole on rank 0" not in runs["fa"][1]
    assert runs["fa"][0] == runs["fq"][0]
    assert "Number of Systems: 2" in runs["fa"][0]
