"""node_counter without dead slots and sub rows in pass B.

Pass A (k_sk_scatter) sizes a workgroup's reservations by the work it has left (knob nc.a_adapt),
so fewer inert slots are written at the end of the kernel; pass B (k_l2_scatter) takes a
descriptor's liveness and fine sub-partition from the descriptor itself (desc_live, desc_sub in
csrc/desc_canon.h) instead of loading the 2-byte sub rows a second time.

No GPU: desc_live / desc_sub against a bit-string model, the same sweep as a stand-alone program
under AddressSanitizer and UndefinedBehaviorSanitizer, and the oracle against
helpers.brute_graph on the smallest input.

GPU: count_edges bit-exact against the CPU oracle for reads of E + 20 bases (one work item each)
drawn from a 20-kbp genome, at three read counts chosen for how many batches of 64 items a wave
of pass A gets on a 256-CU device (3 x 256 workgroups of 4 waves): 5 reads (most workgroups never
scan: every reservation is end-of-kernel tail), 98,304 (half the waves get one batch: sizing is
adaptive from the first flush) and 600,000 (about three batches per wave: the fixed-size phase
hands over to the adaptive one); crossed with nc.a_adapt {0, 1} and nc.a_mini {8, 64, default},
nc.l1_slots = 64 (resize and re-run) and nc.fine_bits {8, 12, 19} (l2_bits 0, 4 and 11). Then the
streamed input (reservations and their sizes carried from launch to launch), the slot accounting
(knob nc.a_stats), and a 2-rank build with the sender-side collapse at nc.fine_bits = 19 (the
weighted pass B)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import mcaat_amd as M
import oracle as O
from tests.helpers import brute_graph, lsb_value, rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SHIFT, H_SHIFT, H_BITS = 44, 50, 14
KS = (15, 21, 27, 30)
N_READS = (5, 98_304, 600_000)
GENOME = 20_000


# ---- desc_live / desc_sub (no GPU) ----------------------------------------------------------

def _model(w1, l2_bits):
    """w1 as a string of 64 bits, most significant first: n is bits 44..49, the sub the top l2_bits."""
    s = format(w1, "064b")
    n = int(s[64 - N_SHIFT - 6:64 - N_SHIFT], 2)
    return n != 0, (int(s[:l2_bits], 2) if l2_bits else 0)


def _words():
    rng = np.random.default_rng(16)
    all_hash = ((1 << H_BITS) - 1) << H_SHIFT
    bases = (1 << N_SHIFT) - 1
    for n in (0, 1, 27, 63):
        yield n << N_SHIFT
        yield (n << N_SHIFT) | all_hash  # all-ones hash bits
        yield (n << N_SHIFT) | all_hash | bases
        yield (n << N_SHIFT) | bases
        for h in range(H_BITS):
            yield (n << N_SHIFT) | (1 << (H_SHIFT + h))
        for x in rng.integers(0, 1 << 63, size=300, dtype=np.uint64):
            yield ((int(x) << 1) & ~(63 << N_SHIFT) & ((1 << 64) - 1)) | (n << N_SHIFT)
    for x in rng.integers(0, 1 << 63, size=2000, dtype=np.uint64):
        yield (int(x) << 1 | int(x) & 1) & ((1 << 64) - 1)
    yield 0
    yield (1 << 64) - 1


@pytest.mark.parametrize("l2_bits", [0, 1, 4, 11, 14])
def test_desc_sub_against_bit_string_model(l2_bits):
    seen_live = set()
    for w1 in _words():
        live, sub = M.desc_sub(w1, l2_bits)
        assert (live, sub) == _model(w1, l2_bits), (hex(w1), l2_bits)
        assert sub < (1 << l2_bits)
        seen_live.add(live)
    assert seen_live == {False, True}
    assert M.desc_sub(0, l2_bits) == (False, 0)  # a zero-filled slot is dead
    assert M.desc_sub(((1 << 64) - 1) & ~(63 << N_SHIFT), l2_bits) == (False, (1 << l2_bits) - 1)


def test_desc_sub_rejects_bad_bit_counts():
    for bad in (-1, H_BITS + 1, 64):
        with pytest.raises(M.McaatError):
            M.desc_sub(1 << N_SHIFT, bad)


def test_sanitized_standalone_sweep(tmp_path):
    exe = tmp_path / "desc_sub_test"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                    os.path.join(ROOT, "tests", "sanitize", "desc_sub_test.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "desc_sub ok" in p.stdout, (p.stdout + p.stderr)[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]


# ---- inputs and the oracle ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _genome_codes():
    return np.random.default_rng(2025).integers(0, 4, size=GENOME, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def read_codes(k, n_reads):
    """n_reads x L base codes: fragments of the genome, every fourth one reverse-complemented."""
    L = k + 1 + 20
    rng = np.random.default_rng(1000 * k + n_reads % 997)
    g = _genome_codes()
    starts = rng.integers(0, GENOME - L, size=n_reads)
    codes = g[starts[:, None] + np.arange(L)[None, :]]
    codes[::4] = 3 - codes[::4, ::-1]
    return codes


def _pack(codes):
    n, L = codes.shape
    flat = codes.reshape(-1).astype(np.uint64)
    flat = np.concatenate([flat, np.zeros((-flat.size) % 32, dtype=np.uint64)]).reshape(-1, 32)
    packed = (flat << (np.uint64(2) * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    return packed, np.arange(n + 1, dtype=np.uint64) * np.uint64(L)


@functools.lru_cache(maxsize=None)
def case(k, n_reads):
    """(packed, offsets, oracle keys, oracle counts) of one input, computed once and left unchanged."""
    packed, offs = _pack(read_codes(k, n_reads))
    ok, oc = O.count_canonical(packed, offs, k, threads=4)
    for a in (packed, offs, ok, oc):
        a.setflags(write=False)
    return packed, offs, ok, oc


@pytest.mark.parametrize("k", KS)
def test_oracle_equals_brute_force(k):
    """No GPU: on the 5-read input the oracle's canonical counts are the pure-Python restatement's."""
    _, _, ok, oc = case(k, N_READS[0])
    seqs = ["".join("ACGT"[c] for c in row) for row in read_codes(k, N_READS[0])]
    edges, mult = brute_graph(seqs, k)
    want = {}
    for e in edges:
        r = rc(e)
        want[min(lsb_value(e), lsb_value(r))] = mult[e] // (2 if e == r else 1)
    assert ok.size == len(want) > 50
    assert np.all(ok[1:] > ok[:-1])
    assert dict(zip(ok.tolist(), oc.tolist())) == want


def test_read_counts_match_their_purpose():
    """No GPU: batches per wave of pass A on a 256-CU device for the three read counts."""
    waves = 3 * 256 * 4
    batches = [(n + 63) // 64 for n in N_READS]
    assert batches[0] == 1
    assert batches[1] * 2 == waves
    assert 3 * waves <= batches[2] < 4 * waves
    for k in KS:
        assert read_codes(k, N_READS[0]).shape == (5, k + 21)  # one work item per read


# ---- GPU: parity under the knobs ------------------------------------------------------------

KNOB_GROUPS = {
    "mini": [{"nc.a_adapt": a, **m} for a in (0, 1) for m in ({"nc.a_mini": 8}, {"nc.a_mini": 64}, {})],
    "resize": [{"nc.a_adapt": a, "nc.l1_slots": 64} for a in (0, 1)],
    "fine": [{"nc.a_adapt": a, "nc.fine_bits": f} for a in (0, 1) for f in (8, 12, 19)],
}


def _count(ctx, k, n_reads, knobs):
    packed, offs, ok, oc = case(k, n_reads)
    reads = M.Reads.from_host(ctx, packed, offs)
    try:
        with ctx.knobs(**{n.replace(".", "__"): v for n, v in knobs.items()}):
            gk, gc = M.count_edges(ctx, reads, k)
    finally:
        reads.free()
    assert gk.size == ok.size, (k, n_reads, knobs, gk.size, ok.size)
    assert np.array_equal(gk, ok), (k, n_reads, knobs)
    assert np.array_equal(gc, oc), (k, n_reads, knobs)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n_reads", N_READS)
@pytest.mark.parametrize("group", sorted(KNOB_GROUPS))
def test_count_edges_equals_oracle(gpu_ctx, k, n_reads, group):
    for knobs in KNOB_GROUPS[group]:
        _count(gpu_ctx, k, n_reads, knobs)


# ---- GPU: streamed input --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("adapt", [0, 1])
def test_streamed_input_equals_one_launch(gpu_ctx, tmp_path, monkeypatch, adapt):
    """Pass A part by part while the input is read (rmode 1, 2, 2, ... 3: the prefetched reservation
    and its size travel in rstate), a last file of five reads giving a part of a few reads; the
    counts equal those of one launch over the same reads, and the oracle's."""
    from tests.test_fastq_ingest import _fastq_text, _packed_by_host, _write

    k = 27
    codes = read_codes(k, N_READS[1])[:6005]
    seqs = ["".join("ACGT"[c] for c in row) for row in codes]
    paths = [_write(tmp_path / "a.fq", _fastq_text(seqs[:6000])), _write(tmp_path / "b.fq", _fastq_text(seqs[6000:]))]
    monkeypatch.setenv("MCAAT_PACK_THREADS", "3")
    with gpu_ctx.knobs(nc__a_adapt=adapt):
        gpu_ctx.reset_timing()
        gpu_ctx.count_ahead(k)
        r = M.Reads.from_fastx(gpu_ctx, paths)
        assert _packed_by_host(gpu_ctx)
        launches = gpu_ctx.kernel_timing("sk_scatter_ahead")[1]
        k1, c1 = M.count_edges(gpu_ctx, r, k)
        assert gpu_ctx.kernel_timing("sk_scatter")[1] == 0  # the first count took the streamed buckets
        launches = gpu_ctx.kernel_timing("sk_scatter_ahead")[1]
        k0, c0 = M.count_edges(gpu_ctx, r, k)
        assert gpu_ctx.kernel_timing("sk_scatter")[1] == 1
    r.free()
    print("streamed launches:", launches)
    assert launches >= 4, launches  # three parts or more, and the closing launch
    assert np.array_equal(k1, k0) and np.array_equal(c1, c0)
    packed, offs = _pack(codes)
    ok, oc = O.count_canonical(packed, offs, k, threads=4)
    assert np.array_equal(k0, ok) and np.array_equal(c0, oc)


# ---- GPU: slot accounting -------------------------------------------------------------------

def _slots(ctx, k, n_reads, adapt):
    packed, offs, ok, oc = case(k, n_reads)
    reads = M.Reads.from_host(ctx, packed, offs)
    try:
        with ctx.knobs(nc__a_adapt=adapt, nc__a_stats=1):
            ctx.reset_timing()
            gk, gc = M.count_edges(ctx, reads, k)
            s = {n: ctx.kernel_timing("a_slots_" + n)[1] for n in ("reserved", "live", "dead_switch", "dead_end")}
    finally:
        reads.free()
    assert np.array_equal(gk, ok) and np.array_equal(gc, oc)
    return s


@pytest.mark.gpu
def test_slot_accounting(gpu_ctx):
    """Every reserved slot is a live descriptor or an inert one, written at a reservation switch or
    at the end of the kernel; sizing by the work left leaves strictly fewer inert slots. The
    ratio is printed, not fixed (on a 256-CU device: 2,083,692 live slots; 400,168,084 inert
    ones at fixed size, 27,857,044 adaptive, ratio 0.070; none at switches)."""
    k, n = 27, N_READS[2]
    fixed, adapt = _slots(gpu_ctx, k, n, 0), _slots(gpu_ctx, k, n, 1)
    for s in (fixed, adapt):
        assert s["live"] > 0
        assert s["live"] + s["dead_switch"] + s["dead_end"] == s["reserved"], s
    assert fixed["live"] == adapt["live"]
    dead = [s["dead_switch"] + s["dead_end"] for s in (fixed, adapt)]
    print("slots, nc.a_adapt=0:", fixed, "\nslots, nc.a_adapt=1:", adapt,
          "\ndead adaptive / dead fixed: %.4f" % (dead[1] / dead[0]))
    assert dead[1] < dead[0]


# ---- GPU: weighted pass B -------------------------------------------------------------------

@pytest.mark.gpu
def test_preagg_two_ranks_at_2048_subs():
    """Two shared-memory ranks with the sender-side collapse and nc.fine_bits = 19: the owners'
    weighted pass B takes 11-bit subs from the descriptors (graph and CycleFinder results equal
    the one-GPU path's, tools/native_multi_check.py)."""
    from tests.test_preagg import _assert_ok, _ranks

    _assert_ok(_ranks(2, ("--knob", "nc.fine_bits=19")))
