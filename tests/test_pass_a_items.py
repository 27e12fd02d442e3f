"""node_counter pass A (k_sk_scatter) at the places its item fetch can go wrong.

A lane of pass A scans one work item: up to 127 edge positions of one read, loaded once as six
words of the packed stream, shifted to base 0 and then walked 8 positions per step, the
registers moving down by one every second step. The inputs below put reads where that fetch,
the alignment and the walk change behaviour: no position, one position, a step boundary, every
value of (first base) mod 32, exactly one full item, a second item of one position, several
items per read, a partial last batch, variable-length reads (the explicit item list), and
low-complexity reads whose super-k-mers are closed by the descriptor's length limit.

count_edges is compared exactly with the CPU oracle; a CPU test checks the oracle itself against
helpers.brute_graph on the small inputs, so the expectations do not come from the code under
test. k = 30 (the largest the library accepts; m = 16, the unmasked m-mer path) stands in for 31.
"""
import functools

import numpy as np
import pytest

import oracle as O
from tests.helpers import brute_graph, lsb_value, pack_reads, rc

KS = (15, 21, 27, 30)
N_READS = 64 * 3 + 5  # three full batches of 64 items and a partial one
ITEM = 127            # edge positions per work item
DESC_BASES = 54       # bases a descriptor holds: a super-k-mer is closed at DESC_BASES - E + 1 edges
KNOBS = {"a_mini8": {"nc.a_mini": 8}, "l1_resize": {"nc.l1_slots": 64}}


def fixed_lengths(k):
    E = k + 1
    return (E - 1, E, E + 7, E + 8, 149, 150, 151, ITEM + E - 1, ITEM + E, 300)


def _genome(seed, n):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), size=n))


def _low_complexity(rng, L, i):
    """A read of L bases around a homopolymer or dinucleotide run longer than DESC_BASES (the
    whole read when L is shorter than that)."""
    unit = ("A", "T", "AC", "GT", "C", "AT")[i % 6]
    run = min(L, DESC_BASES + 9 + 5 * (i % 7))
    left = int(rng.integers(0, L - run + 1))
    flank = "".join(rng.choice(list("ACGT"), size=L - run))
    return flank[:left] + (unit * run)[:run] + flank[left:]


@functools.lru_cache(maxsize=None)
def fixed_reads(k, L):
    """N_READS reads of L bases: fragments of a 3 kbp genome (so edges repeat), one fragment
    planted six times, twelve low-complexity reads, an all-A and an all-T read."""
    rng = np.random.default_rng(1000 * k + L)
    g = _genome(7, 3000)
    seqs = [g[a:a + L] for a in rng.integers(0, len(g) - L, size=N_READS - 20)]
    seqs += [seqs[3]] * 3 + [rc(seqs[3])] * 3
    seqs += [_low_complexity(rng, L, i) for i in range(12)]
    seqs += ["A" * L, "T" * L]
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    assert len(seqs) == N_READS and all(len(s) == L for s in seqs)
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def variable_reads(k):
    """Every length 1..400 once, in random order (lengths below E give no item), then planted
    repeats, low-complexity reads and an all-A and an all-T read of assorted lengths."""
    rng = np.random.default_rng(77 + k)
    g = _genome(8, 4000)
    seqs = []
    for L in rng.permutation(400) + 1:
        a = int(rng.integers(0, len(g) - L))
        seqs.append(g[a:a + L])
    seqs += [seqs[5], rc(seqs[5]), g[100:333], g[100:333], rc(g[100:333])]
    seqs += [_low_complexity(rng, int(L), i) for i, L in enumerate(rng.integers(60, 400, size=10))]
    seqs += ["A" * 211, "T" * 97, "A" * (k + 1), "T" * k]
    return tuple(seqs)


def _reads(k, L):
    return variable_reads(k) if L == "var" else fixed_reads(k, L)


@functools.lru_cache(maxsize=None)
def case(k, L):
    """(packed, offsets, oracle keys, oracle counts) of one input, computed once."""
    packed, offs = pack_reads(list(_reads(k, L)))
    ok, oc = O.count_canonical(packed, offs, k, threads=4)
    return packed, offs, ok, oc


def _brute_canonical(seqs, k):
    edges, mult = brute_graph(seqs, k)
    out = {}
    for e in edges:
        r = rc(e)
        out[min(lsb_value(e), lsb_value(r))] = mult[e] // (2 if e == r else 1)
    return out


@pytest.mark.parametrize("k", KS)
def test_oracle_equals_brute_force(k):
    """No GPU: the oracle's canonical counts are those of the pure-Python restatement, on the
    short fixed-length inputs and on the variable-length one."""
    E = k + 1
    for L in (E - 1, E, E + 7, E + 8, "var"):
        _, _, ok, oc = case(k, L)
        want = _brute_canonical(_reads(k, L), k)
        assert ok.size == len(want), (k, L)
        assert np.all(ok[1:] > ok[:-1]), (k, L)
        assert dict(zip(ok.tolist(), oc.tolist())) == want, (k, L)
    assert case(k, E - 1)[2].size == 0
    assert case(k, E)[2].size > 100


def test_inputs_cover_the_alignments():
    """No GPU: the odd lengths start reads at every base offset mod 32, the long runs exceed a
    descriptor, and the lengths sit on the item boundaries they are meant to."""
    for k in KS:
        E = k + 1
        for L in (149, 151):
            assert {(r * L) & 31 for r in range(N_READS)} == set(range(32))
        npos = [L - E + 1 for L in fixed_lengths(k)]
        assert npos[:4] == [0, 1, 8, 9] and npos[7:9] == [ITEM, ITEM + 1]
        assert (npos[9] + ITEM - 1) // ITEM >= 3
        assert any("A" * (DESC_BASES + 1) in s or "T" * (DESC_BASES + 1) in s for s in fixed_reads(k, 150))
        lens = sorted(len(s) for s in variable_reads(k)[:400])
        assert lens == list(range(1, 401))


def _count(ctx, k, L):
    import mcaat_amd as M

    packed, offs, ok, oc = case(k, L)
    gk, gc = M.count_edges(ctx, M.Reads.from_host(ctx, packed, offs), k)
    assert gk.size == ok.size, (k, L, gk.size, ok.size)
    assert np.array_equal(gk, ok), (k, L)
    assert np.array_equal(gc, oc), (k, L)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("which", range(10))
def test_fixed_length(gpu_ctx, k, which):
    _count(gpu_ctx, k, fixed_lengths(k)[which])


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_variable_length(gpu_ctx, k):
    _count(gpu_ctx, k, "var")


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("knobset", sorted(KNOBS))
def test_same_inputs_under_knobs(gpu_ctx, k, knobset):
    """Reservations of 8 slots, and L1 regions too small for the first run (pass A runs twice)."""
    with gpu_ctx.knobs(**{n.replace(".", "__"): v for n, v in KNOBS[knobset].items()}):
        for L in fixed_lengths(k) + ("var",):
            _count(gpu_ctx, k, L)
