"""Every k the C ABI accepts (2..30) through counting, the SDBG build, CycleFinder and read mapping.

Several code paths are chosen by k alone, and the rest of the suite runs the GPU at a handful of k:
  * node_counter's minimizer length (sk_params): m = 3 for E = k+1 <= 11, E-8 for E = 12..21, 14 for
    E = 22..28, 15 at E = 29, 16 at E = 30, 31; the window is w = E-m+1 (1 at k = 2, 16 at k = 30).
    Odd and even m differ in whether an m-mer can be its own reverse complement, which the canonical
    orientation of a super-k-mer depends on;
  * the MSD edge sort (5 <= k <= 28, D >= 65536): its level widths 2E-11 and 2E-22 are small or
    negative at small k (a level-3 bucket then holds at most one real item), and at k = 28 the item
    word is full (47 remainder bits + 16 multiplicity bits beside the padding value);
  * the label directory (B = min(lg D - 3, 2E, 30) bits, shift 2E-B): shift 0 and a directory as wide
    as the key space at small k, and the clamps at the top of the key space (k_own_bounds,
    dev_index_search) that only a label ending the order in a run of T reaches.

Everything is bit-exact against the CPU oracle; the CPU part checks the oracle itself against
helpers.brute_graph / brute_neighbors at all 29 values of k on the same input, and that the inputs
reach what the sweep claims (test_sweep_covers_what_it_claims).

Inputs (seeded, generated here):
  mixed    300 segments of a 1.5 kbp genome, every length 1..140 at least once (reads shorter than,
           equal to and longer than k+1 at every k), every second one reverse-complemented, plus
           homopolymers, self-reverse-complement repeats and reads whose labels sit at both ends of
           the key space. D = 64 (k = 2, the complete graph) .. ~2900.
  arrays   a 3 kbp genome with one planted array (repeat 30, eight spacers of 32), 1500 reads of
           100 bp plus "T"*120 and "A"*100+"C"; CycleFinder at threshold_multiplicity 5,
           low_abundance.
  dense_k  k = 7..11: uniform random 150-bp reads, D >= 65536 so the default build takes the MSD
           sort where the level-3 width is negative (k <= 9) or just positive; at k = 7 the complete
           graph (D = 4^8: every node four out- and four in-edges).
"""
import functools

import numpy as np
import pytest

import oracle as O
from tests.helpers import boss_key, brute_graph, brute_neighbors, lsb_value, pack_reads, rc

KS = tuple(range(2, 31))
# CycleFinder and mapping start at k = 8: below it the `arrays` graph is dense and the oracle's
# search alone takes minutes (measured: 418 s at k = 7, 329 s at k = 3, 75 s at k = 2; 0.01-0.5 s
# at every k in 8..30). k = 2..7 are excluded from those two stages for that reason only.
CF_KS = tuple(range(8, 31))
DENSE = {7: 6000, 8: 3000, 9: 1500, 10: 1500, 11: 1500}  # k -> number of 150-bp reads
CF = dict(threshold_multiplicity=5, low_abundance=True)
FIXED = ("A" * 70, "T" * 70, "ACGTACGT" * 10, "AT" * 40, "ACGT" * 20, "T" * 33 + "G", "C" + "T" * 64)

GRAPH_KNOBS = {
    "default": {},
    "radix": {"sort.msd": 0},
    "msd": {"sort.msd": 1},  # k <= 28 only (the radix sort takes 29 and 30 whatever the knob says)
    "msd_bitonic": {"sort.msd": 1, "sort.l3_counting": 0},
    "msd_listed": {"sort.msd": 1, "sort.wave_limit": 0},
    "adj_global": {"sdbg.adj_lds": 0},
    "adj_cap0": {"sdbg.adj_cap": 0},
}
GRAPH_CASES = [(k, n) for k in KS for n in GRAPH_KNOBS if not (n == "msd" and k > 28)]


def minimizer_len(k):
    """sk_params' m, restated from its description (not from its code's output)."""
    E = k + 1
    if E <= 11:
        return 3
    if E <= 21:
        return E - 8
    return 14 if E <= 28 else 15 if E == 29 else 16


# ---- inputs -----------------------------------------------------------------------------------
_LUT = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _LUT[ord(_c)] = _i


def _genome(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def _pack_codes(codes):
    """list of 2-bit code arrays -> (packed, offsets) in helpers.pack_reads' layout, vectorised
    (test_oracle_matches_bruteforce checks it against pack_reads itself)."""
    offs = np.zeros(len(codes) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(c) for c in codes], dtype=np.uint64)
    total = int(offs[-1])
    nw = (total + 31) // 32
    flat = np.zeros(nw * 32, dtype=np.uint64)
    flat[:total] = np.concatenate(codes)
    words = np.bitwise_or.reduce(flat.reshape(nw, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1)
    return words, offs


def _pack_seqs(seqs):
    return _pack_codes([_LUT[np.frombuffer(s.encode(), dtype=np.uint8)] for s in seqs])


@functools.lru_cache(maxsize=None)
def mixed_reads():
    rng = np.random.default_rng(20)
    g = _genome(rng, 1500)
    lens = np.concatenate([rng.permutation(140) + 1, rng.integers(1, 141, size=160)])
    seqs = []
    for i, L in enumerate(lens.tolist()):
        a = int(rng.integers(0, len(g) - L + 1))
        seqs.append(rc(g[a:a + L]) if i % 2 else g[a:a + L])
    return tuple(seqs) + FIXED


@functools.lru_cache(maxsize=None)
def arrays_reads():
    rng = np.random.default_rng(21)
    g = _genome(rng, 3000)
    repeat = _genome(rng, 30)
    g = g[:1500] + "".join(repeat + _genome(rng, 32) for _ in range(8)) + repeat + g[1500:]
    seqs = []
    for i in range(1500):
        a = int(rng.integers(0, len(g) - 100 + 1))
        seqs.append(rc(g[a:a + 100]) if i % 2 else g[a:a + 100])
    return tuple(seqs) + ("T" * 120, "A" * 100 + "C")


@functools.lru_cache(maxsize=None)
def packed_input(name):
    """(packed, offsets) of 'mixed', 'arrays' or 'dense<k>', read-only."""
    if name.startswith("dense"):
        k = int(name[5:])
        codes = np.random.default_rng(300 + k).integers(0, 4, size=(DENSE[k], 150), dtype=np.uint8)
        packed, offs = _pack_codes(list(codes))
    else:
        packed, offs = _pack_seqs(mixed_reads() if name == "mixed" else arrays_reads())
    packed.setflags(write=False)
    offs.setflags(write=False)
    return packed, offs


# ---- the oracle's results, each computed once and left unchanged ---------------------------------
@functools.lru_cache(maxsize=None)
def ref_graph(name, k):
    packed, offs = packed_input(name)
    og = O.OGraph.build(packed, offs, k, threads=4)
    keys, mult = og.arrays()
    keys.setflags(write=False)
    mult.setflags(write=False)
    return og, keys, mult


@functools.lru_cache(maxsize=None)
def ref_counts(name, k):
    packed, offs = packed_input(name)
    return O.count_canonical(packed, offs, k, threads=4)


def _ref_nbrs(og, ids):
    """(out[n, 4], out counts, in[n, 4], in counts) of the ids, unused slots 0."""
    out = np.zeros((len(ids), 4), dtype=np.uint64)
    inn = np.zeros((len(ids), 4), dtype=np.uint64)
    oc = np.zeros(len(ids), dtype=np.int32)
    ic = np.zeros(len(ids), dtype=np.int32)
    for i, e in enumerate(ids.tolist()):
        o, p = og.outgoing(e), og.incoming(e)
        out[i, :len(o)], oc[i] = o, len(o)
        inn[i, :len(p)], ic[i] = p, len(p)
    return out, oc, inn, ic


@functools.lru_cache(maxsize=None)
def ref_all_nbrs(name, k):
    og, keys, _ = ref_graph(name, k)
    return _ref_nbrs(og, np.arange(keys.size, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def ref_cycles(k):
    """CycleFinder on `arrays` at threads = 1, on a copy of the graph (ref_graph's stays pristine):
    (result dict, valid bits afterwards, sorted cycle nodes)."""
    _, keys, mult = ref_graph("arrays", k)
    og = O.OGraph.from_arrays(keys, mult, k)
    res = og.cycle_finder(threads=1, **CF)
    nodes = sorted({x for _, cycles in res["entries"] for c in cycles for x in c})
    return res, og.valid(), np.array(nodes, dtype=np.uint64)


def _third_ids(D):
    """Every third edge id, phased so that the last edge (the top of the key space) is one."""
    return np.arange((D - 1) % 3, D, 3, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def ref_mapped(k, which):
    og, keys, _ = ref_graph("arrays", k)
    nodes = ref_cycles(k)[2] if which == "cycle" else _third_ids(keys.size)
    seqs = list(arrays_reads())
    return nodes, og.get_reads(seqs, len(seqs), nodes.tolist())


# ---- CPU part: the reference is right at every k, and the sweep reaches what it claims ------------
@pytest.mark.parametrize("k", KS)
def test_oracle_matches_bruteforce(k):
    seqs = list(mixed_reads())
    packed, offs = packed_input("mixed")
    if k == KS[0]:
        p0, o0 = pack_reads(seqs)
        assert np.array_equal(p0, packed) and np.array_equal(o0, offs)
    og, keys, mult = ref_graph("mixed", k)
    edges, bm = brute_graph(seqs, k)
    assert keys.tolist() == [boss_key(e, k) for e in edges]
    assert mult.tolist() == [bm[e] for e in edges]
    bout, binc = brute_neighbors(edges, k)
    out, oc, inn, ic = ref_all_nbrs("mixed", k)
    assert [out[i, :oc[i]].tolist() for i in range(len(edges))] == bout
    assert [inn[i, :ic[i]].tolist() for i in range(len(edges))] == binc
    canon = {}
    for e in edges:
        r = rc(e)
        canon[min(lsb_value(e), lsb_value(r))] = bm[e] // (2 if e == r else 1)
    ck, cc = ref_counts("mixed", k)
    assert ck.tolist() == sorted(canon)
    assert cc.tolist() == [canon[x] for x in sorted(canon)]


def test_sweep_covers_what_it_claims():
    # every minimizer length and both parities of E
    assert {minimizer_len(k) for k in KS} == set(range(3, 17))
    assert {minimizer_len(k) % 2 for k in KS} == {0, 1} and {(k + 1) % 2 for k in KS} == {0, 1}
    assert [k + 1 - minimizer_len(k) + 1 for k in (2, 30)] == [1, 16]  # the window's two ends
    # mixed: a read of exactly k and one of exactly k+1 bases; the complete graph at k = 2; labels
    # at both ends of the key space (A^k's group first, T^(k+1) the last edge); palindromes for even E
    lens = {len(s) for s in mixed_reads()}
    for k in KS:
        assert {k, k + 1} <= lens
        _, keys, mult = ref_graph("mixed", k)
        assert int(keys[0]) == 0 and int(keys[-1]) == 4 ** (k + 1) - 1, k
        if (k + 1) % 2 == 0:
            assert any(rc(s[:k + 1]) == s[:k + 1] for s in FIXED), k
    assert ref_graph("mixed", 2)[1].size == 64
    assert max(ref_graph("mixed", k)[1].size for k in KS) <= 3000
    # arrays: cycles and relevant reads at every k of its range, the poly-T read among set (b)'s
    for k in CF_KS:
        res, _, nodes = ref_cycles(k)
        D = ref_graph("arrays", k)[1].size
        assert len(res["entries"]) >= 1 and nodes.size >= 1, k
        assert len(ref_mapped(k, "cycle")[1]) >= 1, k
        assert any(max(r) >= D - 4 for r in ref_mapped(k, "third")[1]), k


@pytest.mark.parametrize("k", sorted(DENSE))
def test_dense_inputs_reach_the_msd_sort(k):
    _, keys, mult = ref_graph(f"dense{k}", k)
    assert keys.size >= 65536
    if k == 7:
        assert keys.size == 4 ** 8
        out, oc, inn, ic = ref_all_nbrs("dense7", 7)
        assert (oc == 4).all() and (ic == 4).all()


# ---- GPU part -----------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _default_minimizer_window(monkeypatch):
    monkeypatch.delenv("MCAAT_MINI_W", raising=False)  # the A/B override of sk_params' m


def _knobs(ctx, name):
    return ctx.knobs(**{n.replace(".", "__"): v for n, v in GRAPH_KNOBS[name].items()})


def _upload(ctx, name):
    import mcaat_amd as M

    return M.Reads.from_host(ctx, *packed_input(name))


def _gpu_nbrs(g, ids):
    def masked(a, c):
        return np.where(np.arange(4)[None, :] < c[:, None], a, np.uint64(0))

    out, oc = g.neighbors(ids, incoming=False)
    inn, ic = g.neighbors(ids, incoming=True)
    return masked(out, oc), oc, masked(inn, ic), ic


def _assert_graph(g, name, k, tag):
    _, okeys, omult = ref_graph(name, k)
    keys, mult, valid = g.download()
    assert np.array_equal(keys, okeys), tag
    assert np.array_equal(mult, omult), tag
    assert valid.all(), tag


def _assert_nbrs(got, want, tag):
    for a, b, what in zip(got, want, ("out", "out count", "in", "in count")):
        assert np.array_equal(a, b), (tag, what)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_count_every_k(gpu_ctx, k):
    import mcaat_amd as M

    reads = _upload(gpu_ctx, "mixed")
    gk, gc = M.count_edges(gpu_ctx, reads, k)
    ok, oc = ref_counts("mixed", k)
    assert np.array_equal(gk, ok)
    assert np.array_equal(gc, oc)
    reads.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k,knobset", GRAPH_CASES)
def test_graph_every_k(gpu_ctx, k, knobset):
    import mcaat_amd as M

    reads = _upload(gpu_ctx, "mixed")
    with _knobs(gpu_ctx, knobset):
        g = M.Graph.build(gpu_ctx, reads, k)
        _assert_graph(g, "mixed", k, (k, knobset))
        _assert_nbrs(_gpu_nbrs(g, np.arange(g.size, dtype=np.uint64)), ref_all_nbrs("mixed", k), (k, knobset))
        g.free()
    reads.free()


@pytest.mark.gpu
@pytest.mark.parametrize("knobset", ["default", "radix"])
@pytest.mark.parametrize("k", sorted(DENSE))
def test_dense_small_k(gpu_ctx, k, knobset):
    """The default build's MSD sort at D >= 65536 where its level-3 width is negative (k = 7, 8, 9) or
    barely positive (10, 11), and the radix sort on the same input. Neighbours: every edge at k = 7
    (the oracle side takes 0.2 s), a seeded sample of 3000 plus both ends of the id range otherwise."""
    import mcaat_amd as M

    name = f"dense{k}"
    og, okeys, _ = ref_graph(name, k)
    D = okeys.size
    assert D >= 65536 and (k != 7 or D == 4 ** 8)
    reads = _upload(gpu_ctx, name)
    with _knobs(gpu_ctx, knobset):
        g = M.Graph.build(gpu_ctx, reads, k)
        _assert_graph(g, name, k, (k, knobset))
        if k == 7:
            ids, want = np.arange(D, dtype=np.uint64), ref_all_nbrs(name, k)
        else:
            rng = np.random.default_rng(k)
            ids = np.unique(np.concatenate([rng.choice(D, size=3000, replace=False), np.arange(64),
                                            np.arange(D - 64, D)])).astype(np.uint64)
            want = _ref_nbrs(og, ids)
        _assert_nbrs(_gpu_nbrs(g, ids), want, (k, knobset))
        g.free()
    reads.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", CF_KS)
def test_cycle_finder_every_k(gpu_ctx, k):
    """CycleFinder on `arrays` at every k in 8..30 against the oracle at threads = 1. k = 2..7 are
    excluded: the graph is dense there and the oracle alone takes minutes (see CF_KS); in 8..30 it
    takes at most 0.5 s per k."""
    import mcaat_amd as M

    ores, ovalid, _ = ref_cycles(k)
    reads = _upload(gpu_ctx, "arrays")
    g = M.Graph.build(gpu_ctx, reads, k)
    _assert_graph(g, "arrays", k, k)
    res = g.cycle_finder(M.CfParams(**CF))
    assert res.stats[:6] == ores["stats"]
    assert res.candidates == ores["candidates"]
    assert res.buckets == ores["buckets"]
    assert len(res.entries) == len(ores["entries"])
    for (s, cyc), (os_, ocyc) in zip(res.entries, ores["entries"]):
        assert s == os_
        assert cyc == ocyc
    _, _, valid = g.download()
    assert np.array_equal(valid, ovalid)
    g.free()
    reads.free()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cycle", "third"])
@pytest.mark.parametrize("k", CF_KS)
def test_map_reads_every_k(gpu_ctx, k, which):
    """get_reads on `arrays`: the same reads, order and id chains as the oracle's restatement of
    reads.cpp. 'cycle': the cycle nodes of test_cycle_finder_every_k. 'third': every third edge id in
    batches of 300 ids; it splits multi-edge label groups (nodes that are not their group's last
    edge must not make a read relevant) and holds the last edge, so the poly-T read is relevant and
    every one of its labels resolves through the clamp at the top of the key space."""
    import mcaat_amd as M

    nodes, want = ref_mapped(k, which)
    D = ref_graph("arrays", k)[1].size
    assert len(want) >= 1
    if which == "third":
        assert any(max(r) >= D - 4 for r in want)
    reads = _upload(gpu_ctx, "arrays")
    g = M.Graph.build(gpu_ctx, reads, k)
    assert g.size == D
    mapped = g.map_reads(reads, nodes, max_batch_ids=300 if which == "third" else 0)
    got = [mapped.read(i) for i in range(len(mapped))]
    assert len(got) == len(want)
    assert got == want
    g.free()
    reads.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 15, 30])
def test_map_reads_length_boundary(gpu_ctx, k):
    """A read is mapped only if it is longer than 2k: of three copies of one sequence whose first
    k-mer is the only label in the node set, cut to 2k, 2k+1 and 2k+2 bases, the last two appear."""
    import mcaat_amd as M

    og, keys, _ = ref_graph("arrays", k)
    s = arrays_reads()[0][:2 * k + 2]
    node = og.index_binary_search([("ACGT".index(c) + 1) for c in s[:k]])
    assert 0 <= node < keys.size
    cuts = [s[:2 * k], s[:2 * k + 1], s]
    want = og.get_reads(cuts, len(cuts), [node])
    assert [len(w) for w in want] == [k + 2, k + 3] and want[0][0] == node
    reads = _upload(gpu_ctx, "arrays")
    g = M.Graph.build(gpu_ctx, reads, k)
    short = M.Reads.from_host(gpu_ctx, *_pack_seqs(cuts))
    mapped = g.map_reads(short, np.array([node], dtype=np.uint64))
    assert [mapped.read(i) for i in range(len(mapped))] == want
    assert mapped.records.tolist() == [1, 2]
    g.free()
    short.free()
    reads.free()
