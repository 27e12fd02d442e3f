"""The sharded (multi-rank) build and per-shard CycleFinder at every accepted k (2..30), with ranks
that hold no reads or no edges, and the sharded adjacency itself compared with the CPU oracle.

tests/test_k_sweep.py takes the one-GPU path through every k; the multi-rank path (csrc/dist.hip,
shard.hip, shard_cf.hip) ran at k = 23 and 27 only, on balanced synthetic slices, and every check of
it looked at the graph after mcaat_graph_unshard had rebuilt the adjacency with the one-GPU code.
Here each GPU case is one spawn of `world` ranks of tools/native_multi_check.py --input sharing the
GPU; each rank compares, against the oracle's results written by the parent and never against the
one-GPU path:
  * while still sharded, its own raw adjacency words (mcaat_graph_adjacency_words), decoded in numpy
    by the layout of csrc/common.h, with the oracle's out- and in-neighbours of its id range;
  * after the unshard: keys, multiplicities, all-valid bits, neighbors() of every id and the whole
    graph's decoded words;
  * with CycleFinder: a second sharded build, cycle_finder(comm=...), then valid bits, stats,
    candidates, buckets and entries bit for bit, and that all ranks hold the same results.
The parent asserts the shard layout from the ranks' reports: the (first, n_local) tile [0, D) in
rank order, every interior boundary is a group boundary (edges sharing key >> 4 stay on one rank:
what the sharded adjacency and the per-shard CycleFinder rest on), and the sizes meet the bound that
follows from the split rule.

The CPU part pins the split rule (csrc/splits.h through mcaat_shard_splits) to a restatement written
from its description, in exact integer arithmetic: histogram bits min(12, 2(k-1)), so every split
is a multiple of 16 at every k (the 12 bits used at every k before cut groups at k = 5 and 6 and
made the histogram shift negative at k <= 4), and bit-identical splits at k >= 7.

Inputs and cached oracle results come from tests/test_k_sweep.py (`mixed`, `arrays`).

Measured on an MI355X: see DESIGN.md, "Sharded k sweep".
"""
import bisect
import functools
import gzip
import itertools
import json
import re

import numpy as np
import pytest

import mcaat_amd as M
import oracle as O
from tests.test_k_sweep import (CF, CF_KS, KS, _pack_seqs, _ref_nbrs, arrays_reads, mixed_reads, ref_all_nbrs,
                                ref_cycles, ref_graph)
from tests.test_native_multi import _ranks

WORLDS = (1, 2, 3, 4, 8, 64)
CUT_WORLDS = (2, 3, 4, 8)
TIMEOUT = 120  # per spawn; a rank that reaches it counts as a hang


# ---- the split rule, restated from its description ------------------------------------------------
def hist_bits(k):
    """No histogram bin may resolve the low 4 key bits (a group is key >> 4) and 12 bits are enough."""
    return min(12, 2 * (k - 1))


def restated_splits(hist, world, key_bits, bits):
    """Split o (1 <= o < world) is the upper key edge of the first bin whose running sum reaches
    total * o / world; an all-zero histogram puts every split at the end of the key space. Exact
    integers: cum[b] >= total * o / world  <=>  cum[b] * world >= total * o."""
    assert len(hist) == 1 << bits
    cum = list(itertools.accumulate(int(x) for x in hist))
    total = cum[-1]
    out = []
    for o in range(1, world):
        b = len(hist)
        if total > 0:
            b = bisect.bisect_left(cum, -(-total * o // world)) + 1  # the first bin with cum >= ceil(total*o/world)
        out.append(b << (key_bits - bits))
    return out


def restated_old_splits(hist12, world, k):
    """The rule before: 12 histogram bits at every k (splits at multiples of 2^(2(k+1)-12))."""
    return restated_splits(hist12, world, 2 * (k + 1), 12)


def key_hist(keys, k, bits):
    return np.bincount((keys >> np.uint64(2 * (k + 1) - bits)).astype(np.int64), minlength=1 << bits).astype(np.uint64)


def histograms(k, bits):
    nb = 1 << bits
    rng = np.random.default_rng(1000 + k)
    first, last = np.zeros(nb, np.uint64), np.zeros(nb, np.uint64)
    first[0], last[-1] = 7, 9
    sparse = np.where(rng.random(nb) < 0.1, rng.integers(0, 1 << 20, size=nb), 0).astype(np.uint64)
    dense = rng.integers(0, 1 << 30, size=nb).astype(np.uint64)
    return {"zero": np.zeros(nb, np.uint64), "first": first, "last": last, "sparse": sparse, "dense": dense,
            "mixed": key_hist(ref_graph("mixed", k)[1], k, bits)}


def groups_cut(keys, splits):
    """How many splits fall inside a group of the sorted keys (edges sharing key >> 4)."""
    n = 0
    for s in splits:
        i = int(np.searchsorted(keys, np.uint64(s), side="left"))
        n += 0 < i < keys.size and int(keys[i - 1]) >> 4 == int(keys[i]) >> 4
    return n


def shard_sizes(keys, splits):
    cuts = [0] + [int(np.searchsorted(keys, np.uint64(s), side="left")) for s in splits] + [keys.size]
    return np.diff(cuts)


def size_bound_ok(sizes, D, world, maxbin):
    """Each prefix of owners ends at the first bin whose running sum reaches D*o/world, so it lies
    in [D*o/world, D*o/world + maxbin) and each size strictly within D/world +- maxbin."""
    return all(abs(int(s) * world - D) < maxbin * world for s in sizes)


@pytest.mark.parametrize("k", KS)
def test_shard_splits_equal_the_restated_rule(k):
    bits = hist_bits(k)
    assert M.shard_hist_bits(k) == bits
    for name, hist in histograms(k, bits).items():
        for world in WORLDS:
            got = M.shard_splits(k, world, hist).tolist()
            assert got == restated_splits(hist, world, 2 * (k + 1), bits), (k, name, world)
            assert got == sorted(got) and all(s % 16 == 0 and s <= 4 ** (k + 1) for s in got), (k, name, world)


@pytest.mark.parametrize("k", [k for k in KS if k >= 7])
def test_shard_splits_unchanged_from_k7(k):
    """At k >= 7 the splits are those of the rule before (always 12 bits), bit for bit."""
    assert hist_bits(k) == 12
    for name, hist in histograms(k, 12).items():
        for world in WORLDS:
            assert M.shard_splits(k, world, hist).tolist() == restated_old_splits(hist, world, k), (k, name, world)


def test_shard_splits_rejects_bad_arguments():
    """k outside 2..30 or world outside 1..64: MCAAT_E_INVALID (-1) from the C entry point itself,
    with and without a histogram; a histogram of the wrong size never reaches it (ValueError)."""
    import ctypes as C

    lib = M.load_library()
    hist = np.zeros(4096, np.uint64)
    splits = np.zeros(64, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    for k, world in ((1, 2), (31, 2), (23, 0), (23, 65), (-1, 2), (23, -1)):
        bits = C.c_int(-7)
        assert lib.mcaat_shard_splits(k, world, None, None, C.byref(bits)) == -1, (k, world)
        assert lib.mcaat_shard_splits(k, world, hist.ctypes.data_as(u64p), splits.ctypes.data_as(u64p), None) == -1
        with pytest.raises(M.McaatError) as e:
            M.shard_splits(k, world, hist)
        assert e.value.code == -1
    with pytest.raises(M.McaatError) as e:
        M.shard_hist_bits(31)
    assert e.value.code == -1
    for k, world in ((2, 1), (30, 64)):  # the ends of both ranges are accepted
        bits = C.c_int(-7)
        assert lib.mcaat_shard_splits(k, world, None, None, C.byref(bits)) == 0 and bits.value == hist_bits(k)
    with pytest.raises(ValueError):
        M.shard_splits(23, 2, np.zeros(1024, np.uint64))


def test_sharded_sweep_covers_what_it_claims():
    for k in KS:
        keys = ref_graph("mixed", k)[1]
        D, bits = keys.size, hist_bits(k)
        if k in (5, 6):  # the rule before (12 bits) cuts a group at every world of the sweep
            for world in CUT_WORLDS:
                old = restated_old_splits(key_hist(keys, k, 12), world, k)
                assert groups_cut(keys, old) >= 1, (k, world)
        hist = key_hist(keys, k, bits)
        for world in WORLDS:
            splits = M.shard_splits(k, world, hist).tolist()
            assert groups_cut(keys, splits) == 0, (k, world)
            assert size_bound_ok(shard_sizes(keys, splits), D, world, int(hist.max())), (k, world)
    k2 = ref_graph("mixed", 2)[1]
    assert (shard_sizes(k2, M.shard_splits(2, 8, key_hist(k2, 2, 2)).tolist()) == 0).any()
    # short reads: the first slice of `mixed` sorted by length holds reads, none of them an edge at k = 30
    assert 0 < sum(len(s) < 31 for s in mixed_reads()) < len(mixed_reads())


# ---- GPU part: one spawn of `world` ranks per case ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_ref():
    """One read "A"*100 at k = 23: D = 2 (A^24 and T^24)."""
    og = O.OGraph.build(*_pack_seqs(["A" * 100]), 23, threads=1)
    keys, mult = og.arrays()
    nbrs = _ref_nbrs(og, np.arange(keys.size, dtype=np.uint64))
    cf = O.OGraph.from_arrays(keys, mult, 23)
    res = cf.cycle_finder(threads=1, **CF)
    return keys, mult, nbrs, (res, cf.valid())


# CycleFinder's parameters for `mixed` at k = 2, the complete graph on 16 nodes (D = 64), over 8 ranks:
#   * every search runs into step_cap: at the default 10^7 the oracle alone takes 68 s and commits 60
#     entries without a cycle; at 2000 steps it takes 10 ms and commits cycles, so the case compares
#     cycle contents as well as the cap;
#   * the two region searches take cycle_max_length + 1 hops each, every hop one exchange among all
#     ranks: eight processes sharing one GPU spend 0.18 s a hop (measured: 29 s of 35 s at the default
#     77, like the existing eight-rank CycleFinder cases of test_native_multi.py at 49-54 s). Cycles
#     of 3..8 edges are what a 16-node graph has; 9 hops each way keep the case within seconds.
# The oracle gives 58 candidates and 128 cycles of 4..8 edges in 2 entries.
K2_CF = dict(CF, cycle_min_length=3, cycle_max_length=8, step_cap=2000)


@functools.lru_cache(maxsize=None)
def _mixed_k2_cycles():
    _, keys, mult = ref_graph("mixed", 2)
    og = O.OGraph.from_arrays(keys, mult, 2)
    return og.cycle_finder(threads=1, **K2_CF), og.valid()


def _pack(seqs):
    if not seqs:
        return np.zeros(0, np.uint64), np.zeros(1, np.uint64)
    return _pack_seqs(seqs)


def _slices(seqs, world):
    n = len(seqs)
    return [list(seqs[r * n // world:(r + 1) * n // world]) for r in range(world)]


def _write_input(path, deal, keys, mult, nbrs, cycles=None, cf_params=CF):
    d = {"keys": keys, "mult": mult, "out": nbrs[0], "out_n": nbrs[1], "in": nbrs[2], "in_n": nbrs[3]}
    for r, seqs in enumerate(deal):
        d[f"packed_{r}"], d[f"offsets_{r}"] = _pack(seqs)
    if cycles is not None:
        res, valid = cycles
        d["cf_params"] = np.frombuffer(json.dumps(cf_params).encode(), dtype=np.uint8)
        d["cf_valid"] = np.asarray(valid, dtype=np.uint8)
        d["cf_stats"] = np.asarray(res["stats"], dtype=np.uint64)
        d["cf_candidates"] = np.asarray(res["candidates"], dtype=np.uint64)
        d["cf_buckets"] = np.asarray(res["buckets"], dtype=np.int64)
        d["cf_entries"] = np.frombuffer(json.dumps([[int(s), [[int(x) for x in c] for c in cyc]]
                                                    for s, cyc in res["entries"]]).encode(), dtype=np.uint8)
    np.savez(path, **d)


def _run(tmp_path, k, world, deal, keys, mult, nbrs, cycles=None, cf_params=CF, knobs=(), sharded=True, fastx=None,
         adj_exchanges=0):
    """Spawn the ranks, require every comparison to pass, and assert the shard layout."""
    path = str(tmp_path / "input.npz")
    _write_input(path, deal, keys, mult, nbrs, cycles, cf_params)
    extra = ["--input", path, "--k", str(k)]
    for kn in knobs:
        extra += ["--knob", kn]
    if fastx:
        extra += ["--fastx", fastx]
    outs = _ranks(world, "shm", extra, timeout=TIMEOUT)
    for rc, o, e in outs:
        assert rc == 0, (o[-3000:], e[-3000:])
        assert "NATIVE_MULTI_OK" in o, o
    D = keys.size
    lay = []
    for _, o, _ in outs:
        m = re.search(r"sharded=(True|False) first=(\d+) n_local=(\d+) adj_exchanges=(\d+)", o)
        assert m and (m.group(1) == "True") == sharded, o
        lay.append((int(m.group(2)), int(m.group(3))))
        # the message adjacency runs two exchanges per chunk, every rank as many chunks as the
        # rank with the most edges needs (csrc/shard_cf.hip exchange_chunks); none by key ranges
        assert int(m.group(4)) == (adj_exchanges if sharded else 0), (o, adj_exchanges)
    if sharded:
        assert lay[0][0] == 0 and sum(n for _, n in lay) == D, lay
        for r in range(1, world):
            first = lay[r][0]
            assert first == lay[r - 1][0] + lay[r - 1][1], lay
            assert not (0 < first < D and int(keys[first - 1]) >> 4 == int(keys[first]) >> 4), (r, lay)
        maxbin = int(key_hist(keys, k, hist_bits(k)).max())
        assert size_bound_ok([n for _, n in lay], D, world, maxbin), (lay, D, maxbin)
    return outs, lay


def _mixed(tmp_path, k, world, **kw):
    _, keys, mult = ref_graph("mixed", k)
    return _run(tmp_path, k, world, _slices(mixed_reads(), world), keys, mult, ref_all_nbrs("mixed", k), **kw)


def _arrays(tmp_path, k, world, deal=None, **kw):
    _, keys, mult = ref_graph("arrays", k)
    res, valid, _ = ref_cycles(k)
    return _run(tmp_path, k, world, deal or _slices(arrays_reads(), world), keys, mult, ref_all_nbrs("arrays", k),
                cycles=(res, valid), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_every_k(tmp_path, k):
    _mixed(tmp_path, k, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("k", CF_KS)
def test_every_k_cycle_finder(tmp_path, k):
    _arrays(tmp_path, k, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 30])
def test_worlds(tmp_path, k, world):
    _mixed(tmp_path, k, world)


MESSAGES = ("dist.adj_ranges=0", "dist.win_ranges=0")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 4, 5, 6, 7, 11, 28, 29, 30])
def test_adjacency_by_messages(tmp_path, k):
    """Adjacency, filter windows and flags by request / response messages instead of target ranges."""
    _mixed(tmp_path, k, 3, knobs=MESSAGES, adj_exchanges=2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [11, 28, 29, 30])
def test_adjacency_by_messages_cycle_finder(tmp_path, k):
    _arrays(tmp_path, k, 3, knobs=MESSAGES, adj_exchanges=2)


@pytest.mark.gpu
def test_message_knobs(tmp_path):
    """The message adjacency with dist.adj_chunk=64 and the per-edge directory (dist.dir_edges=1) at
    k = 6. The chunk has a floor of 1024 edges (exchange_chunks), so 64 means 1024, and every rank
    holds fewer (D = 2714 over 3 ranks): one chunk, two exchanges, as without the knob. What this
    case adds to test_adjacency_by_messages[6] is the one-edge-per-prefix directory; more than one
    chunk is test_message_chunks."""
    _mixed(tmp_path, 6, 3, knobs=("dist.adj_chunk=64", "dist.adj_ranges=0", "dist.dir_edges=1"), adj_exchanges=2)


# The first 87 reads of `mixed` and 63 bases of the 88th: at k = 5 over 2 ranks the shards straddle
# the chunk floor of 1024 edges (D = 2033: 1025 and 1008), found by cutting the input on the CPU.
CHUNK_READS, CHUNK_CUT = 87, 63


@functools.lru_cache(maxsize=None)
def _chunk_ref():
    seqs = list(mixed_reads()[:CHUNK_READS]) + [mixed_reads()[CHUNK_READS][:CHUNK_CUT]]
    og = O.OGraph.build(*_pack_seqs(seqs), 5, threads=4)
    keys, mult = og.arrays()
    return seqs, keys, mult, _ref_nbrs(og, np.arange(keys.size, dtype=np.uint64))


def test_chunk_input_straddles_the_chunk_floor():
    _, keys, _, _ = _chunk_ref()
    sizes = shard_sizes(keys, M.shard_splits(5, 2, key_hist(keys, 5, hist_bits(5))).tolist()).tolist()
    assert sizes[1] <= 1024 < sizes[0] <= 2048, sizes


@pytest.mark.gpu
def test_message_chunks(tmp_path):
    """More than one chunk of the message adjacency at a small k (the chunk loop's offsets into the
    keys and the stores, and a rank taking part in an exchange with no edge of its own): k = 5,
    world 2, dist.adj_chunk=1024. Rank 0 holds 1025 edges, a chunk of 1024 and a chunk of 1; rank 1
    holds 1008, so its second chunk is empty. Four exchanges on both ranks, asserted."""
    seqs, keys, mult, nbrs = _chunk_ref()
    _, lay = _run(tmp_path, 5, 2, _slices(seqs, 2), keys, mult, nbrs, knobs=("dist.adj_chunk=1024",) + MESSAGES,
                  adj_exchanges=4)
    assert lay[1][1] <= 1024 < lay[0][1] <= 2048, lay


@pytest.mark.gpu
@pytest.mark.parametrize("knob,sharded", [("dist.shard_cf=0", False), ("dist.desc=0", False), ("dist.oriented=1", False),
                                          ("dist.preagg=1", True)])
@pytest.mark.parametrize("k", [2, 4, 5, 6, 30])
def test_routes(tmp_path, k, knob, sharded):
    """The build's other routes; the first three leave every rank the whole graph, so the
    sharded-words step is skipped and the gathered graph and its words are compared."""
    _mixed(tmp_path, k, 3, knobs=(knob,), sharded=sharded)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 6, 9])
def test_capped_grid(tmp_path, k):
    """Every grid-stride launch of the sharded adjacency capped to one block."""
    _mixed(tmp_path, k, 2, knobs=("dist.grid_blocks=1",))


@pytest.mark.gpu
@pytest.mark.parametrize("holder", [0, 2])
def test_all_reads_on_one_rank(tmp_path, holder):
    """Two of three ranks enter the build without a read (the n == 0 branches of the descriptor
    exchange), with CycleFinder."""
    deal = [list(arrays_reads()) if r == holder else [] for r in range(3)]
    _arrays(tmp_path, 23, 3, deal=deal)


@pytest.mark.gpu
def test_gz_input_goes_whole_to_part_zero(tmp_path):
    """The production form of ranks without reads: a .gz input goes whole to part 0, so ranks 1
    and 2 read (0, 0) and build with nothing."""
    seqs = arrays_reads()
    fq = "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(seqs)).encode()
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(gzip.compress(fq))
    outs, _ = _arrays(tmp_path, 23, 3, deal=[[], [], []], fastx=str(path))
    info = [re.search(r"reads_info=\((\d+), (\d+)\)", o).groups() for _, o, _ in outs]
    assert info[0] == (str(len(seqs)), str(sum(len(s) for s in seqs))), info
    assert info[1] == ("0", "0") and info[2] == ("0", "0"), info


@pytest.mark.gpu
def test_rank_with_only_short_reads(tmp_path):
    """`mixed` sorted by length at k = 30 over 4 ranks in contiguous slices: rank 0 takes exactly the
    reads shorter than k+1 (it has reads and not one edge), the others even slices of the rest."""
    seqs = sorted(mixed_reads(), key=len)
    n_short = sum(len(s) < 31 for s in seqs)
    assert 0 < n_short and all(len(s) < 31 for s in seqs[:n_short]) and len(seqs[n_short]) >= 31
    deal = [seqs[:n_short]] + _slices(seqs[n_short:], 3)
    _, keys, mult = ref_graph("mixed", 30)
    _run(tmp_path, 30, 4, deal, keys, mult, ref_all_nbrs("mixed", 30))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [3, 4])
def test_tiny_graph_two_edges(tmp_path, world):
    """D = 2 over 3 and 4 ranks: at least one rank owns no edge (the n == 0 branches of the target
    ranges, the sharded adjacency and the per-shard CycleFinder)."""
    keys, mult, nbrs, cycles = _tiny_ref()
    assert keys.size == 2
    _, lay = _run(tmp_path, 23, world, [["A" * 100]] + [[] for _ in range(world - 1)], keys, mult, nbrs, cycles=cycles)
    assert any(n == 0 for _, n in lay), lay


@pytest.mark.gpu
def test_tiny_graph_k2_world8(tmp_path):
    """The complete graph at k = 2 (D = 64, four histogram bins) over 8 ranks: empty shards, with
    CycleFinder (K2_CF)."""
    _, lay = _mixed(tmp_path, 2, 8, cycles=_mixed_k2_cycles(), cf_params=K2_CF)
    assert any(n == 0 for _, n in lay), lay
