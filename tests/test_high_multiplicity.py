"""Multiplicities at and above the 16-bit saturation point, on every build path.

An edge's multiplicity is occ(e) + occ(rc e) (twice occ for a palindrome): a 32-bit count that
becomes the graph's 16-bit `mult` clamped to 65535. The clamp is written out at several sites
(DESIGN.md §5 lists them with the test below that covers each); hot_reads(k) is a small read set
whose canonical counts sit at 65534, 65535, 65536, above 2^17, and, for palindromes, at a doubled
count on either side of 65535, so that a truncation instead of a clamp, a wrap of the doubled
count, a partial clamp in the wrong place or a dropped weight each change a result. The same
reads give fine partitions that hold ~10^5 copies of very few distinct descriptors, and single
LDS counters that take ~10^5 adds.

Bar: bit-exact against the CPU oracle; the oracle's own clamp is checked here against the
brute-force restatement of tests/helpers.py (the CPU test below)."""
import functools
import hashlib
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import mcaat_amd as M
import oracle as O
from tests.helpers import HipBuffer, boss_key, brute_graph, lsb_value, rc
from tests.test_strand_collapse import fragments, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (forward copies, reverse-complement copies) of the five boundary (k+1)-mers
BOUNDARY = ((40000, 25534), (65535, 0), (1, 65535), (50000, 50000), (140000, 0))
K_SHARD, THR_SHARD = 23, 20


def palindrome_copies(k):
    """Copies N of "AT"*75: with W = 151 - E windows per read the two alternating E-mers occur
    ceil(W/2) and floor(W/2) times per read, and N is the least that takes the doubled count of
    the first to 65535 or above."""
    W = 151 - (k + 1)
    return -(-65535 // (2 * ((W + 1) // 2)))


def hot_reads(k):
    """~510,000 reads (deterministic in k): the 2,000 background fragments; five boundary E-mers
    as reads of length E on both strands (BOUNDARY); one read of length E + 6 (seven edges at
    70000 each, in descriptors with n > 1); homopolymer, dinucleotide and palindromic runs."""
    E = k + 1
    rng = np.random.default_rng(k)

    def rand(n):
        while True:
            s = "".join(rng.choice(list("ACGT"), size=n))
            mers = [s[i:i + E] for i in range(n - E + 1)]
            if all(m != rc(m) for m in mers) and len(set(mers) | {rc(m) for m in mers}) == 2 * len(mers):
                return s

    seqs = list(fragments())
    for fwd, rev in BOUNDARY:
        e = rand(E)
        seqs += [e] * fwd + [rc(e)] * rev
    m = rand(E + 6)
    seqs += [m] * 40000 + [rc(m)] * 30000
    seqs += ["A" * 150] * 300 + ["T" * 150] * 220
    seqs += ["AC" * 75] * 300 + ["GT" * 75] * 230
    seqs += ["AT" * 75] * palindrome_copies(k)
    return [seqs[i] for i in rng.permutation(len(seqs))]


def _lsb_rc(a, E):
    """Reverse complement of LSB-first packed E-mers (numpy uint64)."""
    out = np.zeros_like(a)
    for i in range(E):
        out = (out << np.uint64(2)) | (np.uint64(3) - ((a >> np.uint64(2 * i)) & np.uint64(3)))
    return out


class _Fixture:
    """hot_reads(k) packed, with the oracle's counts, graph arrays and graph."""

    def __init__(self, k):
        self.k = k
        self.seqs = hot_reads(k)
        self.packed, self.offs = pack(self.seqs)
        self.ck, self.cc = O.count_canonical(self.packed, self.offs, k, threads=4)
        self.og = O.OGraph.build(self.packed, self.offs, k, threads=4)
        self.okeys, self.omult = self.og.arrays()

    def digest(self):
        return hashlib.sha256(self.okeys.tobytes() + self.omult.tobytes()).hexdigest()

    def check(self):
        """On the oracle's output alone: the fixture reaches the values it is built for."""
        k, cc, mult = self.k, self.cc, self.omult
        assert cc.dtype == np.uint32 and mult.dtype == np.uint16
        for v in (65534, 65535, 65536):
            assert (cc == v).any(), (k, v)
        assert (cc >= 1 << 17).any(), k
        assert (mult == 65534).any() and (mult == 65535).any(), k
        if k & 1:  # E even: "AT"*75 gives two palindromic edges, one doubled to >= 2^16, one below 65535
            pal = cc[self.ck == _lsb_rc(self.ck, k + 1)].astype(np.int64)
            assert (2 * pal >= 65536).any(), (k, pal)
            assert ((2 * pal < 65535) & (2 * pal > 60000)).any(), (k, pal)


@functools.lru_cache(maxsize=None)
def fixture(k):
    fx = _Fixture(k)
    fx.check()
    return fx


# ---- 1. CPU: the oracle's clamp against brute force ---------------------------------------
def test_oracle_saturation_matches_brute_force():
    """OGraph.build on hot_reads(23) has the keys and multiplicities of helpers.brute_graph
    (min(occ(e) + occ(rc e), 65535) in Python integers), and count_canonical the unsaturated
    32-bit counts of a plain dictionary count."""
    k = 23
    E = k + 1
    fx = fixture(k)
    edges, mult = brute_graph(fx.seqs, k)
    assert fx.og.size == len(edges)
    assert fx.okeys.tolist() == [boss_key(e, k) for e in edges]
    assert fx.omult.tolist() == [mult[e] for e in edges]
    assert max(mult.values()) == 65535 and 65534 in mult.values()

    occ = {}
    for s in fx.seqs:
        for i in range(len(s) - E + 1):
            e = s[i:i + E]
            occ[e] = occ.get(e, 0) + 1
    canon = {}
    for e, c in occ.items():
        key = min(lsb_value(e), lsb_value(rc(e)))
        canon[key] = canon.get(key, 0) + c
    want = sorted(canon.items())
    assert fx.ck.tolist() == [key for key, _ in want]
    assert fx.cc.tolist() == [c for _, c in want]
    assert max(canon.values()) == 140000


# ---- 2. node_counter: counts stay exact above 16 bits -------------------------------------
COUNT_KNOBS = (
    {},
    {"nc.desc_cap": 2, "nc.fine_bits": 9},         # raw path
    {"nc.edge_cap": 8, "nc.fallback_budget": 1},   # global fallback
    {"nc.big_table": 1},
    {"nc.group_budget": 1, "nc.out_cap": 1},
)


def _knobs(ctx, knobs):
    return ctx.knobs(**{n.replace(".", "__"): v for n, v in knobs.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("k", (23, 26, 27, 30))
def test_counts_exact_above_16_bits(gpu_ctx, k):
    fx = fixture(k)
    reads = M.Reads.from_host(gpu_ctx, fx.packed, fx.offs)
    try:
        for knobs in COUNT_KNOBS:
            gpu_ctx.reset_timing()
            with _knobs(gpu_ctx, knobs):
                gk, gc = M.count_edges(gpu_ctx, reads, k)
            assert gc.dtype == np.uint32
            assert np.array_equal(gk, fx.ck), (k, knobs)
            bad = np.flatnonzero(gc != fx.cc)
            assert bad.size == 0, (k, knobs, bad[:8], gc[bad[:8]], fx.cc[bad[:8]])
            if "nc.fallback_budget" in knobs:
                assert gpu_ctx.kernel_timing("lds_count_overflow_partitions")[1] > 0
    finally:
        reads.free()


# ---- 3. the graph's mult saturates exactly, on both sorts ---------------------------------
SORTS = {
    "msd": {"sort.msd": 1},
    "msd_mid": {"sort.msd": 1, "sort.wave_limit": 0},
    "msd_block": {"sort.msd": 1, "sort.wave_limit": 0, "sort.mid_limit": 0},
    "radix": {"sort.msd": 0},
    "default": {},
}


@pytest.mark.gpu
@pytest.mark.parametrize("k,sort", [(k, s) for k in (23, 27) for s in ("msd", "msd_mid", "msd_block", "radix")]
                         + [(26, "msd"), (29, "default"), (30, "default")])
def test_graph_mult_saturates(gpu_ctx, tmp_path, k, sort):
    fx = fixture(k)
    og = fx.og
    reads = M.Reads.from_host(gpu_ctx, fx.packed, fx.offs)
    with _knobs(gpu_ctx, SORTS[sort]):
        g = M.Graph.build(gpu_ctx, reads, k)
    reads.free()
    keys, mult, valid = g.download()
    assert g.size == og.size
    assert np.array_equal(keys, fx.okeys)
    bad = np.flatnonzero(mult != fx.omult)
    assert bad.size == 0, (k, sort, bad[:8], mult[bad[:8]], fx.omult[bad[:8]])
    assert valid.all()
    rng = np.random.default_rng(k)
    hot = np.flatnonzero(fx.omult >= 65534)
    ids = np.unique(np.concatenate([hot, rng.choice(g.size, size=1000, replace=False)])).astype(np.uint64)
    out, oc = g.neighbors(ids, incoming=False)
    inn, ic = g.neighbors(ids, incoming=True)
    for i, e in enumerate(ids):
        assert list(out[i, : oc[i]]) == og.outgoing(int(e))
        assert list(inn[i, : ic[i]]) == og.incoming(int(e))
    # the file format stores 16 bits
    path = str(tmp_path / "hot.sdbg")
    g.save(path)
    g.free()
    g2 = M.Graph.load(gpu_ctx, path)
    k2, m2, _ = g2.download()
    g2.free()
    assert np.array_equal(k2, fx.okeys) and np.array_equal(m2, fx.omult)


# ---- 4. the C-ABI building blocks ----------------------------------------------------------
@pytest.mark.gpu
def test_sharded_build_blocks_saturate(gpu_ctx):
    """tests/test_gpu_parity.py::test_sharded_build_blocks_two_owners_equal_one_gpu on the two
    interleaved halves of hot_reads(23), against the oracle's arrays: each half holds about half
    of every count, so 65536 is 32768 + 32768 (no partial saturates, the sum does) and 140000 is
    70000 + 70000 (each partial alone is above 16 bits)."""
    k = 23
    fx = fixture(k)
    parts = [M.Reads.from_host(gpu_ctx, *pack(fx.seqs[r::2])) for r in range(2)]
    counts = [M.Counts.count(gpu_ctx, r, k) for r in parts]
    bits = 10
    hist = sum(c.histogram(bits).astype(np.int64) for c in counts)
    cut = int(np.searchsorted(np.cumsum(hist), hist.sum() // 2))
    assert 0 < cut < (1 << bits)
    splits = np.array([cut << (2 * (k + 1) - bits)], dtype=np.uint64)
    sent = []
    for c in counts:
        cap = 2 * c.n + 1
        kd, cd = HipBuffer(np.zeros(cap, np.uint64)), HipBuffer(np.zeros(cap, np.uint32))
        sizes = c.partition(splits, kd.addr, cd.addr, cap).astype(np.int64)
        n = int(sizes.sum())
        sent.append((kd.to_numpy(np.uint64, n), cd.to_numpy(np.uint32, n), sizes))
    assert max(int(cc.max()) for _, cc, _ in sent) > 65535  # a partial above 16 bits is exchanged
    got_k, got_m = [], []
    for o in range(2):
        ks = np.concatenate([kk[sz[:o].sum():sz[:o + 1].sum()] for kk, _, sz in sent])
        cs = np.concatenate([cc[sz[:o].sum():sz[:o + 1].sum()] for _, cc, sz in sent])
        kb, cb = HipBuffer(ks), HipBuffer(cs)
        ko, mo = HipBuffer(np.zeros(max(1, ks.size), np.uint64)), HipBuffer(np.zeros(max(1, ks.size), np.uint16))
        n = M.edges_reduce(gpu_ctx, k, kb.addr, cb.addr, ks.size, ko.addr, mo.addr)
        got_k.append(ko.to_numpy(np.uint64, n))
        got_m.append(mo.to_numpy(np.uint16, n))
    keys, mult = np.concatenate(got_k), np.concatenate(got_m)
    assert np.array_equal(keys, fx.okeys)
    bad = np.flatnonzero(mult != fx.omult)
    assert bad.size == 0, (bad[:8], mult[bad[:8]], fx.omult[bad[:8]])
    kb, mb = HipBuffer(keys), HipBuffer(mult)
    g = M.Graph.from_sorted(gpu_ctx, k, kb.addr, mb.addr, keys.size)
    gk, gm, _ = g.download()
    g.free()
    assert np.array_equal(gk, fx.okeys) and np.array_equal(gm, fx.omult)
    for c in counts:
        c.free()
    for r in parts:
        r.free()


@pytest.mark.gpu
def test_edges_reduce_saturates_sums(gpu_ctx):
    """mcaat_edges_reduce on hand-made (key, count) pairs: the summands of one key arrive apart,
    among 300 other keys; mult = min(sum, 65535) in Python integers."""
    k = 23
    cases = ([65534], [65535], [65536], [32767, 32768], [40000, 40000], [1] * 3, [2 ** 31, 2 ** 31 - 1])
    base = 0x1234_5678_9ABC
    pairs = []
    for i, summands in enumerate(cases):
        pairs += [(base + 1000 * i, c) for c in summands]
    pairs += [(base + 3000 + 1 + j, 1 + j % 7) for j in range(300)]  # a run of distinct keys in between
    rng = np.random.default_rng(4)
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    want = {}
    for key, c in pairs:
        want[key] = want.get(key, 0) + c
    want_k = sorted(want)
    want_m = [min(want[key], 65535) for key in want_k]
    assert want_m.count(65535) == 5 and 65534 in want_m and 3 in want_m
    ks = np.array([p[0] for p in pairs], dtype=np.uint64)
    cs = np.array([p[1] for p in pairs], dtype=np.uint32)
    assert int(ks.max()) < 1 << (2 * (k + 1))
    kb, cb = HipBuffer(ks), HipBuffer(cs)
    ko, mo = HipBuffer(np.zeros(ks.size, np.uint64)), HipBuffer(np.zeros(ks.size, np.uint16))
    n = M.edges_reduce(gpu_ctx, k, kb.addr, cb.addr, ks.size, ko.addr, mo.addr)
    assert n == len(want_k)
    assert ko.to_numpy(np.uint64, n).tolist() == want_k
    assert mo.to_numpy(np.uint16, n).tolist() == want_m


# ---- 5. sharded builds over shared-memory ranks --------------------------------------------
_HOT_RANK = r"""
import hashlib, sys, numpy as np
sys.path.insert(0, {root!r})
import mcaat_amd as M
from tests.test_high_multiplicity import hot_reads, pack, K_SHARD, THR_SHARD
world, rank, name = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
ctx = M.Context(0)
for kv in sys.argv[4:]:
    kn, kval = kv.split("=")
    ctx.set_knob(kn, int(kval))
comm = M.Comm.shm(ctx, world, rank, name, 1 << 20)
packed, offs = pack(hot_reads(K_SHARD)[rank::world])
reads = M.Reads.from_host(ctx, packed, offs)
g = M.Graph.build_sharded(ctx, comm, reads, K_SHARD)
sharded = g.shard_info()[0]
stats = []
if sharded:
    stats = list(g.cycle_finder(M.CfParams(threshold_multiplicity=THR_SHARD), comm=comm).stats[:6])
g.unshard(comm)
keys, mult, _ = g.download()
h = hashlib.sha256(keys.tobytes() + mult.tobytes()).hexdigest()
g.free()
reads.free()
comm.barrier()
comm.close()
ctx.close()
print("HOT", rank, len(keys), h, int(sharded), *stats)
"""

ROUTES = [
    (2, ()),
    (2, ("dist.preagg=1",)),
    (2, ("dist.preagg=1", "nc.desc_cap=4")),
    (2, ("dist.oriented=1",)),
    (2, ("dist.desc=0",)),
    (2, ("dist.shard_cf=0",)),
    (3, ()),
    (3, ("dist.preagg=1",)),
    (1, ("dist.preagg=1", "dist.segs_at_one=1")),
]


@functools.lru_cache(maxsize=None)
def _oracle_stats():
    fx = fixture(K_SHARD)
    og = O.OGraph.from_arrays(fx.okeys, fx.omult, K_SHARD)
    return og.cycle_finder(threshold_multiplicity=THR_SHARD, threads=1)["stats"]


@pytest.mark.gpu
@pytest.mark.parametrize("world,knobs", ROUTES)
def test_sharded_build_saturates(world, knobs):
    """Rank r builds hot_reads(23)[r::world]: at two ranks the 65536-mer is 32768 + 32768 and the
    140000-mer 70000 + 70000. Every rank's gathered graph has the oracle's keys and multiplicities
    (sha256 over both), and where the route leaves the graph sharded the per-shard CycleFinder
    (threshold 20, mult up to 65535 in its filters) has the oracle's stats."""
    fx = fixture(K_SHARD)
    name = f"/mcaat_h_{uuid.uuid4().hex[:12]}"
    code = _HOT_RANK.format(root=ROOT)
    procs = [subprocess.Popen([sys.executable, "-c", code, str(world), str(r), name, *knobs], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=300)
            outs.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (code_, o, e) in enumerate(outs):
        assert code_ == 0, (o[-2000:], e[-3000:])
        f = [ln for ln in o.splitlines() if ln.startswith("HOT")][0].split()
        assert int(f[1]) == r
        assert (int(f[2]), f[3]) == (fx.og.size, fx.digest()), (world, knobs, r)
        sharded = bool(int(f[4]))
        # the count-exchange routes and dist.shard_cf=0 gather the graph on every rank (dist.hip)
        assert sharded == (not set(knobs) & {"dist.shard_cf=0", "dist.desc=0", "dist.oriented=1"}), (world, knobs)
        if sharded:
            assert [int(x) for x in f[5:11]] == _oracle_stats(), (world, knobs, r)
    assert _oracle_stats()[2] > 0


# ---- 6. CycleFinder thresholds at the top of the range -------------------------------------
THRESHOLDS = (65532, 65533, 65534, 65535, 65536, 2 ** 32 + 5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("c1_k23", "pe_err"))
def test_cycle_finder_thresholds_at_the_top(gpu_ctx, name):
    """Graphs whose multiplicities are 65533 + (mult % 3), the same array on both sides, through
    CycleFinder with thresholds around them and one above 32 bits: the `mult > threshold` filters
    see 65535 on one side and thresholds at and above it on the other."""
    from tests.test_gpu_parity import CONFIGS

    spec, k, prm = CONFIGS[name]
    packed, offs = M.synth_host(spec)
    keys, mult = O.OGraph.build(packed, offs, k, threads=4).arrays()
    top = (65533 + (mult.astype(np.uint32) % 3)).astype(np.uint16)
    assert set(np.unique(top).tolist()) == {65533, 65534, 65535}
    kb, mb = HipBuffer(keys), HipBuffer(top)
    n_cand = {}
    for thr in THRESHOLDS:
        og = O.OGraph.from_arrays(keys, top, k)
        ores = og.cycle_finder(threshold_multiplicity=thr, low_abundance=prm.low_abundance,
                               cycle_max_length=prm.cycle_max_length, cycle_min_length=prm.cycle_min_length, threads=1)
        n_cand[thr] = len(ores["candidates"])
        ovalid = og.valid()
        for compact in (0, 1):
            g = M.Graph.from_sorted(gpu_ctx, k, kb.addr, mb.addr, int(keys.size))
            gk, gm, _ = g.download()
            assert np.array_equal(gk, keys) and np.array_equal(gm, top)
            with gpu_ctx.knobs(cf__compact=compact):
                res = g.cycle_finder(M.CfParams(threshold_multiplicity=thr, low_abundance=prm.low_abundance,
                                                cycle_max_length=prm.cycle_max_length,
                                                cycle_min_length=prm.cycle_min_length))
            _, _, valid = g.download()
            g.free()
            tag = (name, thr, compact)
            assert res.stats[:6] == ores["stats"], tag
            assert res.candidates == ores["candidates"] and res.buckets == ores["buckets"], tag
            assert [(s, c) for s, c in res.entries] == [tuple(e) for e in ores["entries"]], tag
            assert np.array_equal(valid, ovalid), tag
    # both sides empty for a trivial reason would pass the comparisons above
    assert n_cand[65534] >= 1, n_cand
    assert n_cand[65535] == 0 and n_cand[65536] == 0 and n_cand[2 ** 32 + 5] == 0, n_cand
