"""The MSD edge sort and the adjacency at real level-3 bucket occupancies and key skew.

msd_sort (mcaat_amd/csrc/sdbg_build.hip) picks a kernel by the number of edges in a level-3 bucket
(the edges sharing the top 22 key bits: the last 11 symbols S of the source label): one wave up to
512, the 128-thread counting sort up to 1024, the 256-thread one up to 2048, the 1024-thread bitonic
block sort up to 16384, the radix sort for the whole graph above that; inside the counting kernels a
bucket with a bin above kMaxBin = 16 items, or with more bins than remaining key values, takes the
in-kernel bitonic network. The parity fixtures spread 1e5..4e6 edges over 2^22 buckets (0-2 items
each), so none of those decisions, the rank-within-bin loops, the multi-wave scan, or LinePlace's
more-than-one-line-per-round path of the scatters sees a realistic bucket there.

The read sets here are built edge by edge (an edge e = P.S.W as a read of exactly k+1 bases gives e
and rc(e)), so that chosen buckets hold chosen numbers of edges with chosen remainders:

  set A (k = 23, 28)  one bucket per size in SIZES (every stage limit, the limit + 1 and - 1), 600
                      edges each in the first (S = A^11) and the last (S = T^11) bucket, buckets of
                      300 / 700 / 1500 edges that share one bin, buckets of 200 / 700 / 1500 whose
                      largest bin holds exactly 16 and exactly 17, every eighth read of the 16384
                      bucket with one more leading base (a dense cluster of targets with sparse
                      predecessors: a run of k_adjacency_own that owns more than kOwnCap in_info
                      slots and still has words to write), read i repeated 1 + i mod 3 times, and
                      2,000 random 60-base reads so that D >= 65536 and the default build sorts by MSD
  set B               set A and one bucket of 16385: the fallback after level 3 has written
  set C (k = 12..17)  one complete bucket (every (P, W) of one S: 4^(k-10) edges, one item per bin,
                      lgb == rb; at k = 12 rb < lgb; at k = 17 exactly kBlockSort) and a few reads

The reference is numpy alone (np.unique over the BOSS keys of all edge windows and their reverse
complements, np.searchsorted for the neighbours), independent of the oracle and of
the library. The CPU test checks on the reference keys that every set has the occupancies it is
built for; the GPU tests hold keys, multiplicities, neighbours and the sort's stage counts
(kernel statistics msd3_*) against it, bit for bit.

Not reached here: a bucket listed because its padded size exceeds 640 items while it holds at most
512 real ones. That needs at least 19 level-2 chunks contributing to one bucket (more than 1.2 M
items in one level-1 bucket), and which chunk an item falls into follows the count output's order,
which a read set cannot steer; it stays with the full-size C5 run of test_scale_parity.py.
"""
import functools

import numpy as np
import pytest

import mcaat_amd as M
from tests.helpers import (boss_key, boss_keys, brute_graph, brute_neighbors, edge_codes, pack_code_groups, pack_reads,
                           rc, rc_codes)

# mirrored from mcaat_amd/csrc/sdbg_build.hip: kMB (bits per MSD level), kCh1, kCh2, kIL, the stage limits
# kWaveSort, kSmallMid, kMidSort, kBlockSort, the counting sorts' kMaxBin and their least bin
# counts (lg of 64 lanes, 128 and 256 threads), and the adjacency's kOwnB and kOwnCap
MB = 11
NB = 1 << (2 * MB)
CH1, CH2, IL = 32768, 65536, 8
WAVE_SORT, SMALL_MID, MID_SORT, BLOCK_SORT = 512, 1024, 2048, 16384
MAX_BIN = 16
LGB_MIN = (6, 7, 8)
OWN_B, OWN_CAP = 2048, 3072

SIZES = (1, 63, 64, 65, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 16384)
END_SIZE = 600
CLUSTERED = (300, 700, 1500)
EXACT = tuple((n, m) for n in (200, 700, 1500) for m in (MAX_BIN, MAX_BIN + 1))
OVERFLOW = BLOCK_SORT + 1


def _rb(k):
    """key bits below the level-3 bucket"""
    return 2 * (k + 1) - 2 * MB


def _distinct(rng, n, bits, keep=None):
    """n distinct uniform values below 2^bits (of those that `keep` accepts), in random order"""
    out = np.zeros(0, dtype=np.uint64)
    for _ in range(64):
        if out.size >= n:
            break
        x = rng.integers(0, 1 << bits, size=2 * (n - out.size) + 16, dtype=np.uint64)
        if keep is not None:
            x = x[keep(x)]
        out = np.unique(np.concatenate([out, x]))
    assert out.size >= n
    return rng.permutation(out)[:n]


def _lgb(n, lgb_min):
    lgb = lgb_min
    while (1 << lgb) < n:
        lgb += 1
    return lgb


def _exact_bin(rng, n, m, rb, free):
    """n distinct remainders (of those `free` accepts) whose largest bin holds exactly m: m of them
    in one bin, no other bin above 15. lgb >= 8 at these n, so the three kernels cut the same bins."""
    lgb = _lgb(n, LGB_MIN[0])
    assert lgb == _lgb(n, LGB_MIN[2]) and lgb <= rb
    w = np.uint64(rb - lgb)
    hot = np.uint64(rng.integers(0, 1 << lgb))
    while True:
        rest = _distinct(rng, n - m, rb, keep=lambda x: ((x >> w) != hot) & free(x))
        if np.bincount((rest >> w).astype(np.int64)).max() < MAX_BIN:
            break
    return np.concatenate([(hot << w) | _distinct(rng, m, rb - lgb, keep=lambda x: free((hot << w) | x)), rest])


def reference_graph(groups, k):
    """(ascending unique BOSS keys, multiplicities) of reads given as 2-D code arrays."""
    parts = []
    for g in groups:
        for i in range(g.shape[1] - k):
            w = g[:, i:i + k + 1]
            parts.append(boss_keys(w, k))
            parts.append(boss_keys(rc_codes(w), k))
    # a key is here occ(e) times as a window and occ(rc e) times as a reverse complement: a
    # palindrome twice per occurrence
    keys, cnt = np.unique(np.concatenate(parts), return_counts=True)
    return keys, np.minimum(cnt, 65535).astype(np.uint16)


def reference_neighbors(keys, k):
    """(out ids descending (D, 4), out degree, in ids ascending (D, 4), in degree); unused slots -1."""
    D = keys.size
    u = np.uint64
    W, R = keys & u(3), keys >> u(2)
    # out: the edges whose source label is e[1..k-1].W
    Rt = (W << u(2 * (k - 1))) | (R >> u(2))
    lo = np.searchsorted(keys, Rt << u(2), "left").astype(np.int64)
    hi = np.searchsorted(keys, (Rt + u(1)) << u(2), "left").astype(np.int64)
    oc = (hi - lo).astype(np.int32)
    j = np.arange(4, dtype=np.int64)
    out = np.where(j[None, :] < oc[:, None], hi[:, None] - 1 - j[None, :], -1)
    # in: the edges x.e[0..k-1], x ascending (their keys ascend with x)
    inn = np.full((D, 4), -1, dtype=np.int64)
    ic = np.zeros(D, dtype=np.int32)
    low = (R & u((1 << (2 * (k - 1))) - 1)) << u(2)
    last = R >> u(2 * (k - 1))
    rows = np.arange(D)
    for x in range(4):
        pk = ((low | u(x)) << u(2)) | last
        at = np.searchsorted(keys, pk, "left")
        hit = keys[np.minimum(at, D - 1)] == pk
        inn[rows[hit], ic[hit]] = at[hit]
        ic[hit] += 1
    return out, oc, inn, ic


class _Set:
    """A read set as code arrays, packed, with its numpy reference and what it is built to hold."""

    def __init__(self, name, k, groups, knobs, intended, exact=(), clustered=(), overflow=None):
        self.name, self.k, self.knobs = name, k, dict(knobs)
        self.intended, self.exact, self.clustered, self.overflow = dict(intended), tuple(exact), tuple(clustered), overflow
        self.raw_groups = list(groups)
        # read i of a group 1 + (i mod 3) times: multiplicities differ from key to key
        groups = [np.repeat(g, 1 + np.arange(g.shape[0]) % 3, axis=0) for g in groups]
        self.n_canonical_max = sum(g.shape[0] * (g.shape[1] - k) for g in groups)
        self.packed, self.offs = pack_code_groups(groups)
        self.keys, self.mult = reference_graph(groups, k)
        self.bucket = (self.keys >> np.uint64(_rb(k))).astype(np.int64)
        self.bids, self.bcnt = np.unique(self.bucket, return_counts=True)

    def size_of(self, bucket):
        at = np.searchsorted(self.bids, bucket)
        return int(self.bcnt[at]) if at < self.bids.size and self.bids[at] == bucket else 0

    def remainders(self, bucket):
        return self.keys[self.bucket == bucket] & np.uint64((1 << _rb(self.k)) - 1)

    @functools.cached_property
    def neighbors(self):
        return reference_neighbors(self.keys, self.k)


def _touches(codes, k, taken):
    """per read: does an edge window, or its reverse complement, fall into one of the buckets `taken`"""
    hit = np.zeros(codes.shape[0], dtype=bool)
    for i in range(codes.shape[1] - k):
        w = codes[:, i:i + k + 1]
        for keys in (boss_keys(w, k), boss_keys(rc_codes(w), k)):
            hit |= np.isin(keys >> np.uint64(_rb(k)), taken)
    return hit


def _filler(rng, n, length, k=0, taken=()):
    """n random reads that leave the buckets `taken` alone"""
    f = rng.integers(0, 4, size=(n + n // 4 + 8, length), dtype=np.uint8)
    if len(taken):
        f = f[~_touches(f, k, taken)]
    assert f.shape[0] >= n
    return f[:n]


class _Crafted:
    """Buckets filled with chosen remainders, as reads of k+1 bases. The buckets that get a chosen
    size are all named first: no reverse complement of a crafted edge is let into one of them."""

    def __init__(self, rng, k, taken):
        self.rng, self.k, self.rb = rng, k, _rb(k)
        self.taken = np.array(sorted(taken), dtype=np.uint64)
        self.groups, self.intended = [], {}

    def free(self, bucket):
        hi = np.uint64(bucket) << np.uint64(self.rb)
        return lambda x: ~np.isin(boss_keys(rc_codes(edge_codes(hi | x, self.k)), self.k) >> np.uint64(self.rb), self.taken)

    def add(self, bucket, rems, lead_every=0):
        k = self.k
        keys = (np.uint64(bucket) << np.uint64(self.rb)) | rems.astype(np.uint64)
        codes = edge_codes(keys, k)
        assert np.array_equal(boss_keys(codes, k), keys) and self.free(bucket)(rems).all()
        if lead_every:  # one more leading base: the edge gets a predecessor
            pick = np.arange(codes.shape[0]) % lead_every == 0
            lead = self.rng.integers(0, 4, size=(int(pick.sum()), 1), dtype=np.uint8)
            self.groups.append(np.concatenate([lead, codes[pick]], axis=1))
            codes = codes[~pick]
        self.groups.append(codes)
        self.intended[bucket] = rems.size


@functools.lru_cache(maxsize=None)
def set_a(k):
    rng = np.random.default_rng(9000 + k)
    rb = _rb(k)
    n_buckets = len(SIZES) + len(CLUSTERED) + len(EXACT)
    ids = [int(x) for x in _distinct(rng, n_buckets, 2 * MB, keep=lambda x: (x != 0) & (x != NB - 1))]
    c = _Crafted(rng, k, ids + [0, NB - 1])
    exact, clustered = [], []
    for n in SIZES:
        b = ids.pop()
        c.add(b, _distinct(rng, n, rb, keep=c.free(b)), lead_every=8 if n == BLOCK_SORT else 0)
    for b in (0, NB - 1):
        c.add(b, _distinct(rng, END_SIZE, rb, keep=c.free(b)))
    for n in CLUSTERED:  # the six symbols before S fixed: the top 12 bits of the remainder
        b = ids.pop()
        top = np.uint64(rng.integers(0, 1 << 12)) << np.uint64(rb - 12)
        clustered.append(b)
        c.add(b, top | _distinct(rng, n, rb - 12, keep=lambda x: c.free(b)(top | x)))
    for n, m in EXACT:
        b = ids.pop()
        exact.append((b, n, m))
        c.add(b, _exact_bin(rng, n, m, rb, c.free(b)))
    c.groups.append(_filler(rng, 2000, 60, k, c.taken))
    return _Set("A" + str(k), k, c.groups, {}, c.intended, exact, clustered)


@functools.lru_cache(maxsize=None)
def set_b(k):
    """set A itself and one bucket above the block sort, in a bucket that set A leaves empty"""
    a = set_a(k)
    rng = np.random.default_rng(9500 + k)
    (over,) = [int(x) for x in _distinct(rng, 1, 2 * MB, keep=lambda x: ~np.isin(x, a.bids))]
    c = _Crafted(rng, k, list(a.intended) + [over])
    c.add(over, _distinct(rng, OVERFLOW, _rb(k), keep=c.free(over)))
    return _Set("B" + str(k), k, a.raw_groups + c.groups, {}, {**a.intended, **c.intended}, a.exact, a.clustered, over)


@functools.lru_cache(maxsize=None)
def set_c(k):
    rng = np.random.default_rng(9700 + k)
    rb = _rb(k)
    (bucket,) = [int(x) for x in _distinct(rng, 1, 2 * MB)]
    keys = (np.uint64(bucket) << np.uint64(rb)) | rng.permutation(1 << rb).astype(np.uint64)
    groups = [edge_codes(keys, k), _filler(rng, 30, 40)]
    return _Set("C" + str(k), k, groups, {"sort.msd": 1}, {bucket: 1 << rb})


C_KS = (12, 13, 14, 15, 16, 17)
ALL_SETS = [(set_a, 23), (set_a, 28), (set_b, 23)] + [(set_c, k) for k in C_KS]


def _ids(params):
    return ["%s%d" % (f.__name__[-1].upper(), k) for f, k in params]


# ---- CPU: the vectorised helpers, the reference, and the occupancies the sets are built for ----
def test_vector_helpers_match_the_string_helpers():
    rng = np.random.default_rng(3)
    k = 9
    groups = [_filler(rng, 40, k + 1), _filler(rng, 25, k + 4), _filler(rng, 3, 70)]
    groups[0][:4] = groups[0][4:8]                       # repeated edges
    groups[0][8] = rc_codes(groups[0][9:10])[0]          # an edge and its reverse complement
    groups[0][10] = [0, 1, 2, 0, 1, 2, 3, 0, 1, 3]       # ACGACGTACT: not a palindrome
    groups[0][11] = [0, 1, 2, 3, 0, 3, 0, 1, 2, 3]       # ACGTATACGT: a palindrome (E even)
    groups[1][1] = groups[1][0]                          # a node with two out-edges
    groups[1][1, -1] ^= 1
    groups[1][2] = groups[1][0]                          # and one with two in-edges
    groups[1][2, 0] ^= 1
    seqs = ["".join("ACGT"[c] for c in row) for g in groups for row in g]
    assert rc(seqs[11]) == seqs[11]
    packed, offs = pack_code_groups(groups)
    p2, o2 = pack_reads(seqs)
    assert np.array_equal(packed, p2) and np.array_equal(offs, o2)
    assert boss_keys(groups[0], k).tolist() == [boss_key(s, k) for s in seqs[:40]]
    assert np.array_equal(edge_codes(boss_keys(groups[0], k), k), groups[0])
    assert ["".join("ACGT"[c] for c in row) for row in rc_codes(groups[0])] == [rc(s) for s in seqs[:40]]
    edges, mult = brute_graph(seqs, k)
    keys, m = reference_graph(groups, k)
    assert keys.tolist() == [boss_key(e, k) for e in edges]
    assert m.tolist() == [mult[e] for e in edges]
    out, inc = brute_neighbors(edges, k)
    ro, roc, ri, ric = reference_neighbors(keys, k)
    assert [r[:c].tolist() for r, c in zip(ro, roc)] == out
    assert [r[:c].tolist() for r, c in zip(ri, ric)] == inc
    assert max(roc) > 1 and max(ric) > 1


def test_reference_clamps_at_65535():
    k = 5
    e = np.array([[0, 1, 1, 2, 3, 0]], dtype=np.uint8)
    keys, m = reference_graph([np.repeat(e, 40000, axis=0), np.repeat(rc_codes(e), 30000, axis=0)], k)
    assert keys.size == 2 and m.tolist() == [65535, 65535]


def _owned_slots(keys, k):
    """k_own_bounds on the host: per run of OWN_B edges (moved to a group start) the in_info slots
    it owns, [O_W(r), O_W(r + 1)) for each W."""
    D = keys.size
    nruns = (D + OWN_B - 1) // OWN_B
    top = 1 << (2 * (k - 1))
    O = np.zeros((nruns + 1, 4), dtype=np.int64)
    for r in range(nruns + 1):
        s = r * OWN_B
        if r == nruns or s >= D:
            s = D
        elif s > 0:
            g0 = int(keys[s - 1]) >> 4
            while s < D and int(keys[s]) >> 4 == g0:
                s += 1
        for W in range(4):
            t = W * top if r == 0 else (W + 1) * top if s >= D else (W * top) | (int(keys[s]) >> 4)
            q = t << 2
            O[r, W] = D if q >> (2 * (k + 1)) else np.searchsorted(keys, np.uint64(q), "left")
    return O


@pytest.mark.parametrize("make,k", ALL_SETS, ids=_ids(ALL_SETS))
def test_fixture_occupancies(make, k):
    """Conditions on the reference keys alone; the stage counts asserted on the GPU rest on them."""
    fx = make(k)
    rb = _rb(k)
    assert np.all(fx.keys[1:] > fx.keys[:-1]) and int(fx.keys[-1]) >> (2 * (k + 1)) == 0
    assert fx.mult.min() >= 1 and len(set(fx.mult.tolist())) >= 3
    # every intended bucket size is present exactly
    for bucket, n in fx.intended.items():
        assert fx.size_of(bucket) == n, (bucket, n, fx.size_of(bucket))
    if fx.name[0] in "AB":
        assert sorted(fx.intended.values()) == sorted(
            SIZES + (END_SIZE, END_SIZE) + CLUSTERED + tuple(n for n, _ in EXACT) + ((OVERFLOW,) if fx.overflow else ()))
        assert fx.intended[0] == END_SIZE and fx.intended[NB - 1] == END_SIZE
        assert fx.keys.size >= 1 << 16  # the default build takes the MSD sort
        assert fx.keys.size <= 300_000
    # the largest bin under each kernel's rule: lgb = max(6 | 7 | 8, ceil lg n), the top lgb
    # bits of the rb-bit remainder
    def largest_bin(bucket, lgb_min):
        rem = fx.remainders(bucket)
        lgb = _lgb(rem.size, lgb_min)
        assert lgb <= rb
        return int(np.bincount((rem >> np.uint64(rb - lgb)).astype(np.int64)).max())

    for bucket, n, m in fx.exact:
        for lgb_min in LGB_MIN:
            assert largest_bin(bucket, lgb_min) == m, (bucket, n, m)
    for bucket in fx.clustered:
        for lgb_min in LGB_MIN:
            assert largest_bin(bucket, lgb_min) == fx.intended[bucket]
    if fx.name[0] in "AB":  # a uniform bucket stays far below the limit
        (b512,) = [b for b, n in fx.intended.items() if n == 512]
        assert largest_bin(b512, LGB_MIN[0]) < MAX_BIN
    if fx.name[0] == "C":  # complete: one item per bin when there are that many bins
        (bucket,) = fx.intended
        assert fx.intended[bucket] == 1 << rb
        for lgb_min in LGB_MIN:
            if _lgb(1 << rb, lgb_min) <= rb:
                assert _lgb(1 << rb, lgb_min) == rb and largest_bin(bucket, lgb_min) == 1
        assert _lgb(1 << _rb(12), LGB_MIN[0]) > _rb(12) and (1 << _rb(17)) == BLOCK_SORT
    # every level-1 bucket fits one level-2 chunk, line padding of its level-1 chunk runs
    # included: a level-3 bucket is then one chunk's run, its padded size is round8(n), and the
    # stage that sorts it follows from n alone
    l1 = np.bincount(fx.bucket >> MB, minlength=1 << MB)
    n_ch1 = -(-fx.n_canonical_max // CH1)
    assert int(l1.max()) + (IL - 1) * n_ch1 < CH2
    # no bucket above the block sort but set B's
    over = fx.bids[fx.bcnt > BLOCK_SORT].tolist()
    assert over == ([fx.overflow] if fx.overflow is not None else [])
    if fx.name[0] in "AB":
        # the dense cluster of targets: some run of k_adjacency_own owns more than the staged
        # cap and has in_info words to write among its slots
        O = _owned_slots(fx.keys, k)
        tot = (O[1:] - O[:-1]).sum(axis=1)
        assert tot.sum() == fx.keys.size and tot.min() >= 0
        r = int(tot.argmax())
        assert tot[r] > OWN_CAP, tot[r]
        ic = fx.neighbors[3]
        assert sum(int((ic[O[r, W]:O[r + 1, W]] > 0).sum()) for W in range(4)) >= 1000


# ---- GPU ----------------------------------------------------------------------------------------
def _build(ctx, fx, knobs):
    reads = M.Reads.from_host(ctx, fx.packed, fx.offs)
    try:
        ctx.reset_timing()
        with ctx.knobs(**{n.replace(".", "__"): v for n, v in {**fx.knobs, **knobs}.items()}):
            return M.Graph.build(ctx, reads, fx.k)
    finally:
        reads.free()


def _where(fx, i):
    """bucket and occupancy of reference edge i, for a failure message"""
    b = int(fx.bucket[min(i, fx.bucket.size - 1)])
    return "edge %d: bucket %d holding %d" % (i, b, fx.size_of(b))


def _assert_keys_and_mult(fx, g, knobs):
    keys, mult, valid = g.download()
    assert keys.size == fx.keys.size, (fx.name, knobs, keys.size, fx.keys.size)
    bad = np.flatnonzero(keys != fx.keys)
    assert bad.size == 0, (fx.name, knobs, bad.size, _where(fx, int(bad[0])), hex(int(keys[bad[0]])), hex(int(fx.keys[bad[0]])))
    bad = np.flatnonzero(mult != fx.mult)
    assert bad.size == 0, (fx.name, knobs, bad.size, _where(fx, int(bad[0])), int(mult[bad[0]]), int(fx.mult[bad[0]]))
    assert valid.all()


A_KNOBS = (
    {},
    {"sort.small_mid": 0},
    {"sort.small_mid": 1},
    {"sort.l3_counting": 0},
    {"sort.wave_limit": 0},   # the 128- and 256-thread kernels see the buckets of <= 512 too
    {"sort.mid_limit": 0},
    {"sort.msd": 0},          # the radix baseline
)
C_KNOBS = ({}, {"sort.wave_limit": 0}, {"sort.small_mid": 0}, {"sort.small_mid": 1})
KEY_CASES = ([(set_a, 23, kn) for kn in A_KNOBS] + [(set_a, 28, kn) for kn in A_KNOBS[:2]]
             + [(set_b, 23, {}), (set_b, 23, {"sort.block_limit": 4096})]
             + [(set_c, k, kn) for k in C_KS for kn in C_KNOBS])


def _case_id(c):
    make, k, kn = c
    return "%s%d-%s" % (make.__name__[-1].upper(), k, ",".join("%s=%d" % (n.split(".")[1], v) for n, v in kn.items()) or "default")


@pytest.mark.gpu
@pytest.mark.parametrize("make,k,knobs", KEY_CASES, ids=[_case_id(c) for c in KEY_CASES])
def test_keys_and_multiplicities(gpu_ctx, make, k, knobs):
    fx = make(k)
    g = _build(gpu_ctx, fx, knobs)
    try:
        _assert_keys_and_mult(fx, g, knobs)
    finally:
        g.free()


ADJ_KNOBS = ({"sdbg.adj_lds": 0}, {}, {"sdbg.adj_cap": 0}, {"sdbg.adj_cap": 700})


@pytest.mark.gpu
def test_neighbors_with_a_dense_target_cluster(gpu_ctx):
    """Every edge's out- and in-neighbours on set A (k = 23) equal the numpy reference's, under the
    per-edge global search, the default (whose run over the 16384 bucket's predecessors is unstaged
    by its own size), every run unstaged, and a cap of 700."""
    fx = set_a(23)
    ro, roc, ri, ric = fx.neighbors
    ids = np.arange(fx.keys.size, dtype=np.uint64)
    col = np.arange(4)[None, :]
    first = None
    for knobs in ADJ_KNOBS:
        g = _build(gpu_ctx, fx, knobs)
        try:
            out, oc = g.neighbors(ids, incoming=False)
            inn, ic = g.neighbors(ids, incoming=True)
        finally:
            g.free()
        for what, got, cnt, want, wcnt in (("out", out, oc, ro, roc), ("in", inn, ic, ri, ric)):
            bad = np.flatnonzero(cnt != wcnt)
            assert bad.size == 0, (knobs, what, bad.size, _where(fx, int(bad[0])), int(cnt[bad[0]]), int(wcnt[bad[0]]))
            bad = np.flatnonzero(((got.astype(np.int64) != want) & (col < wcnt[:, None])).any(axis=1))
            assert bad.size == 0, (knobs, what, bad.size, _where(fx, int(bad[0])), got[bad[0]].tolist(), want[bad[0]].tolist())
        mask = col < roc[:, None], col < ric[:, None]
        got = (np.where(mask[0], out, 0), oc, np.where(mask[1], inn, 0), ic)
        if first is None:
            first = got
        else:
            assert all(np.array_equal(a, b) for a, b in zip(first, got)), knobs


STAGE_SETS = ALL_SETS


@pytest.mark.gpu
@pytest.mark.parametrize("make,k", STAGE_SETS, ids=_ids(STAGE_SETS))
def test_stage_counts(gpu_ctx, make, k):
    """The level-3 stages' forward counts (kernel statistics msd3_*) equal the reference's bucket
    histogram: by test_fixture_occupancies a bucket's stage follows from its size alone. At these
    D the small stage runs by default (D / 2^22 <= 768)."""
    fx = make(k)
    g = _build(gpu_ctx, fx, {})
    try:
        got = {n: gpu_ctx.kernel_timing("msd3_" + n)[1] for n in ("listed", "small_fwd", "mid_fwd", "radix_fallback")}
        _assert_keys_and_mult(fx, g, {})
    finally:
        g.free()
    want = {"listed": int((fx.bcnt > WAVE_SORT).sum()), "small_fwd": int((fx.bcnt > SMALL_MID).sum()),
            "mid_fwd": int((fx.bcnt > MID_SORT).sum()), "radix_fallback": int(fx.overflow is not None)}
    assert got == want, (fx.name, got, want)
    if fx.name[0] in "AB":  # the sizes on either side of each limit are in the set
        assert want["listed"] >= 9 and want["small_fwd"] >= 6 and want["mid_fwd"] >= 3
