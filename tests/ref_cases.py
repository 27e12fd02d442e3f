"""Inputs of the reference-parity tests (tests/test_reference_cycle_finder.py) and of the recorded
reference fixtures (tests/golden/make_ref_golden.py): read sets, hand-built graphs as arrays, a
model of libstdc++'s unordered_map iteration order, and the fixed serialisations that are hashed.
Pure Python / numpy; no product code, no oracle."""
import hashlib

import numpy as np

from tests.helpers import boss_key, pack_reads, rc

ACGT = "ACGT"


def rand_seq(rng, n):
    return "".join(ACGT[int(x)] for x in rng.integers(0, 4, size=n))


# ------------------------------------------------------------------------------ read sets
def planted_reads(seed, k, max_len, error_frac):
    """A repeat-spacer array in random flanks, read from both strands; `error_frac` of the reads
    carry one substitution. Repeat longer than k (so the array's cycles exist), spacer lengths
    chosen so that repeat + spacer falls on both sides of `max_len`. Returns the reads and the
    planted cycle lengths (repeat + spacer, one per spacer)."""
    rng = np.random.default_rng(seed)
    rep = rand_seq(rng, k + 2 + int(rng.integers(0, 5)))
    n_sp = int(rng.integers(4, 9))
    parts = [rand_seq(rng, 3000), rep]
    lengths = []
    for _ in range(n_sp):
        s_len = max(4, max_len - len(rep) + int(rng.integers(-8, 4)))
        parts += [rand_seq(rng, s_len), rep]
        lengths.append(len(rep) + s_len)
    parts.append(rand_seq(rng, 3000))
    genome = "".join(parts)
    read_len = 90
    reads = []
    for _ in range(30 * len(genome) // read_len):
        a = int(rng.integers(0, len(genome) - read_len + 1))
        r = genome[a:a + read_len]
        if rng.random() < error_frac:
            p = int(rng.integers(0, read_len))
            r = r[:p] + ACGT[(ACGT.index(r[p]) + int(rng.integers(1, 4))) % 4] + r[p + 1:]
        reads.append(rc(r) if rng.random() < 0.5 else r)
    return reads, lengths


def palindrome_reads():
    """The read set of test_gpu_parity.py::test_palindromes_and_homopolymers."""
    pal = "ACGTACGT"
    return [pal * 20, "A" * 60, "T" * 30 + pal + "GGCC" * 10]


def long_peel_reads(glen):
    """The read set of test_gpu_parity.py::test_long_peel_chains."""
    rng = np.random.default_rng(glen)
    genome = "".join(rng.choice(list(ACGT), size=glen))
    seqs = []
    for i in range(0, glen - 100 + 1):
        seqs += [genome[i:i + 100], rc(genome[i:i + 100])]
    return seqs


# ------------------------------------------------------------------------------ graphs from arrays
def graph_from_paths(k, paths, default_mult, mult_of=None):
    """Sorted BOSS keys and multiplicities of the (k+1)-mers of `paths` (one strand, as written).
    mult_of maps an edge string to its multiplicity; every other edge gets default_mult.
    Returns (keys, mult, index) with index[edge string] = edge id."""
    mult_of = mult_of or {}
    edges = sorted({p[i:i + k + 1] for p in paths for i in range(len(p) - k)}, key=lambda e: boss_key(e, k))
    assert all(e in edges for e in mult_of), "a multiplicity was given for an edge that is not in the graph"
    keys = np.array([boss_key(e, k) for e in edges], dtype=np.uint64)
    mult = np.array([mult_of.get(e, default_mult) for e in edges], dtype=np.uint16)
    assert mult.min() >= 1
    return keys, mult, {e: i for i, e in enumerate(edges)}


def distinct_ends(rng, lens):
    """Random strings of the given lengths (at most three) whose first symbols are C, G, T and
    whose last symbols are C, G, T in another order: with flanks that end / begin with A, the
    repeat's first edge then has every one of them as its own in-edge."""
    assert len(lens) <= 3
    first, last = "CGT", "TCG"
    return [first[i] + rand_seq(rng, n - 2) + last[i] if n >= 2 else first[i] for i, n in enumerate(lens)]


def array_path(rng, k, rep_len, spacer_lens, flank=40):
    """flank R S1 R S2 ... Sn R flank as one string, plus R and the spacers. With at most three
    spacers the only edge of the array with two or more in-edges is R[0:k+1] (the start node), and
    the cycle through spacer i has rep_len + len(Si) nodes."""
    rep = rand_seq(rng, rep_len)
    sp = distinct_ends(rng, spacer_lens) if len(spacer_lens) <= 3 else [rand_seq(rng, n) for n in spacer_lens]
    path = rand_seq(rng, flank) + "A" + rep
    for s in sp:
        path += s + rep
    path += "A" + rand_seq(rng, flank)
    return path, rep, sp


def multiplicity_boundary_graph():
    """Four arrays at k = 15 for `repeat_multiplicity / neighbor_multiplicity > 500`:
    A: start 1001, one spacer holding an edge of multiplicity 2 (1001 / 2 = 500: kept);
    B: start 1002, the same (501: cut);
    C: a saturated start 65535 with one spacer edge at 131 (500: kept) and one at 130 (504: cut).
    Every other edge has multiplicity 400. Returns (keys, mult, k, starts) with the start ids."""
    k = 15
    rng = np.random.default_rng(500)
    paths, mult_of, start_edges = [], {}, []
    for start_mult, lows in ((1001, [2]), (1002, [2]), (65535, [131, 130])):
        path, rep, sp = array_path(rng, k, 18, [24, 27, 30])
        paths.append(path)
        mult_of[rep[:k + 1]] = start_mult
        start_edges.append(rep[:k + 1])
        for s, low in zip(sp, lows):
            at = path.index(s) + 3  # an edge that lies wholly inside the spacer
            mult_of[path[at:at + k + 1]] = low
    keys, mult, index = graph_from_paths(k, paths, 400, mult_of)
    return keys, mult, k, [index[e] for e in start_edges]


# ------------------------------------------------------------------------------ libstdc++ order
_PRIMES = (13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753, 42043, 85229, 172933)


def unordered_map_order(keys):
    """Iteration order of a libstdc++ unordered_map<uint64_t, T> (identity hash, load factor 1)
    filled key by key. Within one bucket count it is the set model of
    tests/test_oracle.py::test_unordered_set_order_model_matches_libstdcxx: a new key goes before
    the first key of its bucket, or to the front when the bucket is empty. When the size would
    pass the bucket count, the table grows to the next prime of libstdc++'s list at or above twice
    the count, and the keys are put again, in their order of that moment, by the same rule."""
    order, level = [], 0

    def put(L, x, nb):
        pos = next((i for i, y in enumerate(L) if y % nb == x % nb), 0)
        L.insert(pos, x)

    for x in keys:
        if x in order:
            continue
        if len(order) + 1 > _PRIMES[level]:
            level += 1
            old, order = order, []
            for y in old:
                put(order, y, _PRIMES[level])
        put(order, x, _PRIMES[level])
    return order


# ------------------------------------------------------------------------------ digests
def sha_bytes(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def valid_digest(valid):
    """SHA-256 of the valid bits packed eight to a byte (bit i of byte j is edge 8j + i), and
    their popcount."""
    v = (np.asarray(valid) != 0)
    return sha_bytes(np.packbits(v, bitorder="little")), int(v.sum())


def entries_digest(entries):
    """SHA-256 of entries as little-endian uint64: start, cycle count, then per cycle its length
    and its nodes."""
    flat = []
    for s, cycles in entries:
        flat += [s, len(cycles)]
        for c in cycles:
            flat.append(len(c))
            flat += c
    return sha_bytes(np.array(flat, dtype="<u8"))


def packed_reads(seqs):
    return pack_reads(seqs)


# ------------------------------------------------------------------------------ step cap
def step_cap_graph(k, drop, seed=1):
    """A graph on which one FindCycle runs for millions of steps and finds its cycles last.

    Every (k+1)-mer is an edge (id == BOSS key), multiplicity 200. A circular string of 76 symbols
    with distinct k-mers gives a chain start -> c75 -> ... -> c1 -> start; c75 ends in T, so it is
    the start's largest out-edge and FindCycle tries it last. Every other in-edge of a chain edge
    is invalid from the beginning, so the rest of the graph cannot enter the chain, except one more
    in-edge of the start that has no in-edges of its own (the start needs two to be a candidate).
    `drop` of the remaining edges are invalid too, which sets how many steps the search through
    the start's other out-edges takes before the chain's turn comes. The start alone has a
    multiplicity above 60000. Returns (keys, mult, valid, start)."""
    rng = np.random.default_rng(seed)
    E = k + 1
    while True:
        circ = rand_seq(rng, 76)
        ext = circ + circ[:E]
        if len({ext[i:i + k] for i in range(76)}) == 76:
            break
    edges = [ext[i:i + E] for i in range(76)]
    r = next(i for i in range(76) if edges[(i + 1) % 76][-1] == "T")
    edges = edges[r:] + edges[:r]
    n = 4 ** E
    keys = np.arange(n, dtype=np.uint64)
    mult = np.full(n, 200, dtype=np.uint16)
    valid = np.ones(n, dtype=np.uint8)
    q = None
    for i, e in enumerate(edges):
        for x in ACGT:
            o = x + e[:k]
            if o == edges[i - 1]:
                continue
            if i == 0 and q is None:
                q = o
                for y in ACGT:
                    valid[boss_key(y + q[:k], k)] = 0
                continue
            valid[boss_key(o, k)] = 0
    if drop:
        keep = {boss_key(e, k) for e in edges} | {boss_key(q, k)}
        gone = np.flatnonzero(np.random.default_rng(seed + 1000).random(n) < drop)
        valid[[g for g in gone if int(g) not in keep]] = 0
    start = boss_key(edges[0], k)
    mult[start] = 65535
    return keys, mult, valid, int(start)
