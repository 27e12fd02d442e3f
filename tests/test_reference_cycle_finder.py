"""CycleFinder pinned to the reference program.

CPU (build machine, where `make -C oracle ref` has compiled the reference's own cycle_finder.cpp
behind the stand-in SDBG of oracle/ref/): the oracle's restatement against a live run of the
reference at threads = 1 on a seeded sweep and on hand-built graphs at the places a restatement
slips (the integer division of _BackgroundCheck, the length bounds, visited, the cluster bound of
500, set and map iteration orders), and the committed fixtures tests/golden/ref_*.json against a
fresh run.

GPU: the HIP path against those recorded results (the fixtures only: neither the reference nor
oracle/_ref/ is read), with the default cluster bound and step cap.

Pinned: CycleFinder given a graph. Not pinned: the SDBG conventions (MEGAHIT is absent),
multi-threaded order, and the step cap's exact value inside the bracket (9.86 M, 13.47 M) steps
that test_step_cap_of_the_reference sets."""
import json
import os

import numpy as np
import pytest

import oracle as O
from tests import ref_cases as RC
from tests.golden import make_ref_golden as G
from tests.helpers import boss_key, brute_graph, brute_neighbors, pack_reads


def _require_reference():
    """Skip only where neither the runner nor the reference tree exists; a tree without the
    runner is a build that was not made."""
    if O.ref_available():
        return
    if O.ref_tree_present():
        pytest.fail(f"oracle/_ref/ref_cf is missing although the reference tree is here: run `{O.REF_BUILD_COMMAND}`")
    pytest.skip("neither oracle/_ref/ref_cf nor the reference tree is on this machine")


def _both(keys, mult, k, valid=None, **params):
    """Run the reference and the oracle on the same arrays and assert everything equal: entries
    in map order, candidates, buckets, the six stats, the valid bytes afterwards. Returns the
    reference's result."""
    ref = O.ref_cycle_finder(keys, mult, k, valid=valid, **params)
    og = O.OGraph.from_arrays(keys, mult, k)
    if valid is not None:
        og.set_valid(valid)
    ores = og.cycle_finder(threads=1, **params)
    assert ores["stats"] == ref["stats"]
    assert ores["candidates"] == ref["candidates"]
    assert ores["buckets"] == ref["buckets"]
    in_map_order = [ores["entries"][i] for i in ores["map_order"]]
    assert [s for s, _ in in_map_order] == [s for s, _ in ref["entries"]]
    for (s, cyc), (_, rcyc) in zip(in_map_order, ref["entries"]):
        assert cyc == rcyc, f"cycles of start {s} differ"
    assert np.array_equal(og.valid(), ref["valid"])
    # the model the GPU tests use to put commit order into map order
    assert RC.unordered_map_order([s for s, _ in ores["entries"]]) == [s for s, _ in ref["entries"]]
    return ref


# ------------------------------------------------------------------ the stand-in SDBG
@pytest.mark.parametrize("k,seed,cleared", [(4, 1, 0.0), (5, 2, 0.0), (7, 3, 0.0), (5, 4, 0.3)])
def test_standin_sdbg_neighbours_equal_brute_force(k, seed, cleared):
    """The SDBG the reference runs on (oracle/ref/sdbg/sdbg.h) against helpers.brute_neighbors:
    valid out-edges descending, valid in-edges ascending, for every edge, valid or not."""
    _require_reference()
    rng = np.random.default_rng(seed)
    seqs = [RC.rand_seq(rng, int(rng.integers(k + 1, 60))) for _ in range(40)]
    edges, mult = brute_graph(seqs, k)
    keys = np.array([boss_key(e, k) for e in edges], dtype=np.uint64)
    m = np.array([mult[e] for e in edges], dtype=np.uint16)
    valid = (rng.random(len(edges)) >= cleared).astype(np.uint8)
    out, inc = brute_neighbors(edges, k)
    got_out, got_in = O.ref_neighbors(keys, m, k, valid=valid)
    assert cleared == 0.0 or 0 < valid.sum() < valid.size
    assert got_out == [[x for x in o if valid[x]] for o in out]
    assert got_in == [[x for x in i if valid[x]] for i in inc]


# ------------------------------------------------------------------ seeded sweep
_KS = (9, 15, 21, 23, 26, 27, 30)
_THR = (1, 2, 5, 20)
_MM = ((27, 77), (20, 70), (1, 20), (5, 40))


def _sweep_cases():
    cases = []
    for i in range(42):
        k = _KS[i % 7]
        cases.append((i, k, bool((i // 7) % 2), _THR[(i // 2) % 4], _MM[(i // 3) % 4], 0.0))
    # short cycles exist only at small k: both short (min, max) pairs at k = 9, both modes
    for j, (la, mm) in enumerate([(True, (1, 20)), (False, (1, 20)), (True, (5, 40)), (False, (5, 40))]):
        cases.append((100 + j, 9, la, _THR[j], mm, 0.0))
    # initial valid masks with 2 % and 30 % of the edges cleared
    cases.append((200, 23, True, 5, (27, 77), 0.02))
    cases.append((201, 21, False, 2, (20, 70), 0.30))
    return cases


def test_sweep_covers_what_it_should():
    cs = _sweep_cases()
    assert len(cs) >= 42
    assert {c[1] for c in cs} == set(_KS) and {c[2] for c in cs} == {True, False}
    assert {c[3] for c in cs} == set(_THR) and {c[4] for c in cs} == set(_MM)


def _cycles_expected(lengths, mm, cleared):
    """The planted array must give cycles: all edges valid at the start, and a spacer whose cycle
    is longer than min and shorter than max (DepthLevelSearch needs one below max)."""
    return not cleared and any(mm[0] < n < mm[1] for n in lengths)


@pytest.mark.parametrize("seed,k,low_abundance,thr,mm,cleared", _sweep_cases())
def test_oracle_equals_reference_on_seeded_graphs(seed, k, low_abundance, thr, mm, cleared):
    _require_reference()
    rng = np.random.default_rng(seed)
    seqs, lengths = RC.planted_reads(seed, k, mm[1], error_frac=float(rng.uniform(0.0, 0.3)))
    packed, offs = pack_reads(seqs)
    keys, mult = O.OGraph.build(packed, offs, k, threads=4).arrays()
    assert 10_000 < keys.size < 40_000
    valid = None
    if cleared:
        valid = (rng.random(keys.size) >= cleared).astype(np.uint8)
    ref = _both(keys, mult, k, valid=valid, threshold_multiplicity=thr, low_abundance=low_abundance,
                cycle_min_length=mm[0], cycle_max_length=mm[1])
    if _cycles_expected(lengths, mm, cleared):
        assert ref["stats"][5] > 0, "the planted array gave no cycle to compare"


def test_sweep_is_not_vacuous():
    """Most graphs of the sweep have a planted cycle inside the length bounds (each such case
    asserts that the reference found cycles), for every (min, max) pair and both modes."""
    expected = [(c, _cycles_expected(RC.planted_reads(c[0], c[1], c[4][1], 0.0)[1], c[4], c[5]))
                for c in _sweep_cases()]
    with_cycles = [c for c, e in expected if e]
    assert len(with_cycles) >= 30, len(with_cycles)
    assert {c[4] for c in with_cycles} == set(_MM) and {c[2] for c in with_cycles} == {True, False}


# ------------------------------------------------------------------ hand-built graphs
def test_background_check_division_boundary():
    """1001 / 2 = 500 keeps the spacer, 1002 / 2 = 501 cuts it; a saturated 65535 keeps 131 (500)
    and cuts 130 (504): 3 + 2 + 2 cycles."""
    _require_reference()
    keys, mult, k, starts = RC.multiplicity_boundary_graph()
    ref = _both(keys, mult, k)
    assert ref["candidates"] == sorted(starts, key=lambda s: (-int(np.ceil(np.log2(float(mult[s])))), s))
    got = {s: len(c) for s, c in ref["entries"]}
    assert [got[s] for s in starts] == [3, 2, 2]


def test_self_loop_start_is_no_candidate():
    """An edge that is its own in-edge (A^(k+1)) with a second in-edge and a multiplicity above the
    threshold passes every other test of ChunkStartNodes, DepthLevelSearch included, and is left
    out by _IncomingNotEqualToCurrentNode alone."""
    _require_reference()
    k = 15
    rng = np.random.default_rng(77)
    path, _, _ = RC.array_path(rng, k, 18, [24, 27, 30])
    loop = RC.rand_seq(rng, 30) + "C" + "A" * (k + 4) + "G" + RC.rand_seq(rng, 30)
    keys, mult, index = RC.graph_from_paths(k, [path, loop], 400)
    e = index["A" * (k + 1)]
    og = O.OGraph.from_arrays(keys, mult, k)
    assert e in og.incoming(e) and len(og.incoming(e)) == 2 and og.dls(e)
    ref = _both(keys, mult, k)
    assert e not in ref["candidates"] and len(ref["candidates"]) == 1 and ref["stats"][5] == 3


def test_cycle_min_length_boundary():
    """The start's only cycles have path.size() == cycle_min_length and cycle_min_length + 1:
    `path.size() > cycle_min_length` records the second alone."""
    _require_reference()
    k = 15
    path, rep, _ = RC.array_path(np.random.default_rng(27), k, 18, [9, 10])
    keys, mult, index = RC.graph_from_paths(k, [path], 400)
    ref = _both(keys, mult, k)
    assert ref["candidates"] == [index[rep[:k + 1]]]
    assert [len(c) for _, cyc in ref["entries"] for c in cyc] == [28]


def test_cycle_max_length_boundary():
    """Cycles of cycle_max_length - 1, cycle_max_length and cycle_max_length + 1 nodes from one
    start: the path grows to cycle_max_length nodes and no further, so 76 and 77 are recorded.
    Two more starts have one cycle each, of 76 and of 77 nodes: DepthLevelSearch gives up at depth
    cycle_max_length before it looks for the target, so the first is a candidate and the second,
    whose cycle FindCycle would record, is not."""
    _require_reference()
    k = 15
    rng = np.random.default_rng(78)
    paths, starts = [], []
    for lens in ([58, 59, 60], [58], [59]):
        path, rep, _ = RC.array_path(rng, k, 18, lens)
        paths.append(path)
        starts.append(rep[:k + 1])
    keys, mult, index = RC.graph_from_paths(k, paths, 400)
    ref = _both(keys, mult, k)
    got = {s: sorted(len(c) for c in cyc) for s, cyc in ref["entries"]}
    assert got.get(index[starts[0]]) == [76, 77]
    assert got.get(index[starts[1]]) == [76]
    assert index[starts[2]] not in ref["candidates"] and index[starts[2]] not in got


def test_second_start_is_skipped_by_visited():
    """Six spacers: some share their last symbol, so an edge that merges them into the repeat has
    two in-edges and is a candidate too. It lies on cycles of the repeat's first edge, which is
    searched first (higher bucket) and marks it visited: it gets no entry."""
    _require_reference()
    k = 15
    rng = np.random.default_rng(6)
    path, rep, _ = RC.array_path(rng, k, 18, [22, 24, 26, 28, 30, 32])
    keys, mult, index = RC.graph_from_paths(k, [path], 50, {rep[:k + 1]: 300})
    ref = _both(keys, mult, k)
    assert len(ref["candidates"]) >= 2 and ref["candidates"][0] == index[rep[:k + 1]]
    assert [(s, len(c)) for s, c in ref["entries"]] == [(index[rep[:k + 1]], 6)]


@pytest.mark.parametrize("n", [499, 500, 501, 520])
def test_cluster_bound_of_the_reference(n):
    """A start with exactly n cycles at the reference's own bound of 500: 499 are kept and every
    other candidate of the array is then visited; from the 500th on the entry is emptied each
    time, nothing is marked visited, FindCycle repeats its last frame until the step cap ends it,
    and the other candidates are searched afterwards. That the start has n cycles, no more (two
    random spacers can share enough symbols to add some), is counted by an oracle run whose bound
    is out of reach."""
    _require_reference()
    k = 15
    rng = np.random.default_rng(1000 + n)
    path, rep, _ = RC.array_path(rng, k, 18, [int(x) for x in rng.integers(20, 31, size=n)])
    keys, mult, index = RC.graph_from_paths(k, [path], 50, {rep[:k + 1]: 300})
    e0 = index[rep[:k + 1]]
    unbounded = O.OGraph.from_arrays(keys, mult, k).cycle_finder(cluster_bound=60000)
    assert [(s, len(c)) for s, c in unbounded["entries"]] == [(e0, n)]
    ref = _both(keys, mult, k)
    assert ref["candidates"][0] == e0
    got = dict(ref["entries"])
    if n < 500:
        assert len(got[e0]) == n and len(got) == 1
    else:
        assert got[e0] == [] and len(got) > 1 and 0 < ref["stats"][5] < 500


@pytest.mark.parametrize("drop,kept", [(0.3, True), (0.2, False)])
def test_step_cap_of_the_reference(drop, kept):
    """One FindCycle on either side of the reference's cap of 10 000 000 steps (RC.step_cap_graph
    at k = 7: the start's only cycles lie on its last out-edge, behind a search of the rest of the
    graph). With 30 % of the other edges invalid that search takes 9 856 879 steps (counted with
    an instrumented copy of the oracle) and both cycles are recorded; with 20 % it would take
    13 475 081, the cap ends it and the entry is empty although DepthLevelSearch found a cycle.
    A restatement whose cap lies outside (9.86 M, 13.47 M), or that has none, differs here."""
    _require_reference()
    k = 7
    keys, mult, valid, start = RC.step_cap_graph(k, drop)
    ref = _both(keys, mult, k, valid=valid, threshold_multiplicity=60000)
    assert ref["candidates"] == [start]
    assert [(s, len(c)) for s, c in ref["entries"]] == [(start, 2 if kept else 0)]


@pytest.mark.parametrize("name", ["palindromes_k7", "palindromes_k9", "long_peel_400", "long_peel_6000"])
def test_read_sets_of_the_gpu_edge_cases(name):
    """The palindrome / homopolymer read set and the two long-peel read sets of test_gpu_parity.py."""
    _require_reference()
    case = G.CASES[name]
    keys, mult = G.case_graph(case)
    _both(keys, mult, case["k"], **case["params"])


# ------------------------------------------------------------------ fixtures
def _load(name):
    with open(G.fixture_path(name)) as f:
        return json.load(f)


def test_every_case_has_its_fixture_and_no_other():
    have = sorted(f[4:-5] for f in os.listdir(G.OUT_DIR) if f.startswith("ref_") and f.endswith(".json"))
    assert have == sorted(G.CASES)
    for name in have:
        assert os.path.getsize(G.fixture_path(name)) <= G.SIZE_LIMIT


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_fixture_is_fresh(name):
    """The committed fixture equals a fresh run of the live reference: a stale or hand-edited
    file cannot pass where the reference is present."""
    _require_reference()
    assert json.loads(G.dumps(G.make_fixture(name))) == _load(name)


def test_cluster500_fixture_shows_the_clear():
    """No reference needed. An oracle run on the fixture's graph with a bound out of reach counts
    520 cycles for each strand's first repeat edge, and for no other start 500 or more: these two
    reached the reference's bound. The record has an empty entry for both, counts nothing for them
    in the total, and holds cycles for starts searched after them."""
    fx = _load("cluster500")
    case = G.CASES["cluster500"]
    og = O.OGraph.build(*G.case_reads(case), case["k"], threads=4)
    unbounded = {s: len(c) for s, c in og.cycle_finder(cluster_bound=60000, **case["params"])["entries"]}
    over = sorted(s for s, n in unbounded.items() if n >= 500)
    assert len(over) == 2 and [unbounded[s] for s in over] == [520, 520]
    counts = dict(zip(fx["entry_starts"], fx["entry_cycle_counts"]))
    assert [counts.get(s) for s in over] == [0, 0]
    assert fx["candidates"][:2] == over and fx["buckets"][0] == fx["buckets"][1] == 16
    assert fx["stats"][5] == sum(fx["entry_cycle_counts"]) > 0 and max(fx["entry_cycle_counts"]) < 500
    assert fx["params"] == {} and fx["spec"]["spacers_per_array"] == 520


def test_map_order_model_through_rehashes(tmp_path):
    """The unordered_map model of tests/ref_cases.py, which the GPU tests use to put commit order
    into map order, against a compiled libstdc++ probe on key sets that pass several bucket
    counts (13, 29, 59, 127, 257, 541), and against the recorded map order of cluster500."""
    import subprocess

    src = tmp_path / "mapprobe.cpp"
    src.write_text(r'''
#include <unordered_map>
#include <cstdio>
#include <cstdint>
int main(){ int n; while (scanf("%d", &n) == 1) { std::unordered_map<uint64_t, int> m; uint64_t v;
  for (int i = 0; i < n; ++i) { scanf("%lu", &v); m[v] = i; }
  for (auto &kv : m) printf("%lu ", kv.first); printf("\n"); } }''')
    exe = tmp_path / "mapprobe"
    subprocess.run(["g++", "-O1", "-std=c++17", str(src), "-o", str(exe)], check=True)
    rng = np.random.default_rng(0)
    sets = []
    for n in (1, 5, 13, 14, 29, 30, 59, 60, 128, 257, 258, 542, 700):
        sets.append([int(x) for x in rng.choice(1 << 20, size=n, replace=False)])
        sets.append([int(x) for x in np.sort(rng.choice(4 * n + 8, size=n, replace=False))])  # dense, ascending
    inp = "".join(f"{len(s)} " + " ".join(map(str, s)) + "\n" for s in sets)
    out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, check=True).stdout.splitlines()
    for s, line in zip(sets, out):
        assert RC.unordered_map_order(s) == [int(x) for x in line.split()], len(s)
    # the recorded starts are in the reference's map order; their commit order is the candidates'
    # (bucket descending, id ascending)
    fx = _load("cluster500")
    assert fx["n_entries"] > 257
    have = set(fx["entry_starts"])
    assert RC.unordered_map_order([c for c in fx["candidates"] if c in have]) == fx["entry_starts"]


# ------------------------------------------------------------------ GPU: HIP against the record
def _device_graph(ctx, case):
    """The case's graph built on the device, and what has to stay alive with it."""
    import mcaat_amd as M
    from tests.helpers import HipBuffer

    if "arrays" in case:
        keys, mult = G.case_graph(case)
        kb, mb = HipBuffer(keys), HipBuffer(mult)
        return M.Graph.from_sorted(ctx, case["k"], kb.addr, mb.addr, int(keys.size)), (kb, mb)
    if "spec" in case:
        reads = M.Reads.synth(ctx, M.SynthSpec(**case["spec"]))
    else:
        reads = M.Reads.from_host(ctx, *G.case_reads(case))
    return M.Graph.build(ctx, reads, case["k"]), reads


def _gpu_case(gpu_ctx, name, **knobs):
    import mcaat_amd as M

    fx = _load(name)
    case = G.CASES[name]
    assert {k: fx[k] for k in case} == json.loads(json.dumps(case)), "the fixture was recorded for other inputs"
    g, keep = _device_graph(gpu_ctx, case)
    keys, mult, valid = g.download()
    assert g.size == fx["D"]
    assert RC.sha_bytes(keys.astype("<u8")) == fx["keys_sha256"]
    assert RC.sha_bytes(mult.astype("<u2")) == fx["mult_sha256"]
    drop = G.case_invalid_ids(case, g.size)
    if drop.size:
        g.set_valid(drop, False)
    prm = M.CfParams(**case["params"])
    assert (prm.cluster_bound, prm.step_cap) == (500, 10_000_000)
    with gpu_ctx.knobs(**knobs):
        res = g.cycle_finder(prm)
    del keep
    assert res.stats[:6] == fx["stats"]
    assert res.candidates == fx["candidates"]
    assert res.buckets == fx["buckets"]
    by_start = dict(res.entries)
    assert len(by_start) == len(res.entries) == fx["n_entries"]
    order = RC.unordered_map_order([s for s, _ in res.entries])
    assert order == fx["entry_starts"]
    entries = [[s, by_start[s]] for s in order]
    assert [len(c) for _, c in entries] == fx["entry_cycle_counts"]
    assert entries[:len(fx["entries"])] == fx["entries"]
    assert RC.entries_digest(entries) == fx["entries_sha256"]
    _, _, valid = g.download()
    assert RC.valid_digest(valid) == (fx["valid_sha256"], fx["valid_popcount"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_hip_equals_reference_record(gpu_ctx, name):
    _gpu_case(gpu_ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [0, 1])
def test_hip_equals_reference_record_cluster500_compact(gpu_ctx, compact):
    """520 cycles of 62 nodes from one start on the device before the entry is emptied, with and
    without the compacted edge slots."""
    _gpu_case(gpu_ctx, "cluster500", cf__compact=compact)
