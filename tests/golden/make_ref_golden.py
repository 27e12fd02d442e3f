"""Regenerate tests/golden/ref_<case>.json: what the REFERENCE PROGRAM's own CycleFinder gives
(its cycle_finder.cpp behind the stand-in SDBG, oracle/_ref/ref_cf, threads = 1) on the graphs
this project builds for the cases below. Recorded data only.

Build machine only (needs `make -C oracle ref`). Run: python tests/golden/make_ref_golden.py
tests/test_reference_cycle_finder.py regenerates every fixture in memory where the reference is
present and compares it with the committed file, and runs the HIP path against the files.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mcaat_amd as M  # noqa: E402
import oracle as O  # noqa: E402
from tests import ref_cases as RC  # noqa: E402

OUT_DIR = os.path.dirname(os.path.abspath(__file__))
SIZE_LIMIT = 60_089  # bytes: the largest fixture in tests/golden/ before these (low_thr_k23.json)
FULL_ENTRIES = 20    # a case over the limit keeps at most this many leading entries in full

_PE_ERR = dict(seed=7, n_genomes=4, genome_len=20_000, arrays_per_genome=2, spacers_per_array=8,
               repeat_len_min=32, repeat_len_max=36, spacer_len_min=30, spacer_len_max=36,
               n_reads=24_000, error_rate=0.002, paired=True)

# name -> inputs. "spec": SynthSpec fields (reads of mcaat_synth_host); "reads": a recipe of
# tests/ref_cases.py with its arguments; "arrays": a graph recipe of tests/ref_cases.py.
# "invalid": (fraction, rng seed) of edges cleared before CycleFinder runs, drawn as in
# test_gpu_parity.py::test_cycle_finder_on_a_graph_with_invalid_edges.
CASES = {
    "c1_k23": dict(spec=dict(), k=23, params=dict()),
    "c1_k27": dict(spec=dict(), k=27, params=dict()),
    "pe_err": dict(spec=_PE_ERR, k=23, params=dict(threshold_multiplicity=5)),
    "low_thr": dict(spec=dict(seed=11, n_genomes=3, genome_len=15_000, arrays_per_genome=2, spacers_per_array=10,
                              repeat_len_min=30, repeat_len_max=34, spacer_len_min=30, spacer_len_max=34,
                              n_reads=12_000, error_rate=0.004), k=23,
                    params=dict(threshold_multiplicity=2, low_abundance=True)),
    "low_abundance_false": dict(spec=dict(seed=12, n_genomes=2, genome_len=12_000, arrays_per_genome=1,
                                          spacers_per_array=6, n_reads=8_000, error_rate=0.003), k=21,
                                params=dict(threshold_multiplicity=3, low_abundance=False, cycle_min_length=20,
                                            cycle_max_length=70)),
    "pe_err_invalid02": dict(spec=_PE_ERR, k=23, params=dict(threshold_multiplicity=5), invalid=(0.02, 2)),
    "pe_err_invalid30": dict(spec=_PE_ERR, k=23, params=dict(threshold_multiplicity=5), invalid=(0.3, 30)),
    "palindromes_k7": dict(reads=("palindrome_reads", []), k=7,
                           params=dict(threshold_multiplicity=1, cycle_min_length=1, cycle_max_length=20)),
    "palindromes_k9": dict(reads=("palindrome_reads", []), k=9,
                           params=dict(threshold_multiplicity=1, cycle_min_length=1, cycle_max_length=20)),
    "long_peel_400": dict(reads=("long_peel_reads", [400]), k=23, params=dict(threshold_multiplicity=2)),
    "long_peel_6000": dict(reads=("long_peel_reads", [6000]), k=23, params=dict(threshold_multiplicity=2)),
    "mult_boundary": dict(arrays="multiplicity_boundary_graph", k=15, params=dict()),
    # 520 spacers through one 30-base repeat. Each strand's first repeat edge has 520 cycles, passes
    # the reference's cluster bound of 500 and is recorded with an empty entry; it is not marked
    # visited, the printed total counts nothing for it, and FindCycle then repeats its last frame
    # until the step cap ends it. 100 000 reads, not fewer: the repeat occurs 521 times, so at low
    # coverage `repeat_multiplicity / neighbor_multiplicity > 500` cuts most spacers (at 20 000
    # reads no start keeps more than 100 cycles); here the repeat saturates at 65535 and every
    # spacer edge lies above 130, so all 520 pass.
    "cluster500": dict(spec=dict(seed=5, genome_len=60_000, spacers_per_array=520, repeat_len_min=30,
                                 repeat_len_max=30, n_reads=100_000), k=23, params=dict()),
}


def case_reads(case):
    """(packed, offsets) of a case given by spec or by read recipe, else None."""
    if "spec" in case:
        return M.synth_host(M.SynthSpec(**case["spec"]))
    if "reads" in case:
        name, args = case["reads"]
        return RC.packed_reads(getattr(RC, name)(*args))
    return None


def case_graph(case):
    """(keys, mult) on the host: the arrays recipe itself, or the oracle's build of the reads
    (the GPU tests check the device build against the recorded digests of these)."""
    if "arrays" in case:
        keys, mult = getattr(RC, case["arrays"])()[:2]
        return keys, mult
    packed, offs = case_reads(case)
    return O.OGraph.build(packed, offs, case["k"], threads=4).arrays()


def case_invalid_ids(case, D):
    if "invalid" not in case:
        return np.zeros(0, dtype=np.uint64)
    frac, seed = case["invalid"]
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(D, size=int(frac * D), replace=False)).astype(np.uint64)


def make_fixture(name):
    """The fixture of a case as a dict, from a live run of the reference runner."""
    case = CASES[name]
    keys, mult = case_graph(case)
    valid = np.ones(keys.size, dtype=np.uint8)
    valid[case_invalid_ids(case, keys.size).astype(np.int64)] = 0
    res = O.ref_cycle_finder(keys, mult, case["k"], valid=valid, **case["params"])
    vsha, vpop = RC.valid_digest(res["valid"])
    fx = {k: v for k, v in case.items()}
    for key in ("reads", "invalid"):
        if key in fx:
            fx[key] = list(fx[key])
    entries = [[s, c] for s, c in res["entries"]]
    fx.update({
        "D": int(keys.size),
        "keys_sha256": RC.sha_bytes(keys.astype("<u8")),
        "mult_sha256": RC.sha_bytes(mult.astype("<u2")),
        "stats": res["stats"],
        "candidates": res["candidates"],
        "buckets": res["buckets"],
        "n_entries": len(entries),
        "entry_starts": [e[0] for e in entries],
        "entry_cycle_counts": [len(e[1]) for e in entries],
        "entries_sha256": RC.entries_digest(entries),
        "entries": entries,
        "valid_sha256": vsha,
        "valid_popcount": vpop,
    })
    # over the size limit: the leading entries in full (at most FULL_ENTRIES, fewer if even those
    # do not fit), the rest by entries_sha256 and the per-entry counts above
    keep = len(entries)
    while len(dumps(fx)) > SIZE_LIMIT and keep > 0:
        keep = min(keep - 1, FULL_ENTRIES)
        fx["entries"] = entries[:keep]
    assert len(dumps(fx)) <= SIZE_LIMIT, name
    return fx


def dumps(fx):
    return json.dumps(fx, separators=(",", ":"), sort_keys=True)


def fixture_path(name):
    return os.path.join(OUT_DIR, f"ref_{name}.json")


def main():
    for name in CASES:
        fx = make_fixture(name)
        with open(fixture_path(name), "w") as f:
            f.write(dumps(fx) + "\n")
        print(name, fx["D"], fx["stats"], "entries", fx["n_entries"], "in full", len(fx["entries"]),
              "bytes", len(dumps(fx)))


if __name__ == "__main__":
    main()
