"""CPU tests of the C ABI library (loads, exports every declared symbol, fails cleanly
without a GPU), the host-side synthetic generator, and the bench's multi-rank control flow."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mcaat_amd as M
from mcaat_amd import lib as L
from tests.helpers import unpack_read, rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    txt = open(os.path.join(ROOT, "include", "mcaat_gpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mcaat_[a-z_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = M.load_library()
    names = declared_functions()
    assert len(names) >= 30
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [n for n in names if n not in exported]
    assert not missing, missing
    for n in names:
        assert hasattr(lib, n)
    # and the Python binding declares a signature for each of them
    assert sorted(L.SIGNATURES) == names


def test_init_without_gpu_fails_cleanly():
    if M.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(M.McaatError) as ei:
        M.Context(0)
    assert ei.value.code == -2  # MCAAT_E_HIP
    assert "device" in str(ei.value)


def test_default_cf_params_match_reference_settings():
    p = L._CfParams()
    M.load_library().mcaat_cf_default_params(p)
    # settings.h:34-37, cycle_finder.cpp:132,149
    assert (p.threshold_multiplicity, p.low_abundance, p.cycle_max_length, p.cycle_min_length) == (20, 1, 77, 27)
    assert (p.cluster_bound, p.step_cap) == (500, 10_000_000)


def test_synth_reads_are_genome_segments():
    spec = M.SynthSpec(seed=5, n_genomes=2, genome_len=5000, arrays_per_genome=1, spacers_per_array=4,
                       n_reads=300, read_len=100)
    packed, offs = M.synth_host(spec)
    gen = M.synth_genome_host(spec)
    genomes = [unpack_read(gen, g * 5000, (g + 1) * 5000) for g in range(2)]
    both = genomes + [rc(x) for x in genomes]
    for r in range(spec.n_reads):
        s = unpack_read(packed, int(offs[r]), int(offs[r + 1]))
        assert any(s in x for x in both)
    # deterministic
    p2, _ = M.synth_host(spec)
    assert np.array_equal(packed, p2)


def test_synth_paired_reads_and_errors():
    spec = M.SynthSpec(seed=9, n_genomes=1, genome_len=4000, arrays_per_genome=0, n_reads=400, read_len=80,
                       paired=True, error_rate=0.0)
    packed, offs = M.synth_host(spec)
    g = unpack_read(M.synth_genome_host(spec), 0, 4000)
    for p in range(0, 400, 2):
        r1 = unpack_read(packed, int(offs[p]), int(offs[p + 1]))
        r2 = unpack_read(packed, int(offs[p + 1]), int(offs[p + 2]))
        # mates face each other on opposite strands within 270..330 bp
        if r1 in g:
            i1, i2 = g.find(r1), g.find(rc(r2))
        else:
            i1, i2 = g.find(rc(r1)), g.find(r2)
        assert i1 >= 0 and i2 >= 0
        assert 270 <= abs(i2 - i1) + 80 <= 330
    spec.error_rate = 0.05
    pe, _ = M.synth_host(spec)
    diff = int(np.count_nonzero(pe != packed))
    assert diff > 0


@pytest.mark.parametrize("mode,port", [("replicas", 29561), ("shard", 29562)])
def test_bench_two_ranks_gloo_dry_run(mode, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", "tiny", "--dry-run", "--mode", mode]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1
    # value = all k-mers processed / max-over-ranks step time (rank 1 sleeps longer)
    assert d["ms_per_step"] >= 19.0
    total = d["config"]["kmers_total"]
    assert abs(d["value"] - total / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    if mode == "replicas":
        assert d["scaling"] == "weak" and total == 2 * d["config"]["kmers_per_gpu"]
    else:  # one dataset split over the ranks
        assert d["scaling"] == "strong" and total == 2 * d["config"]["kmers_per_gpu"]
        assert d["config"]["reads_total"] == 10_000


def test_bench_dump_arrays_layout_and_sample(tmp_path):
    """bench.py --dump-outputs: the flat float64 layout of one step's results, and the fixed
    sample that keeps a large dump within its size limit."""
    import bench

    u64 = lambda *x: np.array(x, dtype=np.uint64)  # noqa: E731
    res = M.CycleResult(entries=[(7, (u64(7, 8, 9, 7, 3), u64(0, 3, 5))), (2, (u64(2, 4), u64(0, 2)))],
                        stats=[1, 2, 3, 4, 5, 3, 0, 1], candidates=u64(2, 7), buckets=np.array([0, 1], np.int32))
    a = bench.dump_arrays(1 << 40, res)
    assert all(v.dtype == np.float64 and v.ndim == 1 for v in a.values())
    assert a["sdbg_edges"].tolist() == [float(1 << 40)]
    assert a["cycle_starts"].tolist() == [7, 2]
    assert a["cycle_entry_offsets"].tolist() == [0, 2, 3]
    assert a["cycle_offsets"].tolist() == [0, 3, 5, 7]
    assert a["cycle_nodes"].tolist() == [7, 8, 9, 7, 3, 2, 4]
    assert a["cf_stats"].tolist() == res.stats
    assert a["start_candidates"].tolist() == [2, 7] and a["candidate_buckets"].tolist() == [0, 1]
    empty = bench.dump_arrays(0, M.CycleResult(stats=[0] * 8, candidates=u64(), buckets=np.zeros(0, np.int32)))
    assert empty["cycle_nodes"].size == 0 and empty["cycle_offsets"].tolist() == [0]
    res.entries[0] = (1 << 53, res.entries[0][1])  # float64 would round it
    with pytest.raises(ValueError):
        bench.dump_arrays(1, res)

    big = {"small": np.arange(10, dtype=np.float64), "big": np.arange(5000, dtype=np.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, limit=8000)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in big}
    assert np.array_equal(got["small"], big["small"])
    assert 0 < got["big"].size < 5000 and sum(v.nbytes for v in got.values()) <= 8000
    assert np.all(np.diff(got["big"]) > 0)  # a subset of the array, in its order
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))  # the same sample every run


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_step_results(gpu_ctx, tmp_path):
    """A plain bench run times the steps and leaves the --full measurements out of its line;
    --dump-outputs writes what the library returns for the same config."""
    import bench
    from mcaat_amd.configs import CONFIGS

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--config", "tiny", "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["kmers_total"] / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    for key in ("e2e", "post_path", "fastq_ingest", "cpu_baseline"):
        assert d[key] is None
    assert "span" not in d

    cfg = CONFIGS["tiny"]
    reads = M.Reads.synth(gpu_ctx, cfg["spec"])
    g = M.Graph.build(gpu_ctx, reads, cfg["k"])
    want = bench.dump_arrays(g.size, g.cycle_finder(M.CfParams(threshold_multiplicity=cfg["thr"]), as_arrays=True))
    g.free()
    reads.free()
    assert want["cycle_nodes"].size > 0 and want["sdbg_edges"][0] == d["config"]["sdbg_edges_D"]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(n + ".npy" for n in want)
    for name, a in want.items():
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a), name


def test_host_library_exports_every_declared_symbol():
    """libmcaat_host.so (include/mcaat_host.h): the downstream steps' C ABI."""
    from mcaat_amd import downstream as DS

    txt = open(os.path.join(ROOT, "include", "mcaat_host.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(mcaat_host_[a-z_]+)\s*\(", txt)))
    assert len(names) >= 6
    out = subprocess.run(["nm", "-D", "--defined-only", DS.HOST_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]
    assert sorted(DS.HOST_SIGNATURES) == names
    DS.load_host_library()
