"""Sender-side collapse of the sharded build's descriptor exchange (knob dist.preagg):
every rank collapses its own super-k-mer descriptors before the exchange and sends each distinct
one once with a multiplicity; the owners count weighted descriptors. The graph and the CycleFinder
results must equal the one-GPU path's bit for bit (tools/native_multi_check.py compares keys,
multiplicities, valid bits, entries, candidates, buckets and stats), the collapse must conserve
the descriptors it is given (mcaat_desc_preaggregate), and it must shrink what a rank hands to
the exchange when descriptors repeat."""
import hashlib
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mcaat_amd as M  # noqa: E402

PREAGG = ("--knob", "dist.preagg=1")


def _spawn(argv_list, timeout=600):
    procs = [subprocess.Popen(a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for a in argv_list]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=timeout)
            outs.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return outs


def _ranks(world, extra=()):
    name = f"/mcaat_p_{uuid.uuid4().hex[:12]}"
    script = os.path.join(ROOT, "tools", "native_multi_check.py")
    return _spawn([[sys.executable, script, "--world", str(world), "--rank", str(r), "--comm", "shm", "--name", name,
                    *PREAGG, *extra] for r in range(world)])


def _assert_ok(outs, sharded=False):
    for rc, o, e in outs:
        assert rc == 0, (o[-2000:], e[-3000:])
        assert "NATIVE_MULTI_OK" in o, o
        if sharded:
            assert "sharded=True" in o, o


@pytest.mark.gpu
@pytest.mark.parametrize("world,extra", [(1, ("--knob", "dist.segs_at_one=1")), (1, ()), (2, ()), (3, ())])
def test_preagg_parity_default_case(world, extra):
    """30,000 synthetic reads through 1 (segment exchange forced; and the rank keeping its collapsed
    buckets in place), 2 and 3 shared-memory ranks."""
    _assert_ok(_ranks(world, extra))


@pytest.mark.gpu
@pytest.mark.parametrize("case,world", [("pe_err", 2), ("pe_err", 4), ("low_thr", 2), ("low_thr", 4),
                                        ("c5_sample", 2), ("c5_sample", 4), ("c3_sample", 8)])
def test_preagg_parity_cases(case, world):
    """Paired-end with errors, threshold 2 and the C5 sample (shallow, error-rich: few descriptors
    repeat) at 2 and 4 ranks, the C3 sample at 8."""
    _assert_ok(_ranks(world, ("--case", case, "--slot", "0")), sharded=True)


@pytest.mark.gpu
@pytest.mark.parametrize("world,knobs", [
    (2, ("nc.desc_cap=4",)),      # every partition splits into classes, then leaves raw
    (3, ("nc.edge_cap=8",)),      # the owner's weighted edge table overflows: weighted k_fallback
    (2, ("nc.group_budget=20000",)),  # several groups on the sender and on the owner
    (3, ("nc.fine_bits=8",)),     # large partitions
    (2, ("nc.big_table=1",)),
    (3, ("nc.overlap=0",)),
])
def test_preagg_forced_paths(world, knobs):
    extra = []
    for kv in knobs:
        extra += ["--knob", kv]
    _assert_ok(_ranks(world, tuple(extra)))


def _default_spec(n_reads=30000):  # the default case of tools/native_multi_check.py
    return M.SynthSpec(seed=11, n_genomes=3, genome_len=40_000, arrays_per_genome=2, spacers_per_array=10,
                       repeat_len_min=30, repeat_len_max=34, spacer_len_min=30, spacer_len_max=36,
                       n_reads=n_reads, error_rate=2e-3)


@pytest.mark.gpu
def test_preagg_conserves_descriptors(gpu_ctx):
    """The weights a rank emits add up to the live descriptors it was given, at default knobs (no
    raw records on this input) and with a 4-descriptor table (raw records)."""
    reads = M.Reads.synth(gpu_ctx, _default_spec())
    try:
        d = M.desc_preaggregate(gpu_ctx, reads, 27)
        print("default knobs:", d)
        assert d["live_in"] > 0
        assert d["weight_sum"] == d["live_in"]
        assert d["records_out"] <= d["live_in"]
        assert d["raw"] == 0
        assert "shard_preagg" in gpu_ctx.stage_times()
        gpu_ctx.set_knob("nc.desc_cap", 4)
        try:
            r = M.desc_preaggregate(gpu_ctx, reads, 27)
        finally:
            gpu_ctx.set_knob("nc.desc_cap", -1)
        print("nc.desc_cap=4:", r)
        assert r["live_in"] == d["live_in"]
        assert r["weight_sum"] == r["live_in"]
        assert r["records_out"] <= r["live_in"]
        assert 0 < r["raw"] <= r["records_out"]
        assert r["records_out"] >= d["records_out"]
    finally:
        reads.free()


N_PAIRS, READ_LEN, K_TWICE = 10_000, 150, 27


def _twice_reads(first_pair, n_pairs):
    """Pairs [first_pair, first_pair + n_pairs) of a fixed random read set in which every read
    appears twice in a row, packed 2 bits per base (32 bases per word, LSB first)."""
    rng = np.random.default_rng(2027)
    codes = rng.integers(0, 4, size=(N_PAIRS, READ_LEN), dtype=np.uint8)[first_pair:first_pair + n_pairs]
    codes = np.repeat(codes, 2, axis=0).reshape(-1).astype(np.uint64)
    pad = (-codes.size) % 32
    codes = np.concatenate([codes, np.zeros(pad, dtype=np.uint64)]).reshape(-1, 32)
    packed = (codes << (np.uint64(2) * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    offsets = np.arange(2 * n_pairs + 1, dtype=np.uint64) * np.uint64(READ_LEN)
    return packed, offsets


_TWICE_RANK = r"""
import hashlib, sys, numpy as np
sys.path.insert(0, {root!r})
import mcaat_amd as M
from tests.test_preagg import _twice_reads, N_PAIRS, K_TWICE
world, rank, name = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
ctx = M.Context(0)
for kv in sys.argv[4:]:
    kn, kval = kv.split("=")
    ctx.set_knob(kn, int(kval))
comm = M.Comm.shm(ctx, world, rank, name, 1 << 20)
first = rank * N_PAIRS // world
packed, offsets = _twice_reads(first, (rank + 1) * N_PAIRS // world - first)
reads = M.Reads.from_host(ctx, packed, offsets)
ctx.reset_timing()
g = M.Graph.build_sharded(ctx, comm, reads, K_TWICE)
stats = {{n: ctx.kernel_timing(n)[1] for n in ("xb_desc", "preagg_in", "preagg_out", "preagg_raw")}}
stages = sorted(ctx.stage_times())
g.unshard(comm)
keys, mult, _ = g.download()
h = hashlib.sha256(keys.tobytes() + mult.tobytes()).hexdigest()
g.free()
reads.free()
comm.barrier()
comm.close()
ctx.close()
print("TWICE", rank, stats["xb_desc"], stats["preagg_in"], stats["preagg_out"], stats["preagg_raw"], len(keys), h,
      int("shard_preagg" in stages))
"""


def _twice_ranks(world, knobs):
    name = f"/mcaat_p_{uuid.uuid4().hex[:12]}"
    code = _TWICE_RANK.format(root=ROOT)
    outs = _spawn([[sys.executable, "-c", code, str(world), str(r), name, *knobs] for r in range(world)])
    rows = []
    for rc, o, e in outs:
        assert rc == 0, (o[-2000:], e[-3000:])
        f = [ln for ln in o.splitlines() if ln.startswith("TWICE")][0].split()
        rows.append({"xb": int(f[2]), "in": int(f[3]), "out": int(f[4]), "raw": int(f[5]), "D": int(f[6]),
                     "digest": f[7], "stage": int(f[8])})
    return rows


@pytest.mark.gpu
def test_preagg_collapses_repeated_reads(gpu_ctx):
    """Every read twice: a 150-base read is one pass-A work item, so the two copies give identical
    descriptors in the same partitions, and with no raw records at most half the live descriptors
    leave. Through 2 ranks the bytes handed to the exchange are strictly fewer with the collapse,
    the build-stage statistics are filled, and the graph is the same; with a 4-descriptor table the
    statistics report raw records."""
    packed, offsets = _twice_reads(0, N_PAIRS)
    reads = M.Reads.from_host(gpu_ctx, packed, offsets)
    try:
        d = M.desc_preaggregate(gpu_ctx, reads, K_TWICE)
    finally:
        reads.free()
    print("every read twice:", d)
    assert d["raw"] == 0 and d["weight_sum"] == d["live_in"] > 0
    assert 2 * d["records_out"] <= d["live_in"]

    plain = _twice_ranks(2, ())
    agg = _twice_ranks(2, ("dist.preagg=1",))
    raw = _twice_ranks(2, ("dist.preagg=1", "nc.desc_cap=4"))
    print("plain", plain, "\npreagg", agg, "\npreagg, nc.desc_cap=4", raw)
    for r in range(2):
        assert plain[r]["xb"] > 0 and plain[r]["stage"] == 0 and plain[r]["in"] == plain[r]["out"] == 0
        assert agg[r]["xb"] < plain[r]["xb"]
        assert agg[r]["stage"] == 1 and agg[r]["raw"] == 0
        assert 0 < 2 * agg[r]["out"] <= agg[r]["in"]
        # 22 B per record in whole 8-slot groups per L1 bucket
        assert 22 * agg[r]["out"] <= agg[r]["xb"] <= 22 * (agg[r]["out"] + 7 * 256)
        assert raw[r]["raw"] > 0 and raw[r]["in"] == agg[r]["in"]
        assert (agg[r]["D"], agg[r]["digest"]) == (plain[r]["D"], plain[r]["digest"])
        assert (raw[r]["D"], raw[r]["digest"]) == (plain[r]["D"], plain[r]["digest"])


@pytest.mark.gpu
def test_preagg_knob_is_known(gpu_ctx):
    """mcaat_set_knob takes dist.preagg (creating a context needs a device, hence a GPU test)."""
    gpu_ctx.set_knob("dist.preagg", 1)
    gpu_ctx.set_knob("dist.preagg", -1)
    with pytest.raises(M.McaatError):
        gpu_ctx.set_knob("dist.preag", 1)
