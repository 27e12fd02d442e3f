"""node_counter on reads of both strands: pass B stores every super-k-mer descriptor in its
canonical orientation (mcaat_amd/csrc/desc_canon.h), so a read set, its reverse complement and
their union give the same canonical edges, and pass C's collapse sees the same distinct
descriptors for all three."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mcaat_amd as M
import oracle as O
from tests.helpers import rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (23, 27, 30)
_CODE = np.zeros(256, dtype=np.uint64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i


def pack(seqs):
    """tests.helpers.pack_reads, vectorised (same layout)."""
    codes = _CODE[np.frombuffer("".join(seqs).encode(), dtype=np.uint8)]
    total = codes.size
    words = np.zeros(((total + 31) // 32) * 32, dtype=np.uint64)
    words[:total] = codes
    words = np.bitwise_or.reduce(words.reshape(-1, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return words, offs


def fragments():
    """F: 2,000 random 150-bp fragments of a 20 kbp random genome."""
    rng = np.random.default_rng(20)
    genome = "".join(rng.choice(list("ACGT"), size=20_000))
    return [genome[a:a + 150] for a in rng.integers(0, 20_000 - 150, size=2000)]


def strand_inputs():
    f = fragments()
    r = [rc(s) for s in f]
    return {"F": f, "RC": r, "F+RC": f + r}


@pytest.fixture(scope="module")
def inputs():
    return {name: pack(seqs) for name, seqs in strand_inputs().items()}


@pytest.mark.parametrize("k", KS)
def test_count_parity_across_strands(gpu_ctx, inputs, k):
    got, want = {}, {}
    for name, (packed, offs) in inputs.items():
        got[name] = M.count_edges(gpu_ctx, M.Reads.from_host(gpu_ctx, packed, offs), k)
        want[name] = O.count_canonical(packed, offs, k, threads=4)
    fk, fc = got["F"]
    assert fk.size > 15_000
    assert np.array_equal(got["RC"][0], fk) and np.array_equal(got["RC"][1], fc)
    assert np.array_equal(got["F+RC"][0], fk) and np.array_equal(got["F+RC"][1], 2 * fc)
    for name in inputs:
        assert np.array_equal(got[name][0], want[name][0]) and np.array_equal(got[name][1], want[name][1]), name


@pytest.mark.parametrize("k", KS)
def test_count_parity_low_complexity(gpu_ctx, k):
    """F plus reads with a T run of 60-150, a read s + rc(s), and reads shorter than E + 4."""
    E = k + 1
    rng = np.random.default_rng(k)
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n))  # noqa: E731
    seqs = fragments()
    for i in range(40):
        flank = rand(70)
        t = flank[:30] + "T" * (60 + (i * 7) % 91) + flank[30:]
        seqs.append(t if i & 1 else rc(t))
    s = rand(75)
    seqs += [s + rc(s), rand(E + 2), rand(E), "T" * (E + 3), "A" * (E + 3)]
    packed, offs = pack(seqs)
    gk, gc = M.count_edges(gpu_ctx, M.Reads.from_host(gpu_ctx, packed, offs), k)
    ok, oc = O.count_canonical(packed, offs, k, threads=4)
    assert np.array_equal(gk, ok) and np.array_equal(gc, oc)


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import mcaat_amd as M
from tests.test_strand_collapse import pack, strand_inputs
with M.Context(0) as ctx:
    for name, seqs in strand_inputs().items():
        packed, offs = pack(seqs)
        keys, _ = M.count_edges(ctx, M.Reads.from_host(ctx, packed, offs), 27)
        sys.stderr.flush()
        print(name, keys.size, flush=True)
"""


def test_collapse_invariance():
    """The profiled build path (MCAAT_PROF_C=1, read once per process: a child) reports pass C's
    distinct descriptors X of Y live ones: X is the same for F, RC and F+RC, and Y doubles.
    Random fragments only: a super-k-mer longer than nmax is cut from the read's left, so the
    pieces of a low-complexity read mirror only by accident."""
    env = dict(os.environ, MCAAT_PROF_C="1")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    xy = [(int(x), int(y)) for x, y in re.findall(r"distinct descriptors (\d+) of (\d+)", p.stderr)]
    print(xy, p.stdout)
    assert len(xy) == 3, p.stderr[-3000:]
    (xf, yf), (xr, yr), (xb, yb) = xy
    assert xf > 1000
    assert xf == xr == xb
    assert yf == yr and yb == 2 * yf
