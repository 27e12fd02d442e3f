"""Strand-canonical super-k-mer descriptors (mcaat_amd/csrc/desc_canon.h): the host entry
mcaat_desc_canonical against a plain string model (reverse, complement, pack), and the same
sweep in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer
(tests/sanitize/desc_canon_test.cpp). No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mcaat_amd as M
from tests.helpers import lsb_value, rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SHIFT, H_SHIFT, DESC_BASES = 44, 50, 54
BASE1 = (1 << N_SHIFT) - 1
ES = (16, 24, 28, 31)


def pack(s):
    v = lsb_value(s)
    return v & ((1 << 64) - 1), v >> 64


def canon(s, E, hbits):
    n = len(s) - E + 1
    w0, b1 = pack(s)
    o0, o1 = M.desc_canonical(w0, b1 | (n << N_SHIFT) | (hbits << H_SHIFT), E)
    assert o1 >> N_SHIFT == n | (hbits << (H_SHIFT - N_SHIFT)), (s, E)  # n and the hash bits pass through
    return o0, o1 & BASE1


def check(s, E, hbits):
    L = len(s)
    f, r = pack(s), pack(rc(s))
    got = canon(s, E, hbits)
    assert got in (f, r), (s, E)
    assert got == min(f, r), (s, E)  # the smaller w0, then the smaller base bits of w1
    assert got == canon(rc(s), E, hbits), (s, E)
    assert (got[0] | (got[1] << 64)) >> (2 * L) == 0, (s, E)
    assert got[0] != (1 << 64) - 1, (s, E)


def strings(E):
    rng = np.random.default_rng(E)
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n))  # noqa: E731
    for n in range(1, DESC_BASES - E + 2):
        L = n + E - 1
        for rep in range(8):
            s = rand(L)
            yield s
            run = int(rng.integers(1, L + 1))  # a single-base run at either end
            yield ("TA"[rep & 1] * run + s[run:]) if rep & 2 else (s[:L - run] + "TA"[rep & 1] * run)
        yield "T" * L
        yield "A" * L
        if L % 2 == 0:
            h = rand(L // 2)
            yield h + rc(h)  # its own reverse complement


@pytest.mark.parametrize("E", ES)
def test_against_string_model(E):
    rng = np.random.default_rng(100 + E)
    lengths = set()
    for s in strings(E):
        lengths.add(len(s))
        check(s, E, int(rng.integers(0, 1 << 14)))
    assert {32, 33, 54} <= lengths and lengths == set(range(E, DESC_BASES + 1))


@pytest.mark.parametrize("E", ES)
def test_padding_passes_through(E):
    assert M.desc_canonical(0, 0, E) == (0, 0)
    w0, w1 = 0x0123456789ABCDEF, 0x00000FEDCBA98765 | (0x2ABC << H_SHIFT)  # n = 0, other bits set
    assert M.desc_canonical(w0, w1, E) == (w0, w1)


def test_self_reverse_complement_is_kept():
    for E in ES:
        s = "ACGTTGCAAGCT" * 2 + "AT"
        s = s + rc(s)
        assert len(s) <= DESC_BASES and rc(s) == s
        if len(s) >= E:
            assert canon(s, E, 5) == pack(s)


def test_rejects_descriptors_longer_than_the_field():
    with pytest.raises(M.McaatError):
        M.desc_canonical(0, (DESC_BASES - 31 + 2) << N_SHIFT, 31)
    with pytest.raises(M.McaatError):
        M.desc_canonical(0, 1 << N_SHIFT, 32)


def test_sanitized_standalone_sweep(tmp_path):
    exe = tmp_path / "desc_canon_test"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                    os.path.join(ROOT, "tests", "sanitize", "desc_canon_test.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "desc_canon ok" in p.stdout, (p.stdout + p.stderr)[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
