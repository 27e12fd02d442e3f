"""Where a FASTA file is cut into ranks' parts (mcaat_amd/csrc/fasta_split.h): the first line
start at or after a position whose byte is '>', swept over every start position of seeded texts
against a naive scan in a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer (tests/sanitize/fasta_split_test.cpp). No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitized_standalone_sweep(tmp_path):
    exe = tmp_path / "fasta_split_test"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                    os.path.join(ROOT, "tests", "sanitize", "fasta_split_test.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "fasta_split ok" in p.stdout, (p.stdout + p.stderr)[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
