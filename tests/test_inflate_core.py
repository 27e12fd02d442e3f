"""The DEFLATE token decoder and CRC merge the BGZF inflate kernel runs (mcaat_amd/csrc/inflate_core.h)
against zlib, in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer
(tests/sanitize/inflate_core_test.cpp): round trips over stored, fixed and dynamic blocks, several
blocks per member, the copy edge cases (dist 1 / len 258, distance 32768, a match ending on the
last byte), the CRC merge over unequal and empty slices, and 2,000 mutated streams (bit flip,
byte overwrite, truncation) whose verdict must be zlib's, with input and output buffers
allocated at exactly their lengths. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitized_standalone_against_zlib(tmp_path):
    exe = tmp_path / "inflate_core_test"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                    os.path.join(ROOT, "tests", "sanitize", "inflate_core_test.cpp"), "-o", str(exe), "-lz"],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "inflate_core ok" in p.stdout, (p.stdout + p.stderr)[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
