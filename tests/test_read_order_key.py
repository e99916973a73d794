"""The locus key of the seed stage's read ordering (pangea-plus_amd/csrc/read_order.hpp) on the host: the header is free of
HIP, so the rule the kernel compiles builds with plain g++ under AddressSanitizer + UndefinedBehaviorSanitizer into a program
of its own (tests/host/read_order_test.cpp), which checks the bin count and shift at n_bases = 1, 2^20, 10^9, 3 x 10^9 and
2^32 - 1, that the top position lands in a position bin, and the strand / probe choice against a brute-force restatement on
hand-made and random bucket contents.  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")


def test_read_order_key_rule_under_sanitizers():
    if not shutil.which("g++"):
        pytest.skip("no g++")
    os.makedirs(os.path.join(HERE, "bin"), exist_ok=True)
    exe = os.path.join(HERE, "bin", "read_order_asan")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(HERE, "read_order_test.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, env=env)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-3000:]
    assert out.count(" ok") == 4 and "DIFFERENT" not in out and "Sanitizer" not in out, out[-3000:]
