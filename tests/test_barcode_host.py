"""The barcode demultiplexer's host-side text code (pangea-plus_amd/csrc/barcode_host.hpp: the barcode file, the walk back
over the last two records, the last record's rule) as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/host/barcode_host_test.cpp, tests/host/barcode.mk), on every golden case that holds both
inputs; what it prints is compared with tests/barcode_rule.py.  CPU only."""
import os
import shutil
import subprocess

import pytest

import barcode_rule
from conftest import GOLD

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
STATUS = {"E_ARG": -1, "E_LIMIT": -7, "E_REFHANG": -6}


def expected(case):
    src = os.path.join(GOLD, "barcode", case)
    btext = open(os.path.join(src, "barcodes.txt"), "rb").read()
    text = open(os.path.join(src, "reads.fas"), "rb").read()
    try:
        bars = barcode_rule.parse_barcodes(btext)
    except barcode_rule.Refused as r:
        return {"parse": STATUS[r.status]}
    want = {"parse": 0, "bars": len(bars)}
    try:
        recs = barcode_rule.records_of(text)
    except barcode_rule.Refused:
        return want  # (text before the first header: the device finds it, the host walk does not look that far)
    want["any"] = int(bool(recs))
    want["lines"] = len(recs[-1]) if recs else 0
    want["stale"] = len(recs[-2]) if len(recs) > 1 else 0
    try:
        fate, bar, _, bases = barcode_rule.fates(bars, text)[-1]
        want.update(last=0, bar=bar, kept=int(fate == barcode_rule.KEPT), bases=bases)
    except barcode_rule.Refused as r:
        want["last"] = STATUS[r.status]
    return want


def test_host_text_code_under_asan_and_ubsan():
    if not shutil.which("g++"):
        pytest.skip("no g++")
    p = subprocess.run(["make", "-C", HERE, "-f", "barcode.mk", "asan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-3000:]
    assert "Sanitizer" not in out and "runtime error" not in out
    seen = 0
    for line in out.split("\n"):
        words = line.split(" ")
        if len(words) < 2 or not words[1].startswith("parse="):
            continue
        got = {k: int(v) for k, v in (w.split("=") for w in words[1:])}
        want = expected(words[0])
        for k, v in want.items():
            assert got[k] == v, (words[0], k, got, want)
        seen += 1
    assert seen >= 50
