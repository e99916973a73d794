"""GPU: what a plain `bench.py` run prints, and what `--full` adds to it, on a reduced workload (200 000 reads per step
against a 30 Mbp database)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--reads", "200000", "--n-seq", "20000"]


def _bench_line(extra, timeout):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _roofs(j):
    """The seed stage's and the gapped stage's roofline objects, whichever of them is the line's `roofline`."""
    r = j["roofline"]
    if "gapped" in r:
        return r, r["gapped"]
    return r["seed_extend"], r


def test_plain_run_prints_the_headline_and_nothing_that_takes_a_run_of_its_own():
    j = _bench_line([], 600)
    assert j["unit"] == "reads/s" and j["higher_is_better"] is True and j["steps"] == 2 and j["warmup"] == 1
    assert j["value"] > 0 and j["value"] == pytest.approx(200000 * 1e3 / j["ms_per_step"], rel=1e-9)
    assert j["dust_at_import_only"] is None and j["cpu_baseline"] is None and "inclusive" not in j
    seed, gap = _roofs(j)
    assert seed["achieved"] > 0 and gap["achieved"] > 0
    assert seed["random_line_roof"] is None and gap["random_line_roof"] is None and gap["issue"] is None


def test_full_run_adds_the_side_lines_the_measured_roofs_and_the_baselines():
    j = _bench_line(["--full", "--cpu-sample", "2000", "--inclusive-sample", "20000"], 900)
    assert j["value"] > 0 and j["ms_per_step"] > 0
    assert j["dust_at_import_only"]["value"] > 0 and j["dust_at_import_only"]["ms_per_step"] > 0
    assert "error" not in j["inclusive"] and j["inclusive"]["value"] > 0 and j["inclusive"]["first_pass"]["value"] > 0
    assert j["cpu_baseline"]["kind"] == "port" and j["cpu_baseline"]["value"] > 0
    seed, gap = _roofs(j)
    assert seed["random_line_roof"]["roof_lines_per_s"] > 0
    assert gap["issue"]["roof_fast_kind_per_s_per_simd"] > 0 and gap["issue"]["roof_other_kinds_per_s_per_simd"] > 0
