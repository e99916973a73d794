"""GPU parity, SOAP verb with a seed (`-l` / `-v`, soap.man:59-72): the HIP path against the rows the reference's closed
soap ELF printed (tests/golden/soap_seed, sets per read; the unmapped files byte for byte) and, on fuzzed reads, against
the rule restated in tests/soap_seed_rule.py."""
import gzip
import os
import random
import subprocess

import pytest

import soap_seed_rule as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pangea-plus_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
SEED = os.path.join(GOLD, "soap_seed")

# golden run -> (reads file, command-line options)
CASES = {
    "l32v5": ("reads.fa", "-l 32 -v 5 -r 2"),
    "l64": ("reads.fa", "-l 64 -r 2"),
    "l32v2": ("reads.fa", "-l 32 -v 2 -r 2"),
    "l32v20": ("reads.fa", "-l 32 -v 20 -r 2"),
    "l32v5_r0": ("reads.fa", "-l 32 -v 5 -r 0"),
    "l32_M0": ("reads.fa", "-l 32 -M 0 -r 2"),
    "l32_M1": ("reads.fa", "-l 32 -M 1 -r 2"),
    "l32_M2": ("reads.fa", "-l 32 -M 2 -r 2"),
    "l32v5_t": ("reads.fa", "-l 32 -v 5 -r 2 -t"),
    "g3": ("reads.fa", "-g 3 -r 2"),
    "s40": ("reads.fa", "-s 40 -r 2"),
    "sweep_l32v5": ("sweep.fa", "-l 32 -v 5 -r 2"),
    "sweep_l64v3": ("sweep.fa", "-l 64 -v 3 -r 2"),
}


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


@pytest.fixture(scope="module")
def index(pg, tmp_path_factory):
    d = tmp_path_factory.mktemp("soap_seed")
    ref = d / "ref.fa"
    ref.write_bytes(open(os.path.join(GOLD, "soap", "ref.fa"), "rb").read())
    pg.soap_index(str(ref))
    return str(ref)


def reads_path(name):
    return os.path.join(GOLD, "soap", name) if name == "reads.fa" else os.path.join(SEED, name)


def golden(name):
    return gzip.open(os.path.join(SEED, name), "rb").read()


def soap_cli(index, reads, opts, tmp_path, tag="x"):
    out, unm = tmp_path / ("%s.txt" % tag), tmp_path / ("%s.unm" % tag)
    p = subprocess.run([os.path.join(BIN, "soap"), "-a", reads, "-D", index + ".index", "-o", str(out), "-u", str(unm), "-p", "8"]
                       + opts.split(), stderr=subprocess.PIPE, timeout=300)
    return p, out, unm


def test_l32_v5_equals_the_reference_binary(index, tmp_path):
    """the issue's case: 686 rows (a run that ignores -l / -v prints 609)"""
    p, out, unm = soap_cli(index, reads_path("reads.fa"), "-l 32 -v 5 -r 2", tmp_path)
    assert p.returncode == 0, p.stderr
    assert sum(1 for _ in open(out)) == 686
    assert R.rows_by_read(out.read_text()) == R.rows_by_read(golden("out_l32v5.txt.gz").decode())
    assert unm.read_bytes() == golden("unmapped_l32v5.txt.gz")


@pytest.mark.parametrize("tag", sorted(CASES))
def test_cli_equals_the_reference_binary(index, tmp_path, tag):
    reads, opts = CASES[tag]
    p, out, unm = soap_cli(index, reads_path(reads), opts, tmp_path)
    assert p.returncode == 0, p.stderr
    assert R.rows_by_read(out.read_text()) == R.rows_by_read(golden("out_%s.txt.gz" % tag).decode())
    assert unm.read_bytes() == golden("unmapped_%s.txt.gz" % tag)


def test_r1_counts_and_unique_rows_equal_the_reference_binary(index, tmp_path):
    """-r 1: "a random one" (soap.man); the column-4 counts agree everywhere, a unique placement's row byte for byte"""
    p, out, unm = soap_cli(index, reads_path("reads.fa"), "-l 32 -v 5 -r 1", tmp_path)
    assert p.returncode == 0, p.stderr
    want = golden("out_l32v5_r1.txt.gz").decode().splitlines()
    got = out.read_text().splitlines()
    assert len(want) == len(got) == 407
    for a, b in zip(want, got):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[0] == fb[0] and fa[3] == fb[3]
        if fa[3] == "1":
            assert a == b
    assert unm.read_bytes() == golden("unmapped_l32v5_r1.txt.gz")


def test_long_reads_with_a_256_base_seed_equal_the_reference_default(pg, index, tmp_path):
    """reads of 257-600 bases: `l=256, v=5` gives the rows the ELF prints without options"""
    out, unm = tmp_path / "o.txt", tmp_path / "u.txt"
    pg.soap(os.path.join(SEED, "long.fa"), index + ".index", str(out), u=str(unm), r=2, l=256, v=5)
    assert R.rows_by_read(out.read_text()) == R.rows_by_read(golden("out_long_default.txt.gz").decode())
    assert unm.read_bytes() == golden("unmapped_long_default.txt.gz")
    # -M 0 / 1 / 2 on reads over 256 bases: valid with a seed
    for m in (0, 1, 2):
        pg.soap(os.path.join(SEED, "long.fa"), index + ".index", str(out), u=str(unm), M=m, r=2, l=256)


def _fuzz_reads(seed, ref):
    rng = random.Random(seed)
    seqs = [ref.base[ref.off[i]:ref.off[i + 1]] for i in range(len(ref.ids))]
    reads = []
    for k in range(160):
        L = rng.choice([27, 30, 33, 40, 47, 48, 60, 100, 150, 255, 256, 257, 300, 450, 600])
        s = rng.choice([x for x in seqs if len(x) > L + 2])
        o = rng.randrange(0, len(s) - L)
        w = [int(b) for b in s[o:o + L]]
        for p in rng.sample(range(L), rng.choice([0, 1, 2, 3, 3, 4, 5, 6, 8, 12])):
            w[p] = (w[p] + rng.randrange(1, 4)) & 3
        if rng.random() < 0.5:
            w = [3 - b for b in reversed(w)]
        reads.append(("f%d_%d" % (seed, k), "".join("ACGT"[b] for b in w)))
    return reads


@pytest.mark.parametrize("seed,l,v,M", [(1, 32, 5, 4), (2, 27, 3, 4), (3, 48, 8, 4), (4, 64, 0, 4), (5, 100, 20, 4),
                                        (6, 256, 5, 4), (7, 32, 5, 1), (8, 40, 2, 2), (9, 33, 30, 0)])
def test_fuzzed_reads_equal_the_rule(pg, index, tmp_path, seed, l, v, M):
    ref = R.load_ref(index)
    fa = tmp_path / "fuzz.fa"
    fa.write_text("".join(">%s\n%s\n" % x for x in _fuzz_reads(seed, ref)))
    out, unm = tmp_path / "o.txt", tmp_path / "u.txt"
    pg.soap(str(fa), index + ".index", str(out), u=str(unm), M=M, r=2, l=l, v=v)
    want_out, want_unm = R.soap_single(ref, R.load_reads(str(fa)), M=M, r=2, l=l, v=v)
    assert R.rows_by_read(out.read_text()) == R.rows_by_read(want_out)
    assert unm.read_text() == want_unm


def test_without_l_or_v_the_cli_is_the_plain_run(pg, index, tmp_path):
    """no -l / -v: the executable's bytes are those of pgx_soap_run"""
    p, out, unm = soap_cli(index, reads_path("reads.fa"), "-r 2 -M 4", tmp_path)
    assert p.returncode == 0, p.stderr
    o2, u2 = tmp_path / "api.txt", tmp_path / "api.unm"
    pg.soap(reads_path("reads.fa"), index + ".index", str(o2), u=str(u2), r=2)
    assert out.read_bytes() == o2.read_bytes() and unm.read_bytes() == u2.read_bytes()
    assert sum(1 for _ in open(out)) == 609


def test_paired_end_with_a_seed_is_refused(index, tmp_path):
    g = os.path.join(GOLD, "soap")
    for opt in ("-l 32", "-v 5"):
        p, out, unm = soap_cli(index, os.path.join(g, "pe_a.fa"), "-b %s -2 %s %s" % (os.path.join(g, "pe_b.fa"), tmp_path / "u2", opt),
                               tmp_path)
        assert p.returncode == 2 and b"single-end" in p.stderr
