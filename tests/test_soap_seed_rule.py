"""tests/soap_seed_rule.py against the closed soap ELF's seed-mode rows (tests/golden/soap_seed, made by
tools/gen_goldens_soap_seed.py): rows as sets per read, the unmapped files byte for byte.  No device needed."""
import gzip
import os

import pytest

import soap_seed_rule as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = os.path.join(GOLD, "soap_seed")

# golden run -> (reads file, soap_single keywords)
CASES = {
    "l32v5": ("reads.fa", dict(l=32, v=5, r=2)),
    "l64": ("reads.fa", dict(l=64, r=2)),
    "l32v2": ("reads.fa", dict(l=32, v=2, r=2)),
    "l32v20": ("reads.fa", dict(l=32, v=20, r=2)),
    "l32v5_r0": ("reads.fa", dict(l=32, v=5, r=0)),
    "l32_M0": ("reads.fa", dict(l=32, M=0, r=2)),
    "l32_M1": ("reads.fa", dict(l=32, M=1, r=2)),
    "l32_M2": ("reads.fa", dict(l=32, M=2, r=2)),
    "l32v5_t": ("reads.fa", dict(l=32, v=5, r=2, t=True)),
    "g3": ("reads.fa", dict(r=2)),            # -g 3: no gapped rows on these reads, the plain run's rows
    "s40": ("reads.fa", dict(r=2)),           # -s 40: nothing clipped, the plain run's rows
    "sweep_l32v5": ("sweep.fa", dict(l=32, v=5, r=2)),
    "sweep_l64v3": ("sweep.fa", dict(l=64, v=3, r=2)),
    "long_l256v5": ("long.fa", dict(l=256, v=5, r=2)),
}


@pytest.fixture(scope="module")
def ref():
    return R.load_ref(os.path.join(GOLD, "soap", "ref.fa"))


def reads_path(name):
    return os.path.join(GOLD, "soap", name) if name == "reads.fa" else os.path.join(SEED, name)


def golden(name):
    return gzip.open(os.path.join(SEED, name), "rb").read().decode()


@pytest.mark.parametrize("tag", sorted(CASES))
def test_rule_reproduces_the_reference_binary(ref, tag):
    reads, kw = CASES[tag]
    out, unm = R.soap_single(ref, R.load_reads(reads_path(reads)), **kw)
    want = R.rows_by_read(golden("out_%s.txt.gz" % tag))
    assert R.rows_by_read(out) == want and len(want) > 20
    assert unm == golden("unmapped_%s.txt.gz" % tag)


def test_rule_r1_picks_one_of_the_reference_rows(ref):
    """-r 1 prints "a random one" (soap.man): the column-4 counts agree everywhere, a unique placement's row exactly"""
    out, unm = R.soap_single(ref, R.load_reads(reads_path("reads.fa")), l=32, v=5, r=1)
    want = golden("out_l32v5_r1.txt.gz").splitlines()
    got = out.splitlines()
    assert len(want) == len(got) == 407
    for a, b in zip(want, got):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[0] == fb[0] and fa[3] == fb[3]
        if fa[3] == "1":
            assert a == b
    assert unm == golden("unmapped_l32v5_r1.txt.gz")


def test_long_reads_default_is_a_256_base_seed():
    """the ELF without options places reads over 256 bases as with -l 256 -v 5 (soap.man:59-72 defaults)"""
    assert golden("out_long_default.txt.gz") == golden("out_long_l256v5.txt.gz")
    assert golden("unmapped_long_default.txt.gz") == golden("unmapped_long_l256v5.txt.gz")


def test_seed_changes_the_rows(ref):
    """a seeded run differs from a plain one on the golden reads (609 rows without -l / -v, 686 with -l 32 -v 5)"""
    reads = R.load_reads(reads_path("reads.fa"))
    plain, _ = R.soap_single(ref, reads, r=2)
    seeded, _ = R.soap_single(ref, reads, l=32, v=5, r=2)
    assert plain.count("\n") == 609 and seeded.count("\n") == 686


@pytest.mark.parametrize("l", [16, 20, 26, 150, 151, 300])
def test_seed_outside_its_range_is_a_plain_run(ref, l):
    """-l under 27, or not shorter than the read: the read is placed whole (the 150-base reads of the golden set)"""
    reads = [x for x in R.load_reads(reads_path("reads.fa")) if len(x[1]) == 150]
    assert R.soap_single(ref, reads, r=2, l=l, v=5)[0] == R.soap_single(ref, reads, r=2)[0]
