"""pgx_trim_reads (Reads.from_trim): trim2 handed straight to Classify as a resident batch.  The yardstick in every test is the
two-call form at the same build's unchanged path -- pg.trim2, then Reads.from_fasta_text on the FASTA it returns -- never
the new call against itself.  "Equal batch": same length, same letters read by read, byte-equal write_fasta files (names
and ambiguity letters), same DUST `any` and word offsets, the three DUST word arrays equal on the reads with any == 1 (the
header leaves the others' words undefined), and trim2's messages and mode.  The route is asserted wherever the input
decides it, so that no test passes by always falling back to the text route."""
import os
import random

import numpy as np
import pytest

from trim_inputs import fastq_text, qseq_text, random_case

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


def both_forms(pg, tmp_path, a, b=None, **opts):
    """The two-call form and the new call on the same files.  Returns (want reads, got reads, route), or the status both
    raised.  Asserts that messages, mode and status agree."""
    pa = tmp_path / "a.txt"
    pa.write_bytes(a)
    pb = None
    if b is not None:
        pb = tmp_path / "b.txt"
        pb.write_bytes(b)
    args = (str(pa), None if pb is None else str(pb))
    try:
        messages, fasta, mode = pg.trim2(*args, **opts)
    except pg.PangeaError as e:
        with pytest.raises(pg.PangeaError) as e2:
            pg.Reads.from_trim(*args, **opts)
        assert e2.value.status == e.status
        return e.status
    got, got_messages, got_mode, route = pg.Reads.from_trim(*args, **opts)
    assert (got_messages, got_mode) == (messages, mode)
    if fasta is None:
        assert got is None and route == pg.TRIM_ROUTE_NONE
        return None, None, route
    assert got is not None and route in (pg.TRIM_ROUTE_PACKED, pg.TRIM_ROUTE_TEXT)
    return pg.Reads.from_fasta_text(fasta), got, route


def assert_equal_batch(want, got, tmp_path):
    n = len(want)
    assert len(got) == n
    lens = np.zeros(n, dtype=np.int64)
    for i in range(n):
        w = want.get(i)
        assert np.array_equal(got.get(i), w), i
        lens[i] = len(w)
    want.write_fasta(str(tmp_path / "want.fa"))
    got.write_fasta(str(tmp_path / "got.fa"))
    assert (tmp_path / "got.fa").read_bytes() == (tmp_path / "want.fa").read_bytes()
    w_any, w_off, *w_words = want.dust_bits()
    g_any, g_off, *g_words = got.dust_bits()
    assert np.array_equal(g_any, w_any) and np.array_equal(g_off, w_off)
    for i in np.flatnonzero(w_any):
        lo, hi = int(w_off[i]), int(w_off[i]) + (int(lens[i]) + 63) // 64
        for ww, gw in zip(w_words, g_words):
            assert np.array_equal(gw[lo:hi], ww[lo:hi]), i


def check(pg, tmp_path, route, a, b=None, **opts):
    """Equal batch, and the route (None: either).  Returns (want, got, route taken)."""
    want, got, took = both_forms(pg, tmp_path, a, b, **opts)
    assert_equal_batch(want, got, tmp_path)
    if route is not None:
        assert took == route
    return want, got, took


# ---------------------------------------------------------------------------------------------------- 1. FASTQ, single
@pytest.mark.parametrize("n_records", [0, 1, 700])
def test_fastq_single(pg, tmp_path, n_records):
    """Lengths 20..160 straddle the length cutoff (the one-letter "0" read) and the 32- and 64-base word edges, every 17th
    read holds N; 700 records are more than one block of the measure kernel and several lane groups.  The empty file is no
    FASTQ to the script (format not recognised): the empty batch, made of the empty text."""
    a = fastq_text(11, n_records, 20, 160)
    want, got, route = check(pg, tmp_path, pg.TRIM_ROUTE_PACKED if n_records else pg.TRIM_ROUTE_TEXT, a)
    assert len(got) == n_records
    if n_records == 700:
        lens = [len(got.get(i)) for i in range(700)]
        assert 1 in lens and max(lens) > 128 and any(4 in got.get(i) for i in range(0, 700, 17))


# ---------------------------------------------------------------------------------------------------- 2. FASTQ -b "", -g
@pytest.mark.parametrize("g", [None, "7", "100", "2.5"])
def test_fastq_interleaved(pg, tmp_path, g):
    want, got, _ = check(pg, tmp_path, pg.TRIM_ROUTE_PACKED, fastq_text(12, 700, 20, 160), b"", g=g)
    assert len(got) == 350


def test_fastq_interleaved_pieces_search_alike(pg, tmp_path):
    """-g 100: the mates are joined by 100 N's, so the batch is searched as pieces.  Mates cut from the subjects of a small
    database: both batches must give the same hit table, the same offsets and the same -outfmt 6 text, and it is not empty."""
    from pangea_plus_amd import _capi
    rng = random.Random(21)
    subjects = ["".join(rng.choice("ACGT") for _ in range(600)) for _ in range(40)]
    (tmp_path / "db.fa").write_text("".join(">gi|%d|x|s%d|\n%s\n" % (i + 1, i, s) for i, s in enumerate(subjects)))
    db = pg.Db.from_fasta(str(tmp_path / "db.fa"))
    out = []
    for i in range(600):      # 300 pairs, interleaved
        L = rng.randint(120, 150)
        src = rng.choice(subjects)
        off = rng.randrange(0, 600 - L + 1)
        seq = list(src[off:off + L])
        for p in rng.sample(range(L), rng.randint(0, 4)):
            seq[p] = rng.choice([c for c in "ACGT" if c != seq[p]])
        out.append("@P%d/%d\n%s\n+\n%s\n" % (i // 2, i % 2 + 1, "".join(seq), "I" * L))
    want, got, _ = check(pg, tmp_path, pg.TRIM_ROUTE_PACKED, "".join(out).encode(), b"", g="100")
    assert len(got) == 300
    want_hits, got_hits = _capi.blast_search(db, want), _capi.blast_search(db, got)
    assert len(want_hits) > 0
    assert np.array_equal(got_hits.to_numpy(), want_hits.to_numpy())
    assert np.array_equal(got_hits.read_offsets(300), want_hits.read_offsets(300))
    text = want_hits.format(db, want)
    assert got_hits.format(db, got) == text and text.count(b"\n") > 300


# ---------------------------------------------------------------------------------------------------- 3. QSEQ pairs
@pytest.mark.parametrize("t", [None, "5", "30"])
def test_qseq_pairs(pg, tmp_path, t):
    """Dots become N, a pair with a short mate is absent, reads pass 192 and 320 bases (the other flag-word classes)."""
    a, b = qseq_text(13, 600, 10, 300)
    want, got, _ = check(pg, tmp_path, pg.TRIM_ROUTE_PACKED, a, b, g="100", t=t)
    lens = [len(got.get(i)) for i in range(len(got))]
    assert 0 < len(got) < 600 and min(lens) >= 240 and max(lens) > 320 and any(x <= 320 for x in lens)


# ---------------------------------------------------------------------------------------------------- 4. irregular records
def _fq(records):
    return "".join("@%s\n%s\n+\n%s\n" % r for r in records).encode("latin-1")


def _qs(name, mate, seq, qual):
    return "\t".join(["HWI-X", "12", "1", "1101", name, "77", "TTAGGC", str(mate), seq, qual, "1"]) + "\n"


GOOD = "ACGT" * 25


def irregular_cases():
    ok = [("r%d x" % i, GOOD, "I" * 100) for i in range(5)]
    h = "h" * 100     # QSEQ quality offset 64
    qa = [_qs("n%d" % i, 1, GOOD, h) for i in range(4)]
    qb = [_qs("n%d" % i, 2, GOOD, h) for i in range(4)]
    yield "fastq sequence line begins with '>'", _fq(ok[:2] + [("odd", ">" + GOOD, "I" * 101)] + ok[2:]), None, {}
    yield "fastq interleaved, CRLF", _fq(ok + ok[:1]).replace(b"\n", b"\r\n"), b"", {"g": "7"}
    yield ("fastq second mate keeps its line end (quality line longer than the sequence line)",
           _fq(ok[:3] + [("long", GOOD, "I" * 140)] + ok[:2]), b"", {"g": "3"})
    yield ("fastq second mate holds a carriage return",
           _fq(ok[:1] + [("cr", GOOD[:50] + "\r" + GOOD[50:], "I" * 101)]), b"", {"g": "3"})
    yield ("fastq without N's between the mates (-g abc), first mate all blanks, second begins with '>'",
           _fq([("b", " " * 80, "I" * 80), ("c", ">" + GOOD, "I" * 101)] + ok[:2]), b"", {"g": "abc"})
    yield ("qseq base field begins with '>'",
           "".join(qa[:2] + [_qs("odd", 1, "A>" + GOOD, "h" * 102)] + qa[2:]).encode(),     # -t 1 cuts the A off
           "".join(qb[:2] + [_qs("odd", 2, GOOD, h)] + qb[2:]).encode(), {"g": "10", "t": "1"})
    yield ("qseq short line ends in a carriage return (the header takes it)",
           (qa[0] + "HWI-X\t12\t1\r\n" + qa[1]).encode(),
           (qb[0] + _qs("x", 2, GOOD, h) + qb[1]).encode(), {"g": "10"})


@pytest.mark.parametrize("what,a,b,opts", list(irregular_cases()), ids=[c[0] for c in irregular_cases()])
def test_irregular_records_take_the_text_route(pg, tmp_path, what, a, b, opts):
    want, got, _ = check(pg, tmp_path, pg.TRIM_ROUTE_TEXT, a, b, **opts)
    assert len(got) > 0


def text_route_at_size():
    fq = fastq_text(12, 700, 20, 160) + _fq([("odd", ">" + GOOD, "I" * 101)])
    yield "fastq interleaved, 351 records", fq, b"", {"g": "7"}, 300
    a, b = qseq_text(13, 600, 10, 300)
    yield "qseq, 601 pairs", a + b"HWI-X\t12\t1\r\n", b + _qs("x", 2, GOOD, "h" * 100).encode(), {"g": "100"}, 0


@pytest.mark.parametrize("what,a,b,opts,more_than", list(text_route_at_size()), ids=[c[0] for c in text_route_at_size()])
def test_the_text_route_past_one_block(pg, tmp_path, what, a, b, opts, more_than):
    """The inputs of test_fastq_interleaved and test_qseq_pairs with one irregular record behind them (a sequence line that
    begins with '>'; a short -a line that ends in a carriage return): the text route with more records than one block of a
    measure kernel (256) or of a writer (16 lane groups) takes, where the raw text and the columns are let go before the
    FASTA is split.  The oracle prints 351 records for the FASTQ input."""
    want, got, _ = check(pg, tmp_path, pg.TRIM_ROUTE_TEXT, a, b, **opts)
    assert len(got) > more_than


def test_the_regular_twins_take_the_packed_route(pg, tmp_path):
    """The same shapes without the one odd record or byte: packed.  (Blanks and tabs inside a kept span, a '>' that is not
    the first byte of the line, a header with '@' and without a blank are all regular.)"""
    recs = [("r%d x" % i, GOOD, "I" * 100) for i in range(5)]
    recs += [("a@b@c", GOOD[:40] + " \t" + GOOD[40:] + ">", "I" * 104), ("tab\there", "A>" + GOOD, "I" * 103)]
    check(pg, tmp_path, pg.TRIM_ROUTE_PACKED, _fq(recs))
    check(pg, tmp_path, pg.TRIM_ROUTE_PACKED, _fq(recs + recs[:1]), b"", g="3")
    h = "h" * 100
    a = "".join(_qs("n %d" % i, 1, GOOD[:30] + " " + GOOD[30:] + ("" if i else ">"), h + "h" * 10) for i in range(4))
    b = "".join(_qs("n %d" % i, 2, GOOD, h) for i in range(4))
    check(pg, tmp_path, pg.TRIM_ROUTE_PACKED, (a + "HWI-X\t12\t1\n").encode(), (b + _qs("x", 2, GOOD, h)).encode(), g="10", t="1")


# ---------------------------------------------------------------------------------------------------- 5. damaged files
SEEDS = [int(x) for x in os.environ.get("PGX_TRIM_READS_SEEDS",
                                        "101,102,103,104,105,106,107,108,109,110,111,112,113,114,115,116,117,118,119,120,121,122,123,124").split(",")]
ROUTES = {}


@pytest.mark.parametrize("seed", SEEDS)
def test_random_damaged_files(pg, tmp_path, seed):
    a, b, g, t = random_case(seed, 60, 60)
    res = both_forms(pg, tmp_path, a, b, g=g, t=t)
    if isinstance(res, tuple):
        want, got, route = res
        assert_equal_batch(want, got, tmp_path)
        ROUTES[seed] = route
    else:
        ROUTES[seed] = "status %d" % res


def test_random_damaged_files_took_both_routes(pg):
    """Runs behind the seeds above: the list holds inputs of both kinds."""
    assert sorted(ROUTES) == sorted(SEEDS)
    took = list(ROUTES.values())
    print("routes:", ROUTES)
    assert took.count(pg.TRIM_ROUTE_PACKED) >= 1 and took.count(pg.TRIM_ROUTE_TEXT) >= 1


def test_negative_truncate_is_declined_alike(pg, tmp_path):
    assert both_forms(pg, tmp_path, fastq_text(3, 4, 80, 90), None, t="-3") == -1


# ---------------------------------------------------------------------------------------------------- 6. -j: join_fasta
def test_fasta_join_takes_the_text_route(pg, tmp_path):
    rng = random.Random(5)

    def fasta(tag, n):
        out = []
        for i in range(n):
            s = "".join(rng.choice("ACGTN") if i % 5 == 0 else rng.choice("ACGT") for _ in range(rng.randint(30, 200)))
            out.append(">%s%d len\n" % (tag, i) + "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60)))
        return "".join(out).encode()
    want, got, _ = check(pg, tmp_path, pg.TRIM_ROUTE_TEXT, fasta("a", 40), fasta("b", 40), g="25", j=True)
    assert len(got) >= 39
    # and the file of the reference's own run of that mode
    a, b = (open(os.path.join(GOLD, "trim_fasta", "jf_multi_line_records.%s.txt" % x), "rb").read() for x in "ab")
    check(pg, tmp_path, pg.TRIM_ROUTE_TEXT, a, b, g="25", j=True)


def test_fasta_with_quality_file_gives_the_empty_batch(pg, tmp_path):
    (tmp_path / "q.txt").write_text(">s0 x\n30 30 30 30\n>s1 x\n30 30 30 30\n")
    a = b">s0 x\nACGT\n>s1 x\nACGT\n"
    want, got, route = both_forms(pg, tmp_path, a, None, q=str(tmp_path / "q.txt"))
    assert len(want) == 0 and len(got) == 0 and route == pg.TRIM_ROUTE_TEXT
    (tmp_path / "a.txt").write_bytes(a)
    assert pg.Reads.from_trim(str(tmp_path / "a.txt"), q=str(tmp_path / "q.txt"))[2] == pg._capi.TRIM_FASTA_QUAL
    # an unopenable -a: no FASTA, no batch
    assert both_forms(pg, tmp_path, b"") is not None
    got, messages, mode, route = pg.Reads.from_trim(str(tmp_path / "missing.txt"))
    assert got is None and route == pg.TRIM_ROUTE_NONE and messages.startswith(b"Error: Unable to open")
