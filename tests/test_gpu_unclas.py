"""GPU parity of the unclassified-read selector (Unclas_Sel/unclassified_selector.pl).

File verb: every golden case printed by the reference's Perl through pgx_unclas_file and through the CLI binary.
Resident form: pgx_unclassified_batch against tests/unclas_rule.py and against the file verb, both run on the texts of the
same table and batch (pgx_hits_format, pgx_reads_write_fasta), and the subset batch against the batch
pgx_reads_from_fasta_text makes of the verb's output.

The database is hand-made so that every kind of read the row pass can meet is in the 3 000-read batch, and
`test_the_batch_holds_every_kind` asserts each from the table itself.  The read that S3c takes a slot from is a window with
one base deleted (seeds on both sides of the gap grow into one alignment), the construction tests/test_gpu_order_single_pass.py
uses for the same purpose.
"""
import os

import numpy as np
import pytest

import unclas_rule
from pangea_plus_amd import _capi
from conftest import ROOT, run_cmd
from test_unclas_rule import cases, load_case

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "pangea-plus_amd", "bin", "unclassified_selector")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
OTHER = bytes.maketrans(b"ACGT", b"CATG")  # a different letter at every position
MIXES = [{}, {"t": "100", "b": "0", "e": "5"}, {"t": "0", "b": "0", "e": "700"}, {"b": "1e9"}]
SIZES = [0, 1, 63, 64, 65, 3000]


# ------------------------------------------------------------------------------------------ file verb
@pytest.mark.parametrize("name", cases())
def test_file_verb_and_cli_match_the_reference_script(name, tmp_path):
    import pangea_plus_amd as pg
    pg.init(0)
    for how in ("verb", "cli"):
        work = tmp_path / how
        work.mkdir()
        argv, stdout, status, out = load_case(name, work)
        if how == "verb":
            try:
                got_stdout, got_status = pg.unclassified_selector(argv, cwd=str(work)), 0
            except pg.PangeaError as e:
                assert e.status == -2
                got_stdout, got_status = e.stdout, 2
        else:
            got_status, got_stdout, _ = run_cmd([BIN] + argv, cwd=str(work))
        made = work / "out.fas"
        assert got_stdout == stdout
        assert got_status == status
        assert (made.read_bytes() if made.exists() else None) == out


# ------------------------------------------------------------------------------------------ resident form: inputs
def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def _subst(rng, s, k):
    s = bytearray(s)
    for p in rng.choice(len(s), k, replace=False):
        s[p] = rng.choice([c for c in b"ACGT" if c != s[p]])
    return bytes(s)


def make_inputs(rng):
    """(subjects, reads): reads are (kind, sequence); the hand-made ones come first, so every prefix batch holds some."""
    bg = [_rand(rng, 500) for _ in range(250)]
    anc = _rand(rng, 400)
    fam = [_subst(rng, anc, 1 + j % 3) for j in range(70)]
    a = _rand(rng, 500)
    two = bytearray(a[100:250])       # lies in A with one mismatch; its first 60 bases lie exactly in B, whose next 20
    two[100] = OTHER[two[100]]        # letters differ from the read's at every position (the alignment ends there)
    two = bytes(two)
    b = _rand(rng, 200) + two[:60] + two[60:80].translate(OTHER) + _rand(rng, 180)
    subjects = bg + fam + [a, b]

    def window(k=0, s=None, L=150):
        s = bg[rng.randint(len(bg))] if s is None else s
        st = rng.randint(0, len(s) - L + 1)
        w = _subst(rng, s[st:st + L], k)
        return w.translate(COMP)[::-1] if rng.randint(2) else w

    reads = [("exact", window())]
    reads.append(("row2", two))
    reads.append(("indel", bg[3][20:95] + bg[3][96:171]))
    reads.append(("many", fam[5][100:250]))
    reads.append(("short_score", bg[7][40:140] + _rand(rng, 50)))  # pident 100 over 100 bases: the score alone fails
    reads.append(("low_pident", window(10, bg[9])))
    reads.append(("none", _rand(rng, 150)))
    kinds = [("sub", 0), ("sub", 3), ("sub", 6), ("sub", 10), ("sub", 15), ("none", None), ("short_score", None), ("many", None)]
    weight = [0.2, 0.15, 0.1, 0.15, 0.1, 0.2, 0.07, 0.03]
    while len(reads) < SIZES[-1]:
        kind, k = kinds[rng.choice(len(kinds), p=weight)]
        if kind == "sub":
            reads.append(("sub%d" % k, window(k)))
        elif kind == "none":
            reads.append(("none", _rand(rng, 150)))
        elif kind == "short_score":
            reads.append((kind, window(0, L=100) + _rand(rng, 50)))
        else:
            reads.append((kind, window(rng.randint(3), fam[rng.randint(70)])))
    return subjects, reads


def fasta_text(names, seqs):
    return b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(names, seqs))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import pangea_plus_amd as pg
    pg.init(0)
    d = tmp_path_factory.mktemp("unclas")
    rng = np.random.RandomState(20261017)
    subjects, reads = make_inputs(rng)
    (d / "db.fa").write_bytes(b"".join(b">gi|%d|s%d|\n%s\n" % (1000 + i, i, s) for i, s in enumerate(subjects)))
    db = pg.Db.from_fasta(str(d / "db.fa"))
    return pg, d, db, reads, rng


class Case:
    """A batch, its table and the two texts the definition speaks of; made once per batch, never changed."""

    def __init__(self, pg, db, d, tag, fasta):
        self.pg, self.db, self.d, self.tag = pg, db, d, tag
        self.reads = pg.Reads.from_fasta_text(fasta)
        self.n = len(self.reads)
        self.hits = _capi.blast_search(db, self.reads)
        self.table = self.hits.format(db, self.reads)
        self.m_path, self.s_path = str(d / (tag + ".m.tsv")), str(d / (tag + ".s.fas"))
        open(self.m_path, "wb").write(self.table)
        self.reads.write_fasta(self.s_path)
        self.fasta = open(self.s_path, "rb").read()
        self.counts = self.hits.read_counts(self.n)
        lines = self.table.split(b"\n")[:-1]
        assert len(lines) == int(self.counts.sum())
        ends = np.cumsum(self.counts)
        self.rows = [lines[e - c:e] for c, e in zip(self.counts, ends)]  # the rows of every read, in order


def subset_checks(case, opts):
    """The three checks of the definition for one option mix; returns the mask."""
    pg, db = case.pg, case.db
    t, e, b = unclas_rule.thresholds(opts.get("t"), opts.get("e"), opts.get("b"))
    want = np.array(unclas_rule.keep_mask(case.table, case.fasta, t, e, b), dtype=np.uint8)
    mask, out = pg.unclassified(db, case.reads, case.hits, **opts)
    assert len(want) == case.n
    assert np.array_equal(mask, want)                                     # 1: the rule on the two texts
    argv = ["-m", case.m_path, "-s", case.s_path, "-o", str(case.d / (case.tag + ".out.fas"))]
    for k, v in opts.items():
        argv += ["-" + k, v]
    log = pg.unclassified_selector(argv)
    verb_out = (case.d / (case.tag + ".out.fas")).read_bytes()
    text, count = unclas_rule.select(case.table, case.fasta, t, e, b)
    assert verb_out == text                                               # 2: the file verb on the two texts
    assert log.endswith(b"Rejected %d sequence(s).\nFinished!\n" % count) and count == int(mask.sum())
    ref = pg.Reads.from_fasta_text(verb_out)                              # 3: the subset batch
    assert len(out) == len(ref) == count
    out_path, ref_path = str(case.d / "sub.out.fas"), str(case.d / "sub.ref.fas")
    out.write_fasta(out_path)
    ref.write_fasta(ref_path)
    assert open(out_path, "rb").read() == open(ref_path, "rb").read()     # names and letters
    for i in range(count):
        assert np.array_equal(out.get(i), ref.get(i))
    any_o, woff_o, *bits_o = out.dust_bits()
    any_r, woff_r, *bits_r = ref.dust_bits()
    assert np.array_equal(any_o, any_r) and np.array_equal(woff_o, woff_r)
    for i in np.nonzero(any_r)[0]:
        lo, hi = woff_r[i], woff_r[i] + (len(ref.get(int(i))) + 63) // 64
        for x, y in zip(bits_o, bits_r):
            assert np.array_equal(x[lo:hi], y[lo:hi])
    again = _capi.blast_search(db, out).format(db, out)
    assert again == b"".join(r + b"\n" for i in np.nonzero(mask)[0] for r in case.rows[i])
    return mask


@pytest.fixture(scope="module")
def batches(world):
    pg, d, db, reads, rng = world
    out = {}
    for n in SIZES:
        out[n] = Case(pg, db, d, "b%d" % n, fasta_text([b"q%d" % i for i in range(n)], [s for _, s in reads[:n]]))
    return out


def row_fields(row):
    f = row.split(b"\t")
    return float(f[2]), float(f[10]), float(f[11])


def test_the_batch_holds_every_kind(world, batches):
    pg, d, db, reads, rng = world
    case = batches[SIZES[-1]]
    kinds = [k for k, _ in reads]
    mask, _ = pg.unclassified(db, case.reads, case.hits, want_reads=False)
    share = mask.sum() / case.n
    print("selected share under the defaults: %.3f" % share)
    assert 0.10 < share < 0.90
    e_max = unclas_rule.thresholds()[1]
    fields = [[row_fields(r) for r in rows] for rows in case.rows]
    assert any(not f for f in fields)                                                           # no rows
    assert any(f and all(p < 95 and e <= e_max and b >= 200 for p, e, b in f) for f in fields)  # pident alone
    assert any(f and all(p >= 95 and (e > e_max or b < 200) for p, e, b in f) for f in fields)  # score alone
    two = kinds.index("row2")                                                                   # row 2 only
    t, e, b = unclas_rule.thresholds("100", "5", "0")
    passes = [not (p < t or ev > e or bs < b) for p, ev, bs in fields[two]]
    assert passes == [False, True]
    m2, _ = pg.unclassified(db, case.reads, case.hits, t="100", e="5", b="0", want_reads=False)
    assert m2[two] == 0
    slots = np.diff(case.hits.read_offsets(case.n))                                             # slots behind the count
    indel = kinds.index("indel")
    assert slots[indel] - case.counts[indel] > 0
    assert case.counts[kinds.index("many")] > 64                                                # more than 64 rows


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mix", range(len(MIXES)))
def test_resident_form_equals_rule_and_verb(batches, n, mix):
    mask = subset_checks(batches[n], MIXES[mix])
    if MIXES[mix] == {"b": "1e9"}:
        assert mask.all()
    if MIXES[mix] == {"t": "0", "b": "0", "e": "700"}:
        assert np.array_equal(mask, (batches[n].counts == 0).astype(np.uint8))


def test_ungapped_table(world):
    pg, d, db, reads, rng = world
    db.set_ungapped(True)      # (kept for the checks: they search the subset batch through the same handle)
    try:
        case = Case(pg, db, d, "ung", fasta_text([b"u%d" % i for i in range(300)], [s for _, s in reads[:300]]))
        for opts in ({}, {"t": "100", "b": "0", "e": "5"}, {"b": "150"}):
            mask = subset_checks(case, opts)
    finally:
        db.set_ungapped(False)
    assert 0 < mask.sum() < case.n


def test_special_reads(world):
    """Lengths around the word sizes, IUPAC letters, a mate-joined read, a low-complexity read: none has a passing row, all
    are selected, and the subset batch equals the import of the verb's output."""
    pg, d, db, reads, rng = world
    joined_hit = reads[0][1][:70] + b"N" * 8 + reads[0][1][80:]        # its pieces hit; the rows carry the read's number
    seqs = [_rand(rng, L) for L in (31, 32, 33, 64, 65, 513)]
    iupac = bytearray(_rand(rng, 150))
    for p, c in zip((3, 40, 41, 99, 149), b"RYKMN"):
        iupac[p] = c
    seqs += [bytes(iupac), _rand(rng, 70) + b"N" * 8 + _rand(rng, 72), b"A" * 150, b"AC" * 75]
    special = len(seqs)
    seqs += [joined_hit, reads[0][1], reads[3][1], _rand(rng, 150)]
    case = Case(pg, db, d, "special", fasta_text([b"s%d" % i for i in range(len(seqs))], seqs))
    any_dust = case.reads.dust_bits()[0]
    assert any_dust[special - 2] and any_dust[special - 1]
    for opts in MIXES:
        mask = subset_checks(case, opts)
        assert mask[:special].all()
    assert case.counts[special] > 0 and mask[special]                         # (at -b 1e9 everything is selected)
    mask = subset_checks(case, {"t": "0", "b": "0", "e": "700"})
    assert list(mask[special:]) == [0, 0, 0, 1]
    mask = subset_checks(case, {})
    assert list(mask[special:]) == [1, 0, 0, 1]                               # 70-base pieces score under 200 bits


@pytest.mark.parametrize("which", ["classified_first", "classified_last"])
def test_duplicate_names(world, which):
    pg, d, db, reads, rng = world
    hit, miss = reads[0][1], [_rand(rng, 150) for _ in range(4)]
    if which == "classified_first":      # the classified read is dropped, the others are kept
        names, seqs = [b"x", b"dup", b"y", b"dup", b"dup"], [miss[0], hit, miss[1], miss[2], miss[3]]
        want = [1, 0, 1, 1, 1]
    else:                                # only the last has a passing row: the FIRST is dropped, the others are kept
        names, seqs = [b"dup", b"x", b"dup", b"y", b"dup"], [miss[0], miss[1], miss[2], miss[3], hit]
        want = [0, 1, 1, 1, 1]
    case = Case(pg, db, d, which, fasta_text(names, seqs))
    assert list(subset_checks(case, {})) == want
    assert subset_checks(case, {"b": "1e9"}).all()


def test_synthetic_batch_names(world):
    """a generated batch carries no name bytes: the subset's names are rendered as name_of() does"""
    pg, d, db, reads, rng = world
    cfg = pg.SynthCfg.default(n_seq=300, seq_len=500, n_genus=20, read_len=150)
    sdb = pg.Db.from_synth(cfg)
    case = Case.__new__(Case)
    case.pg, case.db, case.d, case.tag = pg, sdb, d, "synth"
    case.reads = pg.Reads.from_synth(cfg, 995, 130)      # names r995 .. r1124: three and four digits
    case.n = len(case.reads)
    case.hits = _capi.blast_search(sdb, case.reads)
    case.table = case.hits.format(sdb, case.reads)
    case.m_path, case.s_path = str(d / "synth.m.tsv"), str(d / "synth.s.fas")
    open(case.m_path, "wb").write(case.table)
    case.reads.write_fasta(case.s_path)
    case.fasta = open(case.s_path, "rb").read()
    case.counts = case.hits.read_counts(case.n)
    lines = case.table.split(b"\n")[:-1]
    ends = np.cumsum(case.counts)
    case.rows = [lines[e - c:e] for c, e in zip(case.counts, ends)]
    for opts in ({}, {"t": "99.5"}, {"b": "1e9"}):
        mask = subset_checks(case, opts)
    assert mask.all()
