"""GPU parity of the barcode demultiplexer (Barcode/barcode.pl).

File verb: every golden case printed by the reference's Perl through pgx_barcode_file and through the CLI binary -- stdout,
status and the full set of files in -d, byte for byte; a refused case leaves -d empty.  Generated inputs against
tests/barcode_rule.py at the sizes where the kernels change path: records per wavefront block, barcodes per ballot (64),
the 8-letter masked word, the aligned loads' edges, lines longer than a wavefront.  Resident form: the batch of every
barcode against the batch pgx_reads_from_fasta makes of the verb's file, and one of them searched.
"""
import os

import numpy as np
import pytest

import barcode_rule
from pangea_plus_amd import _capi
from conftest import ROOT, run_cmd
from test_barcode_rule import cases, load_case

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "pangea-plus_amd", "bin", "barcode")
STATUS = {"E_ARG": -1, "E_LIMIT": -7, "E_REFHANG": -6}
STD = ["-s", "reads.fas", "-b", "barcodes.txt", "-d", "d"]
TAIL = b">tail\nNNNN\n"  # the file's last record goes another way (and may never end): this one takes that place


def files_in(d):
    return {os.fsencode(f): open(os.path.join(str(d), f), "rb").read() for f in os.listdir(str(d))}


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", cases())
def test_file_verb_and_cli_match_the_reference_script(name, tmp_path):
    import pangea_plus_amd as pg
    pg.init(0)
    for how in ("verb", "cli"):
        work = tmp_path / how
        work.mkdir()
        argv, stdout, status, files = load_case(name, work)
        if how == "verb":
            try:
                got_stdout, got_status = pg.barcode(argv, cwd=str(work)), 0
            except pg.PangeaError as e:
                got_stdout, got_status = e.stdout, e.status
            want_status = STATUS.get(status, status)
        else:
            got_status, got_stdout, _ = run_cmd([BIN] + argv, cwd=str(work))
            want_status = 3 if status in STATUS else status
        assert got_stdout == stdout
        assert got_status == want_status
        assert (files_in(work / "d") or None) == files      # (no unexpected file, none at all for a refused case)


# ------------------------------------------------------------------------------------------ generated inputs
def rand_letters(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8)) if n else b""


def rand_barcodes(rng, n, length=8):
    seen, out = set(), []
    while len(out) < n:
        s = rand_letters(rng, length)
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def barcode_file(bars):
    return b"".join(b"s%d\t%s\n" % (i, s) for i, s in enumerate(bars))


KINDS = ["prefix1", "sub1", "prefix2", "sub2", "sub3", "break", "none"]


def make_read(rng, bars, width, kind, n=None, alphabet=b"ACGT"):
    """sequence lines of one read: `kind` says where a barcode is planted"""
    n = int(rng.randint(0, 320)) if n is None else n
    s = bytearray(rand_letters(rng, n, alphabet))
    bc = bars[rng.randint(len(bars))]
    L = len(bc)
    off = {"prefix1": 0, "sub1": 1 + rng.randint(max(1, width - L)), "prefix2": width, "sub2": width + 1 + rng.randint(max(1, width - L)),
           "sub3": 2 * width + 1 + rng.randint(max(1, width - L)), "break": width - 1 - rng.randint(max(1, L - 1)), "none": None}[kind]
    if off is not None and 0 <= off and off + L <= n:
        s[off:off + L] = bc
    s = bytes(s)
    return [s[i:i + width] for i in range(0, len(s), width)]


def make_text(rng, bars, n_rec, width=60, kinds=KINDS, blank=0.02, alphabet=b"ACGT", tail=TAIL):
    out = []
    for r in range(n_rec):
        out.append(b">r%d len\n" % r)
        for ln in make_read(rng, bars, width, kinds[rng.randint(len(kinds))], alphabet=alphabet):
            out.append(ln + b"\n")
            if rng.rand() < blank:
                out.append(b"\n")
    return b"".join(out) + (tail if n_rec else b"")


_run = [0]


def check(pg, tmp_path, btext, text):
    """the verb on (btext, text) against the rule: stdout, status and every file; returns the rule's per-record fates"""
    _run[0] += 1
    work = tmp_path / ("w%d" % _run[0])
    work.mkdir()
    (work / "d").mkdir()
    (work / "barcodes.txt").write_bytes(btext)
    (work / "reads.fas").write_bytes(text)
    want_stdout, want_status, want_files = barcode_rule.run(STD, cwd=str(work))
    try:
        got_stdout, got_status = pg.barcode(STD, cwd=str(work)), 0
    except pg.PangeaError as e:
        got_stdout, got_status = e.stdout, e.status
    assert got_status == STATUS.get(want_status, want_status)
    assert got_stdout == want_stdout
    got_files = files_in(work / "d") or None
    if got_files != want_files:
        for k in sorted(want_files or {}):
            assert (got_files or {}).get(k) == want_files[k], k
    assert got_files == want_files
    if want_status != 0:
        return None
    return barcode_rule.fates(barcode_rule.parse_barcodes(btext), text)


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


@pytest.mark.parametrize("n_rec", [0, 1, 2, 63, 64, 65, 3000])
def test_record_counts(pg, tmp_path, n_rec):
    rng = np.random.RandomState(1000 + n_rec)
    bars = rand_barcodes(rng, 5)
    fates = check(pg, tmp_path, barcode_file(bars), make_text(rng, bars, n_rec))
    if n_rec == 3000:  # every fate, from the rule's own output
        kept = [f for f in fates if f[0] == barcode_rule.KEPT]
        assert sum(f[0] == barcode_rule.NOBAR for f in fates) >= 10
        assert sum(f[0] == barcode_rule.THROWN for f in fates) >= 10
        assert sum(f[2] == 1 for f in kept) >= 10 and sum(f[2] > 1 for f in kept) >= 10
        assert sum(f[0] == barcode_rule.THROWN and f[2] > 1 for f in fates) >= 10


@pytest.mark.parametrize("n_rec", [1, 2, 3])
def test_no_safe_tail(pg, tmp_path, n_rec):
    """the last record is one of the planted ones: decided on the host, written by the same kernel (or refused: the script
    never ends on some)"""
    rng = np.random.RandomState(77 + n_rec)
    bars = rand_barcodes(rng, 3)
    seen = set()
    for k in range(40):
        text = make_text(rng, bars, n_rec, width=[50, 60, 70][k % 3], tail=b"")
        if k % 5 == 0:
            text = text[:-1]
        if k % 7 == 0:
            text = text.replace(b"\n", b"\r\n")
        fates = check(pg, tmp_path, barcode_file(bars), text)
        seen.add("refused" if fates is None else fates[-1][0])
    assert len(seen) >= (2 if n_rec == 1 else 3)   # (a file of one read never yields that read)


@pytest.mark.parametrize("n_bars", [1, 63, 64, 65, 200])
def test_barcode_counts(pg, tmp_path, n_bars):
    rng = np.random.RandomState(2000 + n_bars)
    bars = rand_barcodes(rng, n_bars)
    text = make_text(rng, bars, 300, tail=b"") + make_text(rng, bars[-1:], 12, kinds=["prefix1", "sub1"])  # (the last one, too)
    fates = check(pg, tmp_path, barcode_file(bars), text)
    hit = {f[1] for f in fates if f[0] == barcode_rule.KEPT}
    assert len(hit) >= min(n_bars, 40)
    if n_bars > 64:
        assert any(a >= 64 for a in hit)


@pytest.mark.parametrize("order", [0, 1])
def test_two_barcodes_that_differ_in_their_ninth_letter(pg, tmp_path, order):
    rng = np.random.RandomState(31 + order)
    stem = rand_letters(rng, 8)
    bars = [stem + b"A", stem + b"C"][::1 - 2 * order]
    text = make_text(rng, bars, 200, kinds=["prefix1", "sub1", "prefix2", "sub2"], alphabet=b"GT")
    fates = check(pg, tmp_path, barcode_file(bars), text)
    assert {f[1] for f in fates if f[0] == barcode_rule.KEPT} == {0, 1}


@pytest.mark.parametrize("length", [1, 8, 9, 64])
def test_barcode_lengths(pg, tmp_path, length):
    rng = np.random.RandomState(40 + length)
    bars = rand_barcodes(rng, 2 if length == 1 else 4, length)
    alphabet = bytes(set(b"ACGT") - set(b"".join(bars))) if length == 1 else b"ACGT"
    text = make_text(rng, bars, 200, width=70 if length == 64 else 60, alphabet=alphabet)
    fates = check(pg, tmp_path, barcode_file(bars), text)
    assert sum(f[0] == barcode_rule.KEPT for f in fates) >= 20
    assert sum(f[0] == barcode_rule.NOBAR for f in fates) >= 5


def test_the_limits_hold_what_the_issue_asks(pg, tmp_path):
    """1 024 barcodes of 64 letters work; 2 049 barcodes are refused with nothing written"""
    rng = np.random.RandomState(5)
    bars = rand_barcodes(rng, 1024, 64)
    fates = check(pg, tmp_path, barcode_file(bars), make_text(rng, bars, 60, width=70))
    assert any(f[0] == barcode_rule.KEPT and f[1] >= 512 for f in fates)
    many = rand_barcodes(rng, 2049, 8)
    assert check(pg, tmp_path, barcode_file(many), TAIL) is None


@pytest.mark.parametrize("line", [1, 2])
def test_barcode_offsets_around_the_aligned_loads(pg, tmp_path, line):
    rng = np.random.RandomState(60 + line)
    bars = [b"ACGTACGTAC", b"TTGACCAT"]
    width = 60
    recs = []
    for bc in bars:
        for off in (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, width - len(bc), width - len(bc) - 1):
            for shift in range(8):   # (every alignment of the line's own start: the header's length moves it)
                s = bytearray(rand_letters(rng, 4 * width, b"GC"))
                at = (line - 1) * width + off
                s[at:at + len(bc)] = bc
                recs.append(b">" + b"x" * shift + b"\n" + b"".join(bytes(s[i:i + width]) + b"\n" for i in range(0, len(s), width)))
    fates = check(pg, tmp_path, barcode_file(bars), b"".join(recs) + TAIL)
    assert all(f[0] == barcode_rule.KEPT for f in fates[:-1])
    assert {f[2] for f in fates[:-1]} == ({1} if line == 1 else {1, 2})


@pytest.mark.parametrize("width", [1, 63, 64, 65, 1000])
def test_line_lengths(pg, tmp_path, width):
    rng = np.random.RandomState(80 + width)
    bars = [b"A"] if width == 1 else rand_barcodes(rng, 3, 8)
    out = []
    for r in range(120):
        out.append(b">r%d\n" % r)
        if width == 1:
            s = rand_letters(rng, rng.randint(0, 160), b"GGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGA")
            lines = [s[i:i + 1] for i in range(len(s))]
        else:
            lines = make_read(rng, bars, width, KINDS[rng.randint(len(KINDS))], n=int(rng.randint(0, 3 * width + 40)))
        out += [ln + b"\n" for ln in lines]
    fates = check(pg, tmp_path, barcode_file(bars), b"".join(out) + TAIL)
    assert sum(f[0] == barcode_rule.KEPT for f in fates) >= 10


# ------------------------------------------------------------------------------------------ resident form
def same_batch(a, b, tmp_path, tag):
    assert len(a) == len(b)
    pa, pb = str(tmp_path / (tag + ".a.fas")), str(tmp_path / (tag + ".b.fas"))
    a.write_fasta(pa)
    b.write_fasta(pb)
    assert open(pa, "rb").read() == open(pb, "rb").read()   # names and letters
    for i in range(len(a)):
        assert np.array_equal(a.get(i), b.get(i))


def test_resident_form(pg, tmp_path):
    rng = np.random.RandomState(9)
    subjects = [rand_letters(rng, 500) for _ in range(20)]
    (tmp_path / "db.fa").write_bytes(b"".join(b">gi|%d|s%d|\n%s\n" % (1000 + i, i, s) for i, s in enumerate(subjects)))
    db = pg.Db.from_fasta(str(tmp_path / "db.fa"))
    bars = rand_barcodes(rng, 5)
    unused = 3
    used = [b for i, b in enumerate(bars) if i != unused]
    text = make_text(rng, used, 400, tail=b"")
    for r in range(30):  # reads that lie in the database, behind barcode 0
        s = subjects[r % 20]
        st = rng.randint(0, 300)
        read = bars[0] + s[st:st + 200]
        text += b">db%d\n" % r + b"".join(read[i:i + 60] + b"\n" for i in range(0, len(read), 60))
    text += TAIL
    btext = barcode_file(bars)
    (tmp_path / "d").mkdir()
    (tmp_path / "barcodes.txt").write_bytes(btext)
    (tmp_path / "reads.fas").write_bytes(text)
    pg.barcode(STD, cwd=str(tmp_path))
    counts, files = barcode_rule.demux(barcode_rule.parse_barcodes(btext), text)
    assert files_in(tmp_path / "d") == files
    res = pg.barcode_reads(str(tmp_path / "reads.fas"), str(tmp_path / "barcodes.txt"))
    assert len(res) == 5
    assert res.sequences == counts["count"] and res.no_barcode == counts["nobar"] and res.thrown_out == counts["thrown"]
    for i in range(5):
        assert res.name(i) == b"s%d" % i and res.letters(i) == bars[i]
        assert res.count(i) == counts["bar_count"][i]
        got = res.take_reads(i)
        ref = pg.Reads.from_fasta(str(tmp_path / "d" / ("bars%d.fas" % i)))
        assert len(got) == counts["bar_count"][i]
        same_batch(got, ref, tmp_path, "bar%d" % i)
    assert counts["bar_count"][unused] == 0 and len(res.take_reads(unused)) == 0
    same_batch(res.take_reads(-1), pg.Reads.from_fasta(str(tmp_path / "d" / "nobar.fas")), tmp_path, "nobar")
    got, ref = res.take_reads(0), pg.Reads.from_fasta(str(tmp_path / "d" / "bars0.fas"))   # searched once
    table = _capi.blast_search(db, got).format(db, got)
    assert table == _capi.blast_search(db, ref).format(db, ref)
    assert table.count(b"\n") >= 30
    res.close()


def test_resident_form_refuses_what_the_verb_refuses(pg, tmp_path):
    (tmp_path / "reads.fas").write_bytes(TAIL)
    for btext, status in ((b"A ACGT\n", -1), (b"A\tAC1T\n", -1), (b"A\t" + b"ACGTA" * 13 + b"\n", -7)):
        (tmp_path / "barcodes.txt").write_bytes(btext)
        with pytest.raises(pg.PangeaError) as e:
            pg.barcode_reads(str(tmp_path / "reads.fas"), str(tmp_path / "barcodes.txt"))
        assert e.value.status == status
    (tmp_path / "barcodes.txt").write_bytes(b"A\tACGT\n")
    (tmp_path / "reads.fas").write_bytes(b"stray\n" + TAIL)
    with pytest.raises(pg.PangeaError) as e:
        pg.barcode_reads(str(tmp_path / "reads.fas"), str(tmp_path / "barcodes.txt"))
    assert e.value.status == -1
    with pytest.raises(pg.PangeaError) as e:
        pg.barcode_reads(str(tmp_path / "absent.fas"), str(tmp_path / "barcodes.txt"))
    assert e.value.status == -2
