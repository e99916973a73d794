"""GPU parity after the search step's grow-and-repeat: every device table of `search_pipeline` is sized on a guess, the
kernels drop what falls past a capacity, and the host repeats the step with larger tables when the counters say one was
too small.  Each case builds an input whose shape alone overflows one buffer on a fresh handle, asserts that the step
repeated for that buffer (`pgx_stage_times.grown`: 1 seed table, 2 overflow table, 4 gapped tier list, 8 hit table) and
compares the product's bytes with the oracle's on the same files.

First guesses on a fresh handle (classify.hip, search_pipeline; gapped.hip, gapped_stage), n = reads (or pieces):
  seed table      max(40 n, 65 536) + 256 * 8 * 4 * 2 048 slots (records of reads with <= 128 staged hits)
  overflow table  max(n / 4, 65 536) records (a read spills there once its stage of 128 holds more than 64 hits
                  in the middle of the scan: cases that must not spill keep to 64 hits a read)
  gapped list A   max(2^20, (seed + overflow capacity) / 16) entries (reads of <= 512 bases)
  hit table       max(36 n, 65 536) rows; checked only once the other three held everything
  soap placements max(8 n, 1 024)"""
import numpy as np
import pytest

from conftest import run_cmd

pytestmark = pytest.mark.gpu

THREADS = "16"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
SEED_SLOTS = 256 * 8 * 4 * 2048  # one open chunk of 2 048 slots per wavefront of the seed kernel's largest grid


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


# ------------------------------------------------------------------------------------------------ seeded inputs
def break_runs(w, longest):
    """Changes in place every base of the rows of `w` that would make a homopolymer longer than `longest`."""
    for j in range(longest, w.shape[1]):
        same = np.ones(w.shape[0], dtype=bool)
        for k in range(1, longest + 1):
            same &= w[:, j - k] == w[:, j]
        w[same, j] = (w[same, j] + 1) % 4
    return w


def families(rng, n_fam, per_fam, length, subs, longest_run=0):
    """`n_fam` random ancestors of `length` bases (with no homopolymer longer than `longest_run`, if given); each family
    holds `per_fam` copies of its ancestor with `subs` substitutions each.  Returns the ancestors (n_fam x length codes)
    and the subjects (family-major)."""
    anc = rng.integers(0, 4, size=(n_fam, length), dtype=np.uint8)
    if longest_run:
        break_runs(anc, longest_run)
    subj = np.repeat(anc, per_fam, axis=0)
    rows = np.arange(subj.shape[0])[:, None]
    pos = np.argsort(rng.random((subj.shape[0], length)), axis=1)[:, :subs]
    subj[rows, pos] = (subj[rows, pos] + rng.integers(1, 4, size=pos.shape, dtype=np.uint8)) % 4
    return anc, subj


def windows(rng, anc, n, read_len, subs, deletion=0, minus=True, head=0, longest_run=0):
    """`n` reads: windows of `read_len` bases of random ancestors with up to `subs` substitutions (drawn positions may
    repeat) outside the first `head` bases, and `deletion` bases deleted 60-90 bases into the window; every second read
    from the minus strand when `minus`; with `longest_run`, bases that would make a longer homopolymer are changed too."""
    fam = rng.integers(0, anc.shape[0], size=n)
    start = rng.integers(0, anc.shape[1] - read_len - deletion + 1, size=n)
    col = np.arange(read_len)[None, :]
    idx = start[:, None] + col
    if deletion:
        idx = idx + (col >= rng.integers(60, 91, size=n)[:, None]) * deletion
    w = anc[fam[:, None], idx]
    if subs:
        rows = np.arange(n)[:, None]
        p = rng.integers(head, read_len, size=(n, subs))
        w[rows, p] = (w[rows, p] + rng.integers(1, 4, size=(n, subs), dtype=np.uint8)) % 4
    if longest_run:
        break_runs(w, longest_run)
    if minus:
        w[1::2] = 3 - w[1::2, ::-1]
    text = ACGT[w]
    return [r.tobytes() for r in text]


def write_db(path, subj):
    with open(path, "wb") as f:
        for i, s in enumerate(subj):
            f.write(b">gi|%d|x|c%d|\n%s\n" % (i + 1, i, ACGT[s].tobytes()))


def write_reads(path, reads, tag="r"):
    with open(path, "wb") as f:
        for i, s in enumerate(reads):
            f.write(b">%s%d\n%s\n" % (tag.encode(), i, s))


def oracle_blast(oracle_bin, reads_fa, db_fa, out, timeout, ungapped=False):
    cmd = [oracle_bin, "blastn", "-query", str(reads_fa), "-db", str(db_fa), "-outfmt", "6", "-out", str(out),
           "-num_threads", THREADS] + (["-ungapped"] if ungapped else [])
    rc, _, se = run_cmd(cmd, timeout=timeout)
    assert rc == 0, se
    return out.read_bytes()


def search(pg, db, reads_fa):
    """One search through `db`: the -outfmt 6 bytes and the stage record of that step."""
    from pangea_plus_amd import _capi
    reads = pg.Reads.from_fasta(str(reads_fa))
    hits = _capi.blast_search(db, reads)
    st = _capi.stage_times()
    return hits.format(db, reads), st, len(reads)


def fresh_db(pg, db_fa, ungapped=False):
    db = pg.Db.from_fasta(str(db_fa))
    if ungapped:
        db.set_ungapped(True)
    return db


def subjects_per_read(text):
    per = {}
    for line in text.decode().splitlines():
        q, s = line.split("\t")[:2]
        per.setdefault(q, set()).add(s)
    return per


# ------------------------------------------------------------------------------------------------ 1. hit table
# 30 families of 60 copies: every 150-base read hits the 60 subjects of its family -- under the 64 staged hits that
# would spill, far under the seed table, but 3 000 x 60 = 180 000 rows against a first hit table of 36 x 3 000 = 108 000
HEAVY_FAM, HEAVY_COPIES, HEAVY_N = 30, 60, 3000


@pytest.fixture(scope="module")
def heavy(tmp_path_factory):
    d = tmp_path_factory.mktemp("heavy")
    rng = np.random.default_rng(1101)
    anc, subj = families(rng, HEAVY_FAM, HEAVY_COPIES, 300, 3)
    write_db(d / "db.fa", subj)
    write_reads(d / "reads.fa", windows(rng, anc, HEAVY_N, 150, 2))
    # the piece path: two reads joined by 100 N's (the shape `trim2 -g` writes for a read pair)
    a, b = windows(rng, anc, 1500, 150, 2), windows(rng, anc, 1500, 150, 2)
    write_reads(d / "pairs.fa", [x + b"N" * 100 + y for x, y in zip(a, b)], "p")
    return d, anc


@pytest.mark.parametrize("ungapped", [False, True], ids=["gapped", "ungapped"])
def test_hit_table_alone_grows(pg, oracle_bin, heavy, ungapped):
    d, _ = heavy
    want = oracle_blast(oracle_bin, d / "reads.fa", d / "db.fa", d / ("want_%d.tsv" % ungapped), 300, ungapped)
    rows = want.count(b"\n")
    assert rows > 1.5 * 36 * HEAVY_N
    assert max(len(v) for v in subjects_per_read(want).values()) <= 64
    got, st, n = search(pg, fresh_db(pg, d / "db.fa", ungapped), d / "reads.fa")
    assert (st.grown, st.attempts >= 2) == (8, True), (st.grown, st.attempts, st.hits)
    assert got == want


# ------------------------------------------------------------------------------------------------ 5. pieces
def test_piece_path_repeats_on_the_hit_table(pg, oracle_bin, heavy):
    """Reads split at a 100-N run are searched as 3 000 pieces; the repeated step goes through k_merge_pieces and
    k_piece_ranges again (the hit table's guess follows the piece count: 108 000 rows for about 180 000)."""
    d, _ = heavy
    want = oracle_blast(oracle_bin, d / "pairs.fa", d / "db.fa", d / "want_pairs.tsv", 300)
    assert want.count(b"\n") > 1.5 * 36 * 3000
    got, st, n = search(pg, fresh_db(pg, d / "db.fa"), d / "pairs.fa")
    assert n == 1500
    assert (st.grown, st.attempts >= 2) == (8, True), (st.grown, st.attempts, st.hits)
    assert got == want


# ------------------------------------------------------------------------------------------------ 2. overflow table
def test_overflow_table_alone_grows(pg, oracle_bin, tmp_path):
    """120 reads hit about 3 000 subjects each: some 360 000 hits spill to an overflow table of 65 536 records.  13 000 reads
    of random bases (no hit) raise the hit table's guess to 36 x 13 120 = 472 320 rows, so that only the overflow table
    grows.  The reads of > 64 hits take the segmented sorts behind the repeated step; the 500-subject cut holds."""
    rng = np.random.default_rng(2202)
    anc, subj = families(rng, 1, 3000, 300, 3)
    write_db(tmp_path / "db.fa", subj)
    heavy_reads = windows(rng, anc, 120, 150, 2)
    filler = [ACGT[rng.integers(0, 4, size=150, dtype=np.uint8)].tobytes() for _ in range(13000)]
    reads = [x for pair in zip(heavy_reads, filler[:120]) for x in pair] + filler[120:]
    write_reads(tmp_path / "reads.fa", reads)
    want = oracle_blast(oracle_bin, tmp_path / "reads.fa", tmp_path / "db.fa", tmp_path / "want.tsv", 600)
    per = subjects_per_read(want)
    assert len(per) == 120 and min(len(v) for v in per.values()) == max(len(v) for v in per.values()) == 500
    got, st, n = search(pg, fresh_db(pg, tmp_path / "db.fa"), tmp_path / "reads.fa")
    assert n == 13120 and 65536 < st.hits < 36 * n
    assert (st.grown, st.attempts >= 2) == (2, True), (st.grown, st.attempts, st.hits)
    assert got == want


# ------------------------------------------------------------------------------------------------ 3. gapped list A
def test_gapped_list_alone_grows(pg, oracle_bin, tmp_path):
    """80 000 reads with a 3-base deletion against 20 near-copies each: every HSP holds gap columns and is listed by the
    first tier, about 1.6 M entries against a list of max(2^20, (40 n + 16.8 M + n / 4) / 16) = 1.25 M; 20 hits a read stay
    under the hit table's 36."""
    rng = np.random.default_rng(3303)
    anc, subj = families(rng, 400, 20, 300, 3)
    write_db(tmp_path / "db.fa", subj)
    n = 80000
    write_reads(tmp_path / "reads.fa", windows(rng, anc, n, 150, 1, deletion=3))
    want = oracle_blast(oracle_bin, tmp_path / "reads.fa", tmp_path / "db.fa", tmp_path / "want.tsv", 900)
    listed_cap = max(1 << 20, (40 * n + SEED_SLOTS + max(n // 4, 65536)) // 16)
    assert want.count(b"\n") > 1.2 * listed_cap
    got, st, _ = search(pg, fresh_db(pg, tmp_path / "db.fa"), tmp_path / "reads.fa")
    assert (st.grown, st.attempts >= 2) == (4, True), (st.grown, st.attempts, st.hits, st.gapped_wide)
    assert st.gapped_wide > listed_cap
    assert got == want


def test_gapped_list_alone_grows_in_the_one_list_mode(pg, oracle_bin, tmp_path):
    """Reads of 321-512 bases take the one-list ("deep") form of the gapped stage: the first tier holds 40 differences a
    side and puts what is still alive after them in list A (list B is list A).  110 000 reads of 450 bases, each with a 3-base
    deletion, the first 100 bases as in the ancestor and about 50 substitutions behind them, against 16 near-copies each:
    every HSP has a side with more than 40 differences, 1.76 M entries against a list of
    max(2^20, (40 n + 16.8 M + n / 4) / 16) = 1.33 M; 16 hits a read stay under the hit table's 36.
    (No read holds a homopolymer longer than 4.  About 8 % of random 450-base reads hold one of seven, and reads with a
    DUST-masked base are a search class of their own.  Every class is a launch of the seed kernel whose wavefronts each
    open a chunk of 2 048 slots.  Two large launches outgrow the 16.8 M slots the seed table's guess allows for
    open chunks, so that table would repeat the step too.)"""
    rng = np.random.default_rng(3313)
    anc, subj = families(rng, 2000, 16, 600, 3, longest_run=4)
    write_db(tmp_path / "db.fa", subj)
    n = 110000
    write_reads(tmp_path / "reads.fa", windows(rng, anc, n, 450, 55, deletion=3, head=100, longest_run=4))
    want = oracle_blast(oracle_bin, tmp_path / "reads.fa", tmp_path / "db.fa", tmp_path / "want.tsv", 900)
    listed_cap = max(1 << 20, (40 * n + SEED_SLOTS + max(n // 4, 65536)) // 16)
    assert want.count(b"\n") > 1.2 * listed_cap
    got, st, _ = search(pg, fresh_db(pg, tmp_path / "db.fa"), tmp_path / "reads.fa")
    assert (st.grown, st.attempts >= 2) == (4, True), (st.grown, st.attempts, st.hits, st.gapped_wide)
    assert st.gapped_wide > listed_cap
    assert got == want


# ------------------------------------------------------------------------------------------------ 4. seed table
def test_seed_table_grows_and_three_windows_equal_the_oracle(pg, oracle_bin, tmp_path):
    """1.6 M reads with 62 subjects each (no spill) store 99 M seed records against a first seed table of 40 n + 16.8 M =
    80.8 M slots; the hit table (36 n) then grows as well, on the attempt after.  Three windows of the batch against the
    oracle."""
    from pangea_plus_amd import _capi
    rng = np.random.default_rng(4404)
    anc, subj = families(rng, 100, 62, 300, 3)
    write_db(tmp_path / "db.fa", subj)
    n, part, win = 1600000, 100000, 1500
    firsts = (0, n // 2 - win // 2, n - win)
    kept = {}
    with open(tmp_path / "reads.fa", "wb") as f:
        for p0 in range(0, n, part):
            for i, s in enumerate(windows(rng, anc, part, 150, 2)):
                f.write(b">r%d\n%s\n" % (p0 + i, s))
                if any(a <= p0 + i < a + win for a in firsts):
                    kept[p0 + i] = s
    db = fresh_db(pg, tmp_path / "db.fa")
    all_reads = pg.Reads.from_fasta(str(tmp_path / "reads.fa"))
    hits = _capi.blast_search(db, all_reads)
    st = _capi.stage_times()
    assert (st.grown, st.attempts) == (9, 3), (st.grown, st.attempts, st.hits)
    assert st.hits > 40 * n + SEED_SLOTS
    off = hits.read_offsets(n)
    assert off[-1] == len(hits) == st.hits
    del all_reads
    for first in firsts:
        w_fa = tmp_path / ("w%d.fa" % first)
        with open(w_fa, "wb") as f:
            for i in range(first, first + win):
                f.write(b">r%d\n%s\n" % (i, kept[i]))
        want = oracle_blast(oracle_bin, w_fa, tmp_path / "db.fa", tmp_path / ("w%d.tsv" % first), 300)
        assert want.count(b"\n") > 50 * win, first
        w_reads = pg.Reads.from_fasta(str(w_fa))
        assert hits.slice(first, win).format(db, w_reads) == want, first


# ------------------------------------------------------------------------------------------------ 6. fused path
def test_fused_consensus_after_a_repeat_equals_the_oracle_chain(pg, oracle_bin, tmp_path):
    """classify_consensus with RDP and taxonomy on a synthetic database of 60 sequences per genus: reads hit about 50 of
    them (never more than 60: no spill), 4 000 x 50 rows against a first hit table of 144 000.  k_consensus_serial and the
    ordering kernels run on the repeated step's table; Consensus text against the chain blastn -> taxcollector -> consensus."""
    from pangea_plus_amd import _capi
    shape = dict(n_seq=2400, seq_len=500, n_genus=40, read_len=150)
    args = ["--n-seq", "2400", "--seq-len", "500", "--n-genus", "40", "--read-len", "150"]
    n = 4000
    d = tmp_path
    (d / "Tax_class").mkdir()
    assert run_cmd([oracle_bin, "synth", "db", "--out", str(d / "db.fa")] + args)[0] == 0
    assert run_cmd([oracle_bin, "synth", "reads", "--out", str(d / "reads.fa"), "--count", str(n)] + args)[0] == 0
    assert run_cmd([oracle_bin, "synth", "rdp", "--out", str(d / "rdp.tsv"), "--count", str(n)] + args)[0] == 0
    assert run_cmd([oracle_bin, "synth", "taxdump", "--out", str(d / "Tax_class")] + args)[0] == 0
    assert run_cmd([oracle_bin, "tax_class", "-c"], cwd=d / "Tax_class")[0] == 0
    want = oracle_blast(oracle_bin, d / "reads.fa", d / "db.fa", d / "hits.tsv", 300)
    assert run_cmd([oracle_bin, "taxcollector", "-f", str(d / "hits.tsv"), "-o", str(d / "hits_class.tsv"), "-d",
                    str(d / "Tax_class")], timeout=300)[0] == 0
    assert run_cmd([oracle_bin, "consensus", "-b", str(d / "hits_class.tsv"), "-r", str(d / "rdp.tsv"), "-o",
                    str(d / "consensus.txt")], timeout=300)[0] == 0
    assert want.count(b"\n") > 1.2 * 36 * n
    assert max(len(v) for v in subjects_per_read(want).values()) <= 60
    cfg = pg.SynthCfg.default(**shape)
    db = pg.Db.from_synth(cfg)
    db.bind_taxonomy(pg.TaxDb.open(str(d / "Tax_class")))
    reads = pg.Reads.from_synth(cfg, 0, n)
    rdp = pg.Rdp.from_synth(cfg, 0, n, db)
    hits, recs = _capi.classify_consensus(db, reads, rdp)
    st = _capi.stage_times()
    assert (st.grown, st.attempts >= 2) == (8, True), (st.grown, st.attempts, st.hits)
    assert hits.format(db, reads) == want
    assert _capi.consensus_format(db, reads, hits, recs) == (d / "consensus.txt").read_bytes()


# ------------------------------------------------------------------------------------------------ 7. handle reuse
def test_one_handle_grown_then_reused(pg, oracle_bin, tmp_path):
    """One handle: a heavy batch that repeats, the same batch again in one attempt, a lighter batch of another size (no
    stale rows from the grown tables), then batches of 400- and 1 400-base reads (one gapped list; long reads)."""
    rng = np.random.default_rng(7707)
    anc, subj = families(rng, 20, 90, 1500, 12)
    write_db(tmp_path / "db.fa", subj)
    batches = [("heavy", 3000, 150), ("light", 500, 150), ("r400", 300, 400), ("r1400", 40, 1400)]
    for tag, count, length in batches:
        write_reads(tmp_path / (tag + ".fa"), windows(rng, anc, count, length, max(2, length // 75)), tag)
    db = fresh_db(pg, tmp_path / "db.fa")
    want = oracle_blast(oracle_bin, tmp_path / "heavy.fa", tmp_path / "db.fa", tmp_path / "heavy.tsv", 300)
    got, st, _ = search(pg, db, tmp_path / "heavy.fa")
    assert st.grown & 8 and st.attempts >= 2, (st.grown, st.attempts, st.hits)
    assert got == want
    got, st, _ = search(pg, db, tmp_path / "heavy.fa")
    assert (st.attempts, st.grown) == (1, 0)
    assert got == want
    for tag, count, length in batches[1:]:
        want = oracle_blast(oracle_bin, tmp_path / (tag + ".fa"), tmp_path / "db.fa", tmp_path / (tag + ".tsv"), 600)
        assert want.count(b"\n") > 50 * count, tag
        got, st, n = search(pg, db, tmp_path / (tag + ".fa"))
        assert n == count
        if tag == "light":
            assert (st.attempts, st.grown) == (1, 0)
        assert got == want, tag


# ------------------------------------------------------------------------------------------------ 9. soap
def test_soap_placement_list_grows(pg, oracle_bin, tmp_path):
    """1 500 reads of 50 bases, each placed (at most 2 mismatches) in 20-60 identical copies of its segment: about 60 000
    placements against a first list of 8 x 1 500 = 12 000.  -r 2 and -r 1, rows and unmapped reads against the oracle."""
    rng = np.random.default_rng(9909)
    n_seg = 150
    seg = rng.integers(0, 4, size=(n_seg, 200), dtype=np.uint8)
    copies = rng.integers(20, 61, size=n_seg)
    subj = np.concatenate([np.repeat(seg[i:i + 1], copies[i], axis=0) for i in range(n_seg)])
    write_db(tmp_path / "ref.fa", subj)
    n = 1500
    reads = []
    for i in range(n):
        k = int(rng.integers(0, n_seg))
        o = int(rng.integers(0, 150))
        w = seg[k, o:o + 50].copy()
        m = int(rng.integers(0, 3))
        if m:
            p = rng.choice(50, size=m, replace=False)
            w[p] = (w[p] + rng.integers(1, 4, size=m, dtype=np.uint8)) % 4
        s = ACGT[w].tobytes()
        reads.append(s[::-1].translate(COMP) if i % 2 else s)
    write_reads(tmp_path / "reads.fa", reads, "s")
    pg.soap_index(str(tmp_path / "ref.fa"))
    index = str(tmp_path / "ref.fa") + ".index"
    # (the device's placement list holds every placement at the best level whatever -r says: -r only chooses how many of
    # a read's placements are printed, soap_run_single.  The -r 2 rows count that list, and -r 1 fills the same list)
    for r in (2, 1):
        p, pu, o, ou = (tmp_path / ("%s%d.txt" % (x, r)) for x in ("p", "pu", "o", "ou"))
        rc, _, se = run_cmd([oracle_bin, "soap", "-a", str(tmp_path / "reads.fa"), "-D", index, "-o", str(o), "-u", str(ou),
                             "-r", str(r)], timeout=300)
        assert rc == 0, se
        if r == 2:
            placements = o.read_bytes().count(b"\n")
            assert placements > max(8 * n, 1024) * 3
        else:
            assert o.read_bytes().count(b"\n") == n < placements  # one row a read, out of the same list
        pg.soap(str(tmp_path / "reads.fa"), index, str(p), u=str(pu), r=r)
        assert p.read_bytes() == o.read_bytes(), r
        assert pu.read_bytes() == ou.read_bytes(), r
