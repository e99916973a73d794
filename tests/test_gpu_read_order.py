"""GPU: the seed stage walks its reads in database order (classify.hip: order_reads; the key rule: csrc/read_order.hpp).

The order a search walks its reads in may change no output: every table is addressed by the read's number.  Each case
searches one batch twice through the C ABI, with `pgx_db_set_read_order(1)` (every class ordered) and `(2)` (never), and
compares the hit table (slot offsets, kept counts, the rows a text would show), the consensus records and the counters
probes / postings / survivors / candidates / hits of the two steps: a read that the list dropped or doubled shows in all of
them.  `pgx_db_get_read_order` gives the list itself: a permutation of the batch, class after class, bins non-decreasing
inside a class.  The key's quality is checked on synthetic reads with 1 % substitutions against the subjects they hit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COUNTERS = ("probes", "postings", "survivors", "candidates", "hits")


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


@pytest.fixture(scope="module")
def world(pg, tmp_path_factory):
    """A synthetic database of 3 000 sequences of 1 500 bases in 90 genera (33 relatives side by side, as in the bench's
    database) with its taxonomy bound."""
    from pangea_plus_amd import _capi
    cfg = pg.SynthCfg.default(n_seq=3000, n_genus=90)
    d = tmp_path_factory.mktemp("ro_tax")
    _capi._check(pg.lib().pgx_synth_write_taxdump(C.byref(cfg), str(d).encode()))
    pg.TaxDb.create(str(d))
    tax = pg.TaxDb.open(str(d))
    db = pg.Db.from_synth(cfg)
    db.bind_taxonomy(tax)
    return cfg, db, tax


def order_shift(n_bases):
    s = 0
    while ((n_bases - 1) >> s) + 2 > 65536:
        s += 1
    return s


def classify(pg, db, reads, rdp, mode):
    """One fused step in `mode`: what it computed, its counters, and the list it walked."""
    from pangea_plus_amd import _capi
    db.set_read_order(mode)
    hits, recs = _capi.classify_consensus(db, reads, rdp)
    st = _capi.stage_times()
    n = len(reads)
    h, off, mask = hits.rows(n)
    out = {"off": off, "cnt": hits.read_counts(n), "rows": h[mask], "recs": recs, "st": st,
           "counters": tuple(getattr(st, c) for c in COUNTERS)}
    out["order"], out["keys"] = db.read_order(reads)
    db.set_read_order(0)
    return out


def blast(pg, db, reads, mode):
    from pangea_plus_amd import _capi
    db.set_read_order(mode)
    hits = _capi.blast_search(db, reads)
    st = _capi.stage_times()
    n = len(reads)
    h, off, mask = hits.rows(n)
    out = {"off": off, "cnt": hits.read_counts(n), "rows": h[mask], "recs": None, "st": st,
           "counters": tuple(getattr(st, c) for c in COUNTERS)}
    out["order"], out["keys"] = db.read_order(reads)
    db.set_read_order(0)
    return out


def assert_same(a, b):
    assert a["counters"] == b["counters"], (COUNTERS, a["counters"], b["counters"])
    assert np.array_equal(a["off"], b["off"]) and np.array_equal(a["cnt"], b["cnt"])
    assert a["rows"].tobytes() == b["rows"].tobytes()
    if a["recs"] is not None:
        assert a["recs"].tobytes() == b["recs"].tobytes()


def assert_list(res, n_units):
    """The list of a mode-1 search: every read (piece) once; class after class; bins non-decreasing inside a class."""
    order, keys = res["order"], res["keys"]
    assert len(order) == n_units
    assert np.array_equal(np.sort(order), np.arange(n_units, dtype=np.uint32))
    assert np.all(np.diff(keys.astype(np.int64)) >= 0)  # class index << 16 | bin
    return keys >> 16


def letters(reads, i):
    return "".join("ACGTN"[b] for b in reads.get(i))


# ------------------------------------------------------------------------------------------------ plain batches
@pytest.fixture(scope="module")
def plain(pg, world):
    """3 001 synthetic reads of 150 bases, both strands, 1 % substitutions: an odd count, so the last wavefront of the seed
    kernel holds a lone read; searched once per mode and shared."""
    cfg, db, _ = world
    n = 3001
    reads = pg.Reads.from_synth(cfg, 0, n)
    rdp = pg.Rdp.from_synth(cfg, 0, n, db)
    return n, classify(pg, db, reads, rdp, 1), classify(pg, db, reads, rdp, 2), classify(pg, db, reads, rdp, 0)


def test_odd_batch_same_results_in_both_modes(plain):
    n, on, off, _ = plain
    assert on["counters"][4] > 20 * n  # a read hits most of its genus
    assert_same(on, off)
    assert len(off["order"]) == 0  # mode 2: no list
    cls = assert_list(on, n)
    assert len(np.unique(cls)) <= 2  # the batch, and its reads with a DUST-masked base


def test_auto_leaves_a_small_batch_alone(plain):
    """3 001 reads against 4.5 Mbp are far below both thresholds of the auto rule: today's launch, no list."""
    n, on, _, auto = plain
    assert len(auto["order"]) == 0 and len(auto["keys"]) == 0
    assert_same(on, auto)


def test_key_points_at_a_subject_the_read_hits(plain, world):
    """Of the reads with a hit, at least 0.75 must carry the bin of one of their own hit subjects, or a neighbour bin.  The
    first probe of the read's strand is intact with probability 0.99^16 = 0.85, the second-probe rule only adds to that, chance
    buckets are negligible in 4.5 Mbp, and the margin covers the sampling noise of 3 000 reads."""
    cfg, db, _ = world
    n, on, _, _ = plain
    n = 3000
    shift = order_shift(db.num_bases)
    key_of = np.zeros(n + 1, dtype=np.int64)
    key_of[on["order"]] = on["keys"] & 0xFFFF
    rows = on["rows"][on["rows"]["read"] < n]
    lo = (rows["subject"].astype(np.int64) * cfg.seq_len >> shift) - 1
    hi = ((rows["subject"].astype(np.int64) + 1) * cfg.seq_len - 1 >> shift) + 1
    k = key_of[rows["read"]]
    good = np.zeros(n, dtype=bool)
    np.logical_or.at(good, rows["read"], (k >= lo) & (k <= hi))
    has_hit = np.zeros(n, dtype=bool)
    has_hit[rows["read"]] = True
    frac = good[has_hit].sum() / has_hit.sum()
    print("reads with a hit: %d, key on a hit subject: %.4f" % (has_hit.sum(), frac))
    assert has_hit.sum() > 2900
    assert frac >= 0.75


def test_one_read_and_no_read(pg, world):
    cfg, db, _ = world
    reads = pg.Reads.from_synth(cfg, 17, 1)
    rdp = pg.Rdp.from_synth(cfg, 17, 1, db)
    on, off = classify(pg, db, reads, rdp, 1), classify(pg, db, reads, rdp, 2)
    assert on["counters"][4] > 0
    assert_same(on, off)
    assert_list(on, 1)
    empty = pg.Reads.from_fasta_text(b"")
    assert len(empty) == 0
    for mode in (1, 2):
        res = blast(pg, db, empty, mode)
        assert len(res["order"]) == 0 and len(res["rows"]) == 0 and res["counters"] == (0, 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ mixed batches
def mixed_records(pg, cfg, rng):
    """Reads of every kind the seed stage tells apart: 150-base reads of both strands, reads that are not from the database,
    reads under 16 and under 28 bases, reads with a homopolymer (the DUST class), 250- and 600-base reads (five flag words; one
    read per wavefront)."""
    recs = []
    base = pg.Reads.from_synth(cfg, 0, 900)
    for i in range(900):
        s = letters(base, i)
        if i % 9 == 1:
            s = "".join(rng.choice(list("ACGT"), size=150))  # not from the database: no hit, the last bin
        elif i % 9 == 2:
            s = s[:int(rng.integers(1, 16))]
        elif i % 9 == 3:
            s = s[:int(rng.integers(16, 28))]
        elif i % 9 == 4:
            p = int(rng.integers(20, 100))
            s = s[:p] + "A" * 30 + s[p + 30:]
        elif i % 9 == 5:
            s = "T" * 12 + s[12:]  # the homopolymer over the first probe
        recs.append(s)
    for read_len, count in ((250, 151), (600, 77)):
        c = pg.SynthCfg.default(n_seq=cfg.n_seq, n_genus=cfg.n_genus, read_len=read_len)
        long_reads = pg.Reads.from_synth(c, 0, count)
        recs += [letters(long_reads, i) for i in range(count)]
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def fasta(recs):
    return "".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(recs)).encode()


def test_mixed_classes_with_dust_inside_the_search(pg, world):
    cfg, db, _ = world
    rng = np.random.default_rng(31)
    recs = mixed_records(pg, cfg, rng)
    reads = pg.Reads.from_fasta_text(fasta(recs))
    n = len(reads)
    assert n == len(recs) == 1128
    rdp = pg.Rdp.from_synth(cfg, 0, n, db)
    db.set_dust_each_search(True)
    try:
        on, off = classify(pg, db, reads, rdp, 1), classify(pg, db, reads, rdp, 2)
    finally:
        db.set_dust_each_search(False)
    assert_same(on, off)
    cls = assert_list(on, n)
    # classes: flag words (<= 192, <= 320, longer) x masked or not -- each class of the list holds reads of one kind
    length = np.array([len(s) for s in recs])
    kind = np.where(length <= 192, 0, np.where(length <= 320, 1, 2))
    assert len(np.unique(cls)) >= 4
    for c in np.unique(cls):
        assert len(np.unique(kind[on["order"][cls == c]])) == 1
    # the planted homopolymers put their reads into the DUST class of the short reads: one class, and not the only short one
    planted = np.flatnonzero(np.array(["A" * 30 in s or s.startswith("T" * 12) for s in recs]) & (length <= 192))
    cls_of = np.zeros(n, dtype=np.int64)
    cls_of[on["order"]] = cls
    assert len(planted) >= 150 and len(np.unique(cls_of[planted])) == 1
    assert np.any((kind == 0) & (cls_of != cls_of[planted[0]]))
    # reads without a usable probe carry the last bin
    last_bin = ((db.num_bases - 1) >> order_shift(db.num_bases)) + 1
    key_of = np.zeros(n, dtype=np.int64)
    key_of[on["order"]] = on["keys"] & 0xFFFF
    assert np.all(key_of <= last_bin)
    assert np.all(key_of[length < 16] == last_bin)
    # ... and so do reads that are not from the database, unless a probe meets a bucket by chance: this index hashes
    # 4.5 M postings into 2^25 buckets, a random 16-mer finds one non-empty with probability 1 - e^-0.134 = 0.125, and the key
    # is the last bin when all four probes find none: e^-0.536 = 0.585 of 100 reads (sigma 0.05)
    foreign = np.array([i for i, s in enumerate(recs) if len(s) == 150 and on["cnt"][i] == 0 and "A" * 30 not in s])
    frac = np.mean(key_of[foreign] == last_bin)
    print("reads without a hit: %d, in the last bin: %.3f" % (len(foreign), frac))
    assert len(foreign) >= 95 and frac >= 0.4

def test_mate_joined_reads_are_ordered_piece_by_piece(pg, world):
    """Mates joined by a run of N's are searched as pieces: the list then names pieces, and the hits go back to the reads."""
    cfg, db, _ = world
    base = pg.Reads.from_synth(cfg, 5000, 802)
    recs = []
    for i in range(401):
        a, b = letters(base, 2 * i), letters(base, 2 * i + 1)
        recs.append(a + "N" * 100 + b if i % 4 else a)
    reads = pg.Reads.from_fasta_text(fasta(recs))
    n = len(reads)
    rdp = pg.Rdp.from_synth(cfg, 0, n, db)
    on, off = classify(pg, db, reads, rdp, 1), classify(pg, db, reads, rdp, 2)
    assert_same(on, off)
    n_pieces = sum(2 if i % 4 else 1 for i in range(401))
    assert_list(on, n_pieces)
    assert on["counters"][4] > 20 * n


# ------------------------------------------------------------------------------------------------ file-built databases
def family_db(rng, n_fam, per_fam, length, subs):
    anc = rng.integers(0, 4, size=(n_fam, length), dtype=np.uint8)
    subj = np.repeat(anc, per_fam, axis=0)
    rows = np.arange(subj.shape[0])[:, None]
    pos = np.argsort(rng.random((subj.shape[0], length)), axis=1)[:, :subs]
    subj[rows, pos] = (subj[rows, pos] + rng.integers(1, 4, size=pos.shape, dtype=np.uint8)) % 4
    return anc, subj


def family_reads(rng, anc, n, read_len, subs):
    fam = rng.integers(0, anc.shape[0], size=n)
    start = rng.integers(0, anc.shape[1] - read_len + 1, size=n)
    w = anc[fam[:, None], start[:, None] + np.arange(read_len)[None, :]]
    rows = np.arange(n)[:, None]
    p = rng.integers(0, read_len, size=(n, subs))
    w[rows, p] = (w[rows, p] + rng.integers(1, 4, size=(n, subs), dtype=np.uint8)) % 4
    w[1::2] = 3 - w[1::2, ::-1]
    return [r.tobytes().decode() for r in ACGT[w]]


def write_db(path, texts):
    with open(path, "wb") as f:
        for i, s in enumerate(texts):
            f.write(b">gi|%d|x|c%d|\n%s\n" % (i + 1, i, s))


def test_database_with_iupac_letters(pg, tmp_path):
    rng = np.random.default_rng(77)
    anc, subj = family_db(rng, 40, 20, 600, 12)
    texts = []
    for i, s in enumerate(subj):
        t = bytearray(ACGT[s].tobytes())
        if i % 3 == 0:
            for p in rng.integers(0, 600, size=3):
                t[p] = b"RYKMSWN"[int(rng.integers(0, 7))]
        texts.append(bytes(t))
    write_db(tmp_path / "db.fa", texts)
    db = pg.Db.from_fasta(str(tmp_path / "db.fa"))
    assert db.shape()[2]  # ambiguity letters
    reads = pg.Reads.from_fasta_text(fasta(family_reads(rng, anc, 1501, 150, 2)))
    on, off = blast(pg, db, reads, 1), blast(pg, db, reads, 2)
    assert on["counters"][4] > 10 * 1501
    assert_same(on, off)
    assert_list(on, 1501)


def test_first_call_of_a_fresh_handle_repeats_its_step(pg, tmp_path):
    """30 families of 60 copies: 3 000 reads x 60 rows against a first hit table of 36 rows a read, so the first search through
    a fresh handle repeats its step (tests/test_gpu_capacity.py).  The list is made ahead of the attempts and serves both."""
    rng = np.random.default_rng(1101)
    anc, subj = family_db(rng, 30, 60, 300, 3)
    write_db(tmp_path / "db.fa", [ACGT[s].tobytes() for s in subj])
    reads = pg.Reads.from_fasta_text(fasta(family_reads(rng, anc, 3000, 150, 2)))
    res = []
    for mode in (1, 2):
        db = pg.Db.from_fasta(str(tmp_path / "db.fa"))  # fresh: its tables are first guesses
        res.append(blast(pg, db, reads, mode))
        assert res[-1]["st"].attempts > 1 and res[-1]["st"].grown & 8, (mode, res[-1]["st"].attempts, res[-1]["st"].grown)
    assert_same(res[0], res[1])
    assert_list(res[0], 3000)
