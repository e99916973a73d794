"""The ordering kernel's two routes against the oracle: rows exactly and in order, consensus records exactly.

`k_sort_consensus<G>` ranks a read's hits in one pass over (subject, score) rows when no read of the wavefront has two
hits on one subject, and builds the full S5 keys (with S3c and the tie pass) only when one has.  The batch below is
hand-made so that both routes, both launches (G = 32 and 64), the hand-over between them and the pass-on to the big-read
path all occur, and `test_the_oracle_rows_hold_every_case` asserts from the oracle's own rows that each case is there:
a generator that stops producing a case fails instead of hiding it.

The database is a set of families.  Every member of a family is the family's 200-base ancestor `P` with a few
substitutions of its own, followed by a 200-base tail `Q` that no other sequence shares.  A 150-base window of a member's
`P` therefore has one row per family member and never two on one subject; a read spliced from a piece of a member's `P`
and a piece of its own `Q` has two rows on that member (two diagonals 110 bases apart) and one on every other member; a
read with one base deleted in the middle has seeds on both sides of the gap that grow into one alignment (S3c drops one).
The expected rows and records come from the oracle chain (blastn, taxcollector, consensus), never from the library.
"""
import os
import random

import numpy as np
import pytest

import consensus_inputs
import consensus_rule
from tax_inputs import write_dumps

P_LEN, Q_LEN, READ_LEN = 200, 200, 150
# family sizes: both edges of each launch, the hand-over through the G = 64 list, one past 64, and the special families
SIZES = [1, 2, 31, 32, 33, 63, 64, 70, 40, 3, 6, 5]
F_40, F_BEST, F_IDENT, F_INDEL = 8, 9, 10, 11   # indices into SIZES of the families the hand-made reads use
COMP = str.maketrans("ACGT", "TGCA")


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _sub(rng, s, p):
    return s[:p] + rng.choice([c for c in "ACGT" if c != s[p]]) + s[p + 1:]


def database(rng):
    """[(gi, family, member, sequence)].  Member j of a family carries 1 + j % 3 substitutions in P[25:175] (so different
    subjects often score the same); the members of F_IDENT carry none (every row of a read has one score)."""
    subj = []
    for f, size in enumerate(SIZES):
        anc = _rand(rng, P_LEN)
        for j in range(size):
            p = anc
            if f == F_BEST:
                p = _sub(rng, p, 75) if j else p       # member 0 is the ancestor; the others differ inside every window
            elif f != F_IDENT:
                for q in rng.sample(range(25, 175), 1 + j % 3):
                    p = _sub(rng, p, q)
            subj.append((1000 + len(subj), f, j, p + _rand(rng, Q_LEN)))
    return subj


def reads(subj, rng):
    """[(kind, family, member, sequence)] in batch order.  G = 32 wavefronts hold reads 2k and 2k+1, so the pairs that
    matter are placed at even indices."""
    mem = {}
    for gi, f, j, s in subj:
        mem.setdefault(f, []).append(s)

    def window(f, j, st=None):
        st = rng.randint(0, P_LEN - READ_LEN) if st is None else st
        return mem[f][j][st:st + READ_LEN]

    def spliced(f, j):      # 90 bases of P, then 60 bases of the member's own tail 110 bases further on
        return mem[f][j][30:120] + mem[f][j][230:290]

    def deleted(f, j):      # one base of P missing in the middle: 75 + 75 bases around a gap
        s = mem[f][j]
        return s[20:95] + s[96:171]

    out = []

    def add(kind, f, j, seq, flip=None):
        flip = rng.random() < 0.5 if flip is None else flip
        out.append((kind, f, j, seq.translate(COMP)[::-1] if flip else seq))

    add("n32", 3, 0, window(3, 0))                     # 0, 1: a read of 32 rows with a read of none in its wavefront
    add("none", -1, -1, _rand(rng, READ_LEN))
    add("best", F_BEST, 0, spliced(F_BEST, 0))         # 2, 3: a repeat whose partner has none (the slow route serves both)
    add("partner", 1, 1, window(1, 1))
    add("drop", F_INDEL, 2, deleted(F_INDEL, 2))       # 4, 5: S3c drops a row; two repeats in one wavefront
    add("stay", 2, 5, spliced(2, 5))
    add("rep40", F_40, 7, spliced(F_40, 7))            # 6: a repeat among the 33-64-row reads (40 + 1 rows)
    add("ident", F_IDENT, 1, window(F_IDENT, 1))       # 7: every row has one score
    for f, size in enumerate(SIZES):                   # plain windows of every family, on both strands
        for k in range(12 if size <= 70 else 4):
            add("plain", f, rng.randrange(size), window(f, rng.randrange(size)))
    for k in range(8):                                 # more repeats and indels scattered among the plain reads
        add("stay", 4 + k % 3, k, spliced(4 + k % 3, k))
        add("drop", k % 3, 0, deleted(k % 3, 0))
    return out


def taxonomy(subj):
    """Seven one-word ranks; the members of a family alternate between two species of two genera."""
    nodes = [(1, 1, "no rank", ""), (2, 1, "superkingdom", "")]
    names = {1: [("root", "", "scientific name")], 2: [("Bacteria", "", "scientific name")]}
    gis = []
    for f in range(len(SIZES)):
        c = chr(97 + f // 26) + chr(97 + f % 26)
        b = 1000 + 100 * f
        spec = [(b + 1, 2, "phylum", "Phy" + c), (b + 2, b + 1, "class", "Cls" + c), (b + 3, b + 2, "order", "Ord" + c),
                (b + 4, b + 3, "family", "Fam" + c), (b + 5, b + 4, "genus", "Gen" + c), (b + 6, b + 4, "genus", "Hgen" + c),
                (b + 11, b + 5, "species", "Gen%s alpha" % c), (b + 12, b + 6, "species", "Hgen%s delta" % c),
                (b + 13, b + 5, "species", "Gen%s beta" % c)]
        for t, p, r, n in spec:
            nodes.append((t, p, r, ""))
            names[t] = [(n, "", "scientific name")]
    for gi, f, j, _ in subj:
        gis.append((gi, 1000 + 100 * f + 11 + (j * 7 + f) % 3))
    return nodes, names, gis


def build(d, oracle_bin, seed=20261017):
    d = str(d)
    rng = random.Random(seed)
    subj = database(rng)
    rd = reads(subj, rng)
    run = consensus_inputs.run
    p = {"db": os.path.join(d, "db.fa"), "reads": os.path.join(d, "reads.fa"), "hits": os.path.join(d, "hits.tsv"),
         "tax": d, "rdp": os.path.join(d, "rdp.tsv"), "class": os.path.join(d, "hits_class.tsv"),
         "cons": os.path.join(d, "consensus.txt"), "kinds": [r[0] for r in rd], "n_reads": len(rd)}
    with open(p["db"], "w") as f:
        f.write("".join(">gi|%d|f%d|m%d|\n%s\n" % (gi, fa, j, s) for gi, fa, j, s in subj))
    with open(p["reads"], "w") as f:
        f.write("".join(">r%d\n%s\n" % (k, r[3]) for k, r in enumerate(rd)))
    with open(os.path.join(d, "subjects.tsv"), "w") as f:
        f.write(consensus_inputs.subject_table(subj))
    run([oracle_bin, "blastn", "-query", p["reads"], "-db", p["db"], "-outfmt", "6", "-out", p["hits"], "-num_threads", "8"])
    write_dumps(d, *taxonomy(subj))
    run([oracle_bin, "tax_class", "-c"], cwd=d)
    run([oracle_bin, "taxcollector", "-f", os.path.join(d, "subjects.tsv"), "-o", os.path.join(d, "subjects_class.tsv"), "-d", d])
    with open(os.path.join(d, "subjects_class.tsv")) as f:
        lin = [l.split("\t")[1] for l in f.read().splitlines()]
    assert len(lin) == len(subj)
    first = {}
    for i, (gi, f, j, _) in enumerate(subj):
        first.setdefault(f, i)
    lines = []
    for k, (kind, f, j, _) in enumerate(rd):
        if k % 23 == 11 or f < 0:
            continue                                    # a read without a line
        # the line names the source's lineage, another member's (the other genus), or nothing that agrees
        mode = ["same", "other", "none"][k % 3]
        target = first[f] + (j if mode != "other" else (j + 1) % SIZES[f])
        lines.append("r%d\t\t\t\t\t" % k + consensus_inputs.rdp_line("T1", lin[target], mode, k, rng))
    with open(p["rdp"], "w") as f:
        f.write("\n".join(lines) + "\n")
    run([oracle_bin, "taxcollector", "-f", p["hits"], "-o", p["class"], "-d", d])
    run([oracle_bin, "consensus", "-b", p["class"], "-r", p["rdp"], "-o", p["cons"]])
    return p


@pytest.fixture(scope="module")
def batch(tmp_path_factory, oracle_bin):
    return build(tmp_path_factory.mktemp("order"), oracle_bin)


def oracle_rows(p):
    """{read number: [(subject, bits, gapopen, qstart, qend)] in the oracle's order}"""
    rows = {}
    for line in open(p["hits"]):
        f = line.rstrip("\n").split("\t")
        rows.setdefault(int(f[0][1:]), []).append((f[1], float(f[11]), int(f[5]), int(f[6]), int(f[7])))
    return rows


def _repeats(rows):
    subj = [r[0] for r in rows]
    return len(set(subj)) < len(subj)


def test_the_oracle_rows_hold_every_case(batch):
    rows = oracle_rows(batch)
    kinds, n = batch["kinds"], batch["n_reads"]
    count = [len(rows.get(k, [])) for k in range(n)]
    plain = [k for k in range(n) if kinds[k] in ("plain", "n32", "partner", "ident")]
    assert not any(_repeats(rows[k]) for k in plain if k in rows)
    # both edges of each launch, the hand-over, and the pass-on from the G = 64 launch -- all without a repeated subject
    for want in (1, 2, 31, 32, 33, 63, 64):
        assert any(count[k] == want for k in plain), want
    assert any(count[k] > 64 for k in plain)
    # a read of 32 rows and a read of none in one G = 32 wavefront
    assert (count[0], count[1]) == (32, 0)
    # two different subjects with one score; a read whose rows all have one score
    assert any(a[0] != b[0] and a[1] == b[1] for k in plain if k in rows for a, b in zip(rows[k], rows[k][1:]))
    ident = rows[kinds.index("ident")]
    assert len(ident) == SIZES[F_IDENT] and len({r[1] for r in ident}) == 1 and not _repeats(ident)
    # two rows on one subject, both kept
    stay = [k for k in range(n) if kinds[k] in ("stay", "best", "rep40") and _repeats(rows[k])]
    assert len(stay) >= 4
    # the repeating subject's best score moves its lower row ahead of another subject's higher row
    best = rows[kinds.index("best")]
    assert [r[0] for r in best][:2] == [best[0][0]] * 2 and best[2][0] != best[0][0] and best[1][1] < best[2][1] < best[0][1]
    # that read's partner in the wavefront has no repeat and stays in the G = 32 launch
    kb = kinds.index("best")
    assert kb % 2 == 0 and kinds[kb + 1] == "partner" and 0 < count[kb + 1] <= 32 and count[kb] <= 32
    # S3c: one gapped row that spans the deleted base stands for the seeds on both sides of it
    drops = [k for k in range(n) if kinds[k] == "drop" and any(r[2] >= 1 and r[3] <= 40 and r[4] >= 110 for r in rows[k])]
    assert len(drops) >= 4
    assert all(not _repeats(rows[k]) for k in drops)
    # a repeat among the reads of 33-64 rows
    k40 = kinds.index("rep40")
    assert 33 <= count[k40] <= 64 and _repeats(rows[k40])


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


@pytest.fixture(scope="module")
def device(pg, batch):
    db = pg.Db.from_fasta(batch["db"])
    db.bind_taxonomy(pg.TaxDb.open(batch["tax"]))
    reads = pg.Reads.from_fasta(batch["reads"])
    assert len(reads) == batch["n_reads"]
    return db, reads, pg.Rdp.from_file(batch["rdp"], reads, db)


@pytest.mark.gpu
def test_rows_match_the_oracle_without_records(pg, batch, device):
    from pangea_plus_amd import _capi
    db, reads, rdp = device
    want = open(batch["hits"], "rb").read()
    assert _capi.blast_search(db, reads).format(db, reads) == want
    hits, recs = _capi.classify_consensus(db, reads, rdp, want_records=False)
    assert recs is None
    assert hits.format(db, reads) == want
    # the reads whose gapped row stands for two seeds: the device's table holds the dropped slots behind the kept rows
    n = batch["n_reads"]
    slots, kept = np.diff(hits.read_offsets(n)), hits.read_counts(n)
    dropped = {k for k in range(n) if slots[k] > kept[k]}
    assert len([k for k in dropped if batch["kinds"][k] == "drop"]) >= 4


@pytest.mark.gpu
def test_rows_and_records_match_the_oracle(pg, batch, device):
    from pangea_plus_amd import _capi
    db, reads, rdp = device
    n = batch["n_reads"]
    hits, recs = _capi.classify_consensus(db, reads, rdp)
    assert hits.format(db, reads) == open(batch["hits"], "rb").read()
    want = open(batch["cons"], "rb").read()
    assert _capi.consensus_format(db, reads, hits, recs) == want
    # record by record: the row within the read and the agreement count, from the restatement of the script on the
    # oracle's annotated table (its text is the oracle's)
    text, _, rule = consensus_rule.consensus(open(batch["class"], "rb").read(), open(batch["rdp"], "rb").read(),
                                             v=consensus_rule.PERL)
    assert text == want
    cnt = hits.read_counts(n)
    first = np.concatenate(([0], np.cumsum(cnt)))      # rows before the read in the table's text
    rows = hits.rows(n)
    slot_off = hits.read_offsets(n)
    printed = np.zeros(n, dtype=bool)
    for r in rule:
        k = int(r.read[1:])
        printed[k] = True
        assert (int(recs["hit"][k]) - int(slot_off[k]), int(recs["matches"][k])) == (r.row, r.matches), (k, batch["kinds"][k])
    assert len(rule) > n // 2
    assert (recs["hit"][~printed] == -2).all()
    assert rows is not None and first[-1] == len(open(batch["hits"]).readlines())
    # the records alone (no table kept) are the same records
    _, recs_only = _capi.classify_consensus(db, reads, rdp, want_hits=False)
    assert (recs_only == recs).all()
