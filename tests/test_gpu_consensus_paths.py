"""Every form of the device consensus against the Perl selection rule (Consensus_BLAST_SOAP_RDP-1.1.pl:141-204).

The inputs (tests/consensus_inputs.py) reach each hit-count group (k_sort_consensus<32>, <64>, the big reads'
k_consensus_serial) with each selection form (closed form, successor chain, literal walk, all-zero start), on 32- and
64-byte pair records, records that escape to the general count, the 7x6 and the 15x8 compare grid and the general count
of more than 8 triplets; test_oracle_consensus.py counts the reads of every cell on the CPU.  The 64-bit walk is not
reached: it needs agreement or token counts of 10^8 and more (lineages hold a few dozen tokens) or a pident rank of
2^25 and more (there are about 10 000 pident texts).
"""
import numpy as np
import pytest

import consensus_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


@pytest.fixture(scope="module")
def paths(tmp_path_factory, oracle_bin):
    return consensus_inputs.build(tmp_path_factory.mktemp("paths"), oracle_bin)


def _bound_db(pg, paths, tax):
    db = pg.Db.from_fasta(paths["db"])
    db.bind_taxonomy(pg.TaxDb.open(paths["tax_" + tax]))
    return db


@pytest.mark.parametrize("tax", ["T1", "T2", "T3"])
def test_every_path_gives_the_scripts_answer(pg, paths, tax, tmp_path, monkeypatch):
    from pangea_plus_amd import _capi
    want = open(paths["cons_" + tax], "rb").read()
    rule_text, _, rule_recs, _, _ = consensus_inputs.labelled(paths, tax)
    assert rule_text == want
    db = _bound_db(pg, paths, tax)
    reads = pg.Reads.from_fasta(paths["reads"])
    n = len(reads)
    assert n == paths["n_reads"]
    rdp = pg.Rdp.from_file(paths["rdp_" + tax], reads, db)

    # the fused hot path: hit table, records, text
    hits, recs = _capi.classify_consensus(db, reads, rdp)
    assert hits.format(db, reads) == open(paths["hits"], "rb").read()
    assert _capi.consensus_format(db, reads, hits, recs) == want
    off = hits.read_offsets(n)
    printed = np.zeros(n, dtype=bool)
    for r in rule_recs:
        k = int(r.read[1:])
        printed[k] = True
        assert (int(recs["hit"][k]) - int(off[k]), int(recs["matches"][k])) == (r.row, r.matches), \
            (tax, r.read, r.group, r.form, r.grid)
    assert (recs["hit"][~printed] == -2).all()      # the reads without an RDP line

    # consensus over the existing hit table (k_consensus_serial for every read)
    recs2 = np.zeros(n, dtype=_capi.REC_DTYPE)
    _capi._check(pg.lib().pgx_consensus_batch(db.ptr, hits.ptr, rdp.ptr, recs2.ctypes.data, n))
    assert (recs2 == recs).all()

    # the `consensus` file verb on the oracle's annotated table
    pg.consensus(paths["class_" + tax], paths["rdp_" + tax], str(tmp_path / "c.txt"))
    assert (tmp_path / "c.txt").read_bytes() == want

    # the RDP lines parsed on the host instead of the device
    monkeypatch.setenv("PGX_RDP_HOST", "1")
    rdp_h = pg.Rdp.from_file(paths["rdp_" + tax], reads, db)
    monkeypatch.delenv("PGX_RDP_HOST")
    _, recs_h = _capi.classify_consensus(db, reads, rdp_h, want_hits=False)
    assert (recs_h == recs).all()


@pytest.mark.parametrize("tax", ["T1", "T3"])
def test_batch_cut_in_two_windows_gives_the_whole(pg, paths, tax):
    """The same reads in two windows, each with its own RDP import, joined.  Read 0 of a window starts from
    simrank_undef (the script's undef $blastsim) where the whole batch has "0" there.  That is harmless only because ""
    and "0" both sort below every "%.2f" pident text, so the first row always replaces either."""
    from pangea_plus_amd import _capi
    want = open(paths["cons_" + tax], "rb").read()
    db = _bound_db(pg, paths, tax)
    n = paths["n_reads"]
    parts = []
    for first, count in ((0, n // 2 + 5), (n // 2 + 5, n - n // 2 - 5)):
        reads = pg.Reads.from_fasta(paths["reads"], first, count)
        assert len(reads) == count
        rdp = pg.Rdp.from_file(paths["rdp_" + tax], reads, db)
        hits, recs = _capi.classify_consensus(db, reads, rdp)
        parts.append(_capi.consensus_format(db, reads, hits, recs))
    assert parts[0] and parts[1]
    assert b"".join(parts) == want
