"""GPU: argument, I/O and limit errors that the host checks before or between device calls.  Each case returns its status,
hands out no handle, and leaves the process able to make the next valid call.  The verbs that hand back a log text give
the same status and the same text on a missing input as before (the values are stated here)."""
import ctypes as C
import os
import shutil

import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_IO, E_LIMIT = -1, -2, -7
SHAPE = dict(n_seq=1200, seq_len=400, n_genus=30, read_len=150)


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


@pytest.fixture(scope="module")
def cfg(pg):
    return pg.SynthCfg.default(**SHAPE)


@pytest.fixture(scope="module")
def synth_taxdir(tmp_path_factory, pg, cfg):
    d = tmp_path_factory.mktemp("etax") / "Tax_class"
    d.mkdir()
    assert pg.lib().pgx_synth_write_taxdump(C.byref(cfg), str(d).encode()) == 0
    pg.TaxDb.create(str(d))
    return d


@pytest.fixture(scope="module")
def gold_taxdb(tmp_path_factory, pg, gold):
    d = tmp_path_factory.mktemp("gtax") / "Tax_class"
    d.mkdir()
    for n in ("nodes.dmp", "names.dmp", "gi_taxid_nucl.dmp"):
        shutil.copy(os.path.join(gold, "tax", n), d / n)
    pg.TaxDb.create(str(d))
    with pg.TaxDb.open(str(d)) as db:
        yield db


def _status_and_handle(call, *args):
    p = C.c_void_p()
    return call(*args, C.byref(p)), p.value


def _status_and_text(pg, name, *args):
    from pangea_plus_amd import _capi
    text = C.c_void_p()
    rc = getattr(pg.lib(), name)(*args, C.byref(text))
    return rc, _capi._take_text(text.value)


def _last_error(pg):
    return pg.lib().pgx_last_error().decode()


def test_synthetic_batch_over_the_word_limit(pg, cfg):
    """150-base reads take 8 words each: 2^29 of them are 2^32 words, refused before anything is allocated."""
    rc, p = _status_and_handle(pg.lib().pgx_reads_from_synth, C.byref(cfg), 0, 1 << 29)
    assert (rc, p) == (E_LIMIT, None)
    assert "more than 2^32 words" in _last_error(pg)
    with pg.Reads.from_synth(cfg, 0, 500) as reads:
        assert len(reads) == 500


def test_taxonomy_directory_without_binaries(pg, tmp_path, synth_taxdir):
    (tmp_path / "empty").mkdir()
    rc, p = _status_and_handle(pg.lib().pgx_tax_open, str(tmp_path / "empty").encode())
    assert (rc, p) == (E_IO, None)
    assert "taxonomy binaries missing" in _last_error(pg)
    with pg.TaxDb.open(str(synth_taxdir)) as tax:
        assert tax.ptr


def test_rdp_import_errors(pg, cfg, synth_taxdir, tmp_path):
    rdp_file = tmp_path / "rdp.txt"
    rdp_file.write_text("")
    with pg.Db.from_synth(cfg) as db, pg.Reads.from_synth(cfg, 0, 200) as reads:
        # before bind_taxonomy: refused, whether or not the file is there
        rc, p = _status_and_handle(pg.lib().pgx_rdp_from_file, str(rdp_file).encode(), reads.ptr, db.ptr)
        assert (rc, p) == (E_ARG, None)
        with pg.TaxDb.open(str(synth_taxdir)) as tax:
            db.bind_taxonomy(tax)
        missing = str(tmp_path / "missing.txt")
        rc, p = _status_and_handle(pg.lib().pgx_rdp_from_file, missing.encode(), reads.ptr, db.ptr)
        assert (rc, p) == (E_IO, None)
        assert _last_error(pg) == "cannot open RDP file " + missing
        with pg.Rdp.from_synth(cfg, 0, 200, db) as rdp:
            assert rdp.ptr


def test_consensus_missing_inputs(pg, gold, tmp_path):
    b = os.path.join(gold, "consensus", "basic.blast.tsv")
    r = os.path.join(gold, "consensus", "basic.rdp.tsv")
    missing = str(tmp_path / "missing.txt")
    o = str(tmp_path / "out.txt")
    for args in ((missing, r, None), (b, missing, None), (b, r, missing)):
        enc = [None if a is None else a.encode() for a in args]
        assert _status_and_text(pg, "pgx_consensus_file", *enc, o.encode()) == (
            E_IO, ("\nLoading input files...\nError: Unable to open %s file.\n" % missing).encode())
        assert _last_error(pg) == "cannot open " + missing
    assert _status_and_text(pg, "pgx_consensus_file", None, r.encode(), None, o.encode()) == (E_ARG, b"")
    log = pg.consensus(b, r, o)
    assert log.replace(o.encode(), b"@OUT@") == open(os.path.join(gold, "consensus", "basic.log.txt"), "rb").read()


def test_taxcollector_missing_input(pg, gold_taxdb, gold, tmp_path):
    missing = str(tmp_path / "missing.tsv")
    o = str(tmp_path / "out.tsv")
    assert _status_and_text(pg, "pgx_taxcollect_file", gold_taxdb.ptr, missing.encode(), o.encode()) == (
        E_IO, ("Error: Unable to open classification results file %s.\n" % missing).encode())
    assert _last_error(pg) == "cannot open " + missing
    inp = os.path.join(gold, "taxcollect", "basic.in.tsv")
    assert gold_taxdb.collect_file(inp, o) == open(os.path.join(gold, "taxcollect", "basic.report.txt"), "rb").read()


def test_megaclust2_missing_inputs(pg, tmp_path):
    from pangea_plus_amd import _capi
    missing = str(tmp_path / "missing.tsv")
    o = str(tmp_path / "out.csv")
    assert _status_and_text(pg, "pgx_megaclust_file", C.byref(_capi._mc_opts(missing, o))) == (E_IO, b"")
    assert _last_error(pg) == "couldn't open infile " + missing
    inp = tmp_path / "in.tsv"
    inp.write_text("q1\tOTU_1\t99.00\t150\t0\t0\t1\t150\t1\t150\t1e-70\t 270\n")
    no_dir = str(tmp_path / "no" / "out.csv")
    assert _status_and_text(pg, "pgx_megaclust_file", C.byref(_capi._mc_opts(str(inp), no_dir))) == (E_IO, b"")
    assert _last_error(pg) == "couldn't open outfile " + no_dir
    assert b"1 hits examined" in pg.megaclust2(str(inp), o)
    assert b"OTU_1,1\n" in open(o, "rb").read()
