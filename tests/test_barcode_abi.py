"""No-GPU checks of the barcode demultiplexer: the symbols are declared, exported and mirrored, the entry points refuse to
compute without a device, and what ends before any file is touched -- the usage lines, a missing -d -- needs none."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("pgx_barcode_file", "pgx_barcode_reads", "pgx_barcodes_count", "pgx_barcodes_name", "pgx_barcodes_letters",
         "pgx_barcodes_reads", "pgx_barcodes_sequences", "pgx_barcodes_no_barcode", "pgx_barcodes_thrown_out",
         "pgx_barcodes_take_reads", "pgx_barcodes_free")


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    if not os.path.exists(pg.lib_path) or not hasattr(pg.lib(), "pgx_barcode_file"):
        import importlib.util
        spec = importlib.util.spec_from_file_location("pgx_build", os.path.join(ROOT, "pangea-plus_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build_all()
    return pg


def test_symbols_are_declared_exported_and_mirrored(pg):
    from pangea_plus_amd import _capi
    header = open(os.path.join(ROOT, "include", "pangea_hip.h")).read()
    assert re.search(r"\bint pgx_barcode_file\(int argc, const char \*const \*argv, char \*\*log_text\);", header)
    assert re.search(r"\bint pgx_barcode_reads\(const char \*reads_path, const char \*barcodes_path, pgx_barcodes \*\*out\);", header)
    assert re.search(r"\bint pgx_barcodes_take_reads\(const pgx_barcodes \*b, int64_t i, pgx_reads \*\*out\);", header)
    assert re.search(r"\bvoid pgx_barcodes_free\(pgx_barcodes \*b\);", header)
    for name in NAMES:
        assert name in _capi.SYMBOLS
        assert hasattr(pg.lib(), name)
    assert callable(pg.barcode) and callable(pg.barcode_reads)
    assert os.access(os.path.join(ROOT, "pangea-plus_amd", "bin", "barcode"), os.X_OK)


def test_usage_lines_and_a_missing_d_need_no_device(pg, tmp_path):
    assert pg.barcode(["-s", "a", "-b"]) == b"Please enter the -s sequences and -b barcodes.\n"
    assert pg.barcode(["-s", "a", "-b", "b", "-d", "d", "x"]) == b"Too many inputs\n"
    assert pg.barcode(["-s", "a", "-d", "d"]) == b"Must enter at least -s sequences and -b barcodes.\n"
    with pytest.raises(pg.PangeaError) as e:
        pg.barcode(["-s", "a", "-b", "b", "x"], cwd=str(tmp_path))
    assert e.value.status == -1 and e.value.stdout == b""
    assert os.listdir(str(tmp_path)) == []


def test_null_handles_answer_without_a_device(pg):
    assert pg.lib().pgx_barcodes_count(None) == 0
    assert pg.lib().pgx_barcodes_name(None, 0) is None
    assert pg.lib().pgx_barcodes_reads(None, 0) == -1
    pg.lib().pgx_barcodes_free(None)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is visible")
def test_the_entry_points_fail_loudly_without_a_device(pg, tmp_path):
    (tmp_path / "b.txt").write_bytes(b"A\tACGT\n")
    (tmp_path / "s.fas").write_bytes(b">r\nACGT\n")
    (tmp_path / "d").mkdir()
    with pytest.raises(pg.PangeaError) as e:
        pg.barcode(["-s", "s.fas", "-b", "b.txt", "-d", "d"], cwd=str(tmp_path))
    assert e.value.status == -3
    assert os.listdir(str(tmp_path / "d")) == []
    with pytest.raises(pg.PangeaError) as e:
        pg.barcode_reads(str(tmp_path / "s.fas"), str(tmp_path / "b.txt"))
    assert e.value.status == -3
    # the accessor that computes checks for a device before it looks into its handle (none can exist without one)
    out = C.c_void_p(1)
    assert pg.lib().pgx_barcodes_take_reads(C.c_void_p(1), 0, C.byref(out)) == -3
    assert out.value is None
