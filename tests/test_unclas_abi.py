"""No-GPU checks of the unclassified-read selector: both symbols are declared, exported and mirrored, both calls refuse to
compute without a device, and the two usage cases -- which end before any file is touched -- print the script's lines."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    if not os.path.exists(pg.lib_path):
        import importlib.util
        spec = importlib.util.spec_from_file_location("pgx_build", os.path.join(ROOT, "pangea-plus_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build_all()
    return pg


def test_symbols_are_declared_exported_and_mirrored(pg):
    from pangea_plus_amd import _capi
    header = open(os.path.join(ROOT, "include", "pangea_hip.h")).read()
    assert re.search(r"\bint pgx_unclas_file\(int argc, const char \*const \*argv, char \*\*log_text\);", header)
    assert re.search(r"typedef struct \{\s*const char \*t, \*e, \*b;\s*\} pgx_unclas_opts;", header)
    assert re.search(r"\bint pgx_unclassified_batch\(pgx_db \*db, const pgx_reads \*reads, const pgx_hits \*hits, const pgx_unclas_opts \*o, "
                     r"uint8_t \*mask_out,\s*int64_t cap, int64_t \*n_selected, pgx_reads \*\*out\);", header)
    for name in ("pgx_unclas_file", "pgx_unclassified_batch"):
        assert name in _capi.SYMBOLS
        assert hasattr(pg.lib(), name)
    assert [f[0] for f in _capi._UnclasOpts._fields_] == ["t", "e", "b"]
    assert callable(pg.unclassified_selector) and callable(pg.unclassified)
    assert os.access(os.path.join(ROOT, "pangea-plus_amd", "bin", "unclassified_selector"), os.X_OK)


def test_usage_lines_need_no_device(pg):
    assert pg.unclassified_selector(["-m", "a", "-s", "b", "-o"]).startswith(b"Please enter the -m megablast")
    assert pg.unclassified_selector(["-m", "a", "-s", "b", "-t", "95"]) == b"Must have at least -m megablast -s sequences -o output file.\n"


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is visible")
def test_both_calls_fail_loudly_without_a_device(pg, tmp_path):
    (tmp_path / "m.tsv").write_bytes(b"")
    (tmp_path / "s.fas").write_bytes(b">r\nACGT\n")
    with pytest.raises(pg.PangeaError) as e:
        pg.unclassified_selector(["-m", "m.tsv", "-s", "s.fas", "-o", "out.fas"], cwd=str(tmp_path))
    assert e.value.status == -3
    assert not (tmp_path / "out.fas").exists()
    # the resident form checks for a device before it looks into its handles (none can exist without one)
    n_sel = C.c_int64(-1)
    handle = C.c_void_p(1)
    assert pg.lib().pgx_unclassified_batch(handle, handle, handle, None, None, 0, C.byref(n_sel), None) == -3
    assert n_sel.value == 0
