"""No-GPU checks of pgx_trim_reads (Trim handed straight to Classify): the symbol is exported and mirrored, the call refuses
to compute without a device, and the usage case -- which returns before any read is touched -- is trim2's."""
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


def outcome(call):
    """What a call gave: ("raised", status), or ("returned", value)."""
    import pangea_plus_amd as pg
    try:
        return "returned", call()
    except pg.PangeaError as e:
        return "raised", e.status


def test_symbol_is_exported_declared_and_mirrored(pg):
    from pangea_plus_amd import _capi
    assert "pgx_trim_reads" in _capi.SYMBOLS
    assert hasattr(pg.lib(), "pgx_trim_reads")
    header = open(os.path.join(ROOT, "include", "pangea_hip.h")).read()
    assert re.search(r"\bint pgx_trim_reads\(const pgx_trim_opts \*o, char \*\*log_text, pgx_reads \*\*out, int \*mode, int \*route\);", header)
    routes = re.search(r"enum \{ PGX_TRIM_ROUTE_NONE = (\d), PGX_TRIM_ROUTE_PACKED = (\d), PGX_TRIM_ROUTE_TEXT = (\d) \};", header)
    assert routes and tuple(int(x) for x in routes.groups()) == (pg.TRIM_ROUTE_NONE, pg.TRIM_ROUTE_PACKED, pg.TRIM_ROUTE_TEXT) == (0, 1, 2)
    assert callable(pg.Reads.from_trim)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is visible")
def test_from_trim_fails_loudly_without_a_device(pg, tmp_path):
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\n" + b"ACGT" * 20 + b"\n+\n" + b"I" * 80 + b"\n")
    with pytest.raises(pg.PangeaError) as e:
        pg.Reads.from_trim(str(fq))
    assert e.value.status == -3


def test_usage_case_is_trim2s(pg):
    """No -a: trim2 prints its usage and makes no FASTA (with a device), or refuses (without one); from_trim does the same."""
    if os.path.exists("/dev/kfd"):
        pg.init(0)
    want = outcome(lambda: pg.trim2(None))
    got = outcome(lambda: pg.Reads.from_trim(None))
    if want[0] == "raised":
        assert got == want
    else:
        messages, fasta, mode = want[1]
        assert fasta is None and messages.startswith(b"Usage: perl trim2.pl")
        assert got == ("returned", (None, messages, mode, pg.TRIM_ROUTE_NONE))
