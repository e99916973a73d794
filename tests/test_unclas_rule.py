"""tests/unclas_rule.py -- unclassified_selector.pl restated in Python -- against every golden case printed by the
reference's own Perl (tools/gen_goldens_unclas.py): stdout, exit status and the -o file, byte for byte."""
import os
import shutil

import pytest

import unclas_rule
from conftest import GOLD

UNCLAS = os.path.join(GOLD, "unclas")


def cases():
    return sorted(os.listdir(UNCLAS)) if os.path.isdir(UNCLAS) else []


def load_case(name, work):
    """The case's inputs copied into `work` (a run writes its -o file next to them):
    (argv, stdout, status, output file bytes or None)."""
    src = os.path.join(UNCLAS, name)
    for f in ("m.tsv", "s.fas"):
        if os.path.exists(os.path.join(src, f)):
            shutil.copy(os.path.join(src, f), os.path.join(str(work), f))
    argv = open(os.path.join(src, "argv.txt"), "rb").read().decode("latin-1").split("\n")[:-1]
    out = os.path.join(src, "out.fas")
    return (argv, open(os.path.join(src, "stdout.bin"), "rb").read(), int(open(os.path.join(src, "status.txt")).read()),
            open(out, "rb").read() if os.path.exists(out) else None)


def test_the_goldens_are_there():
    assert len(cases()) >= 30
    for must in ("t_equal", "e_equal", "b_equal", "rows_apart_pass_last", "blank_line_mid", "tabs_0", "tabs_1", "tabs_2", "tabs_11",
                 "empty_e_field", "header_description", "dup_classified", "dup_rejected", "gt_inside_sequence", "text_before_header",
                 "crlf", "empty_table", "empty_fasta", "flag_as_value", "flag_last", "args_5", "args_13", "unopenable_m",
                 "unopenable_s", "unopenable_o", "e_abc", "t_empty"):
        assert must in cases()


@pytest.mark.parametrize("name", cases())
def test_rule_equals_the_reference_script(name, tmp_path):
    argv, stdout, status, out = load_case(name, tmp_path)
    assert unclas_rule.run(argv, cwd=str(tmp_path)) == (stdout, status, out)


def test_mask_and_output_agree():
    """keep_mask() is select() record by record (the GPU tests compare the resident form's mask with it)"""
    table = b"a\ts\t99\t1\t1\t1\t1\t1\t1\t1\t1e-50\t250\nb\ts\t50\t1\t1\t1\t1\t1\t1\t1\t1e-50\t250\n"
    fasta = b">a\nAC\n>b\nGG\n>a\nTT\n>c\nAA\n"
    t, e, b = unclas_rule.thresholds()
    assert unclas_rule.keep_mask(table, fasta, t, e, b) == [0, 1, 1, 1]
    assert unclas_rule.select(table, fasta, t, e, b) == (b">b \nGG\n>a \nTT\n>c \nAA\n", 3)
    assert unclas_rule.thresholds("100", "5", "0")[1] == pytest.approx(148.4131591025766)
