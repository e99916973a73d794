"""tests/barcode_rule.py -- Barcode/barcode.pl restated in Python -- against every golden case printed by the reference's
own Perl (tools/gen_goldens_barcode.py): stdout, exit status and every file of the -d directory, byte for byte; a refused
case gives its refusal and nothing else."""
import os
import shutil

import pytest

import barcode_rule
from conftest import GOLD

BARCODE = os.path.join(GOLD, "barcode")


def cases():
    return sorted(os.listdir(BARCODE)) if os.path.isdir(BARCODE) else []


def load_case(name, work):
    """The case's inputs copied into `work`, with an empty directory `d` next to them:
    (argv, stdout, status, {file name: bytes} or None); status is an int, or the name of the refusal."""
    src = os.path.join(BARCODE, name)
    for f in ("reads.fas", "barcodes.txt"):
        if os.path.exists(os.path.join(src, f)):
            shutil.copy(os.path.join(src, f), os.path.join(str(work), f))
    os.mkdir(os.path.join(str(work), "d"))
    argv = open(os.path.join(src, "argv.txt"), "rb").read().decode("latin-1").split("\n")[:-1]
    status = open(os.path.join(src, "status.txt")).read().strip()
    if status.startswith("E_"):
        return argv, b"", status, None
    files = None
    if os.path.isdir(os.path.join(src, "d")):
        files = {os.fsencode(f): open(os.path.join(src, "d", f), "rb").read() for f in os.listdir(os.path.join(src, "d"))}
    return argv, open(os.path.join(src, "stdout.bin"), "rb").read(), int(status), files


def test_the_goldens_are_there():
    assert len(cases()) >= 50
    for must in ("prefix_line1", "substring_line1_file_order", "prefix_of_other_short_first", "prefix_of_other_long_first",
                 "prefix_line2", "substring_line2", "substring_line3", "split_across_break", "lowercase_read", "bases_99",
                 "bases_100", "first_line_100_long", "gt_not_in_column_1", "gt_inside_sequence", "header_only",
                 "empty_sequence_file", "empty_barcode_file", "one_record", "last_predecessor_shorter",
                 "last_predecessor_longer", "refuse_last_second_prefix", "crlf", "no_final_newline", "info_101_and_100",
                 "refuse_no_d", "refuse_line_without_tab", "refuse_empty_name", "refuse_empty_letters",
                 "refuse_letters_not_alphabetic", "refuse_name_with_slash", "refuse_name_with_nul", "refuse_name_twice",
                 "refuse_text_before_first_header", "refuse_65_letters", "args_3", "args_7", "unopenable_s", "unopenable_b"):
        assert must in cases()


@pytest.mark.parametrize("name", cases())
def test_rule_equals_the_reference_script(name, tmp_path):
    argv, stdout, status, files = load_case(name, tmp_path)
    assert barcode_rule.run(argv, cwd=str(tmp_path)) == (stdout, status, files)


def test_a_file_of_one_read_never_yields_that_read(tmp_path):
    """the last record's sum of line lengths runs to the line count of the record before it: 0 here"""
    _, _, _, files = load_case("one_record", tmp_path)
    assert files[b"barA.fas"] == b"" and files[b"nobar.fas"] == b""
    assert files[b"barcode_count.txt"] == b"01\tACGTACGT\t0\n02\tTTGGCCAA\t0\n"


def test_fates_are_reported_per_record():
    bars = barcode_rule.parse_barcodes(b"A\tACGTACGT\n")
    g = b"G" * 60 + b"\n"
    text = (b">a\nACGTACGT" + b"G" * 52 + b"\n" + g + b">b\n" + g + b"ACGTACGT" + b"G" * 52 + b"\n" + g + b">c\n" + g + b"GGACGTACGT\n" + g + g
            + b">d\n" + g + b">e\nACGTACGT\n>tail\nCC\n")
    assert barcode_rule.fates(bars, text) == [
        (barcode_rule.KEPT, 0, 1, 113), (barcode_rule.KEPT, 0, 1, 175), (barcode_rule.KEPT, 0, 2, 172),
        (barcode_rule.NOBAR, -1, 0, 0), (barcode_rule.THROWN, 0, 1, 52), (barcode_rule.NOBAR, -1, 0, 0)]
