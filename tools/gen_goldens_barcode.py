"""Golden vectors for Barcode/barcode.pl, printed by the reference's own Perl script, and a sweep of
tests/barcode_rule.py against it.

Runs on a machine that holds the reference tree and perl; no test imports it.  Each case is a directory
tests/golden/barcode/<case>/ with
  argv.txt     the script's @ARGV, one word per line (file names are relative to the case directory; -d is always `d`)
  reads.fas barcodes.txt   the two inputs, where the case has them
  status.txt   the script's exit status -- or `E_ARG` / `E_LIMIT` / `E_REFHANG` for an input the project refuses;
               the Perl is not run on those, except the two on which it never ends: the tool checks that it does not
  stdout.bin   what the script printed on stdout (not for refused cases)
  d/           every file the script left in its -d directory
usage: python3 tools/gen_goldens_barcode.py --root REFERENCE [--sweep N [--seed S] [--jobs J]]
  --sweep N: N random inputs through the Perl and through the rule; both must agree byte for byte (stdout, status, every
  file).  Where the rule says the script never ends, the Perl must still be running after two seconds.  Writes no golden.
"""
import argparse
import concurrent.futures
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "..", "tests", "golden", "barcode")
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

STD = ["-s", "reads.fas", "-b", "barcodes.txt", "-d", "d"]
A, B = "ACGTACGT", "TTGGCCAA"
AB = "A\t%s\nB\t%s\n" % (A, B)
G60 = "G" * 60
TAIL = ">tail\nCCCC\n"  # the last record of a file goes another way; this one keeps it off the read under test


def rec(name, *lines):
    return ">" + name + "\n" + "".join(ln + "\n" for ln in lines)


def pre(bc, n=60):
    return bc + "G" * (n - len(bc))


def many(bc, name, n):
    return "".join(rec("%s%d" % (name, i), bc, "G" * 43) for i in range(n))


# case -> (argv, barcode file text or None, sequence file text or None, "" or the refusal, True when the Perl never ends)
CASES = {
    "prefix_line1": (STD, AB, rec("r1", pre(A), G60, G60) + rec("r2", pre(B), G60, G60) + TAIL),
    "substring_line1_file_order": (STD, AB, rec("r1", "GG" + B + "GG" + A + "G" * 40, G60, G60) + TAIL),
    "prefix_of_other_short_first": (STD, "S\tACGT\nL\tACGTAC\n", rec("r1", pre("ACGTAC"), G60, G60) + rec("r2", "GG" + pre("ACGTAC", 58), G60, G60) + TAIL),
    "prefix_of_other_long_first": (STD, "L\tACGTAC\nS\tACGT\n", rec("r1", pre("ACGTAC"), G60, G60) + rec("r2", pre("ACGTGG"), G60, G60) + TAIL),
    "prefix_line2": (STD, AB, rec("r1", G60, pre(A), G60) + TAIL),
    "prefix_line3": (STD, AB, rec("r1", G60, G60, pre(A), G60) + TAIL),
    "substring_line2": (STD, AB, rec("r1", G60, "GGG" + pre(A, 57), G60, G60) + TAIL),
    "substring_line3": (STD, AB, rec("r1", G60, G60, "GGG" + pre(B, 57), G60, G60) + TAIL),
    "split_across_break": (STD, AB, rec("r1", "G" * 56 + "ACGT", "ACGT" + "G" * 56, G60) + TAIL),
    "lowercase_read": (STD, AB, rec("r1", pre(A.lower()), G60, G60) + rec("r2", pre(A), G60.lower(), G60) + TAIL),
    "lowercase_barcode_file": (STD, "a\tacgtacgt \nb\tTtGgCcAa\n", rec("r1", pre(A), G60, G60) + rec("r2", pre(B), G60, G60) + TAIL),
    "bases_99": (STD, AB, rec("r1", pre(A), "G" * 46) + TAIL),
    "bases_100": (STD, AB, rec("r1", pre(A), "G" * 47) + TAIL),
    "first_line_100_long": (STD, AB, rec("r1", pre(A, 100), "G" * 46) + rec("r2", pre(A, 100), "G" * 47) + TAIL),
    "first_line_18_long": (STD, AB, rec("r1", pre(A, 18), "G" * 47) + rec("r2", pre(A, 18), "G" * 46) + TAIL),
    "gt_not_in_column_1": (STD, AB, "ab>cd e\n" + pre(A) + "\n" + G60 + "\n" + TAIL),
    "gt_inside_sequence": (STD, AB, rec("r1", pre(A), "GGG>GGG", G60, G60) + TAIL),
    "header_only": (STD, AB, ">r1\n>r2\n" + pre(A) + "\n" + G60 + "\n>r3\n" + TAIL),
    "blank_lines": (STD, AB, "\n" + rec("r1", pre(A), "", G60, "", "") + "\n" + rec("r2", "", G60, pre(B), G60) + TAIL + "\n"),
    "empty_sequence_file": (STD, AB, ""),
    "empty_barcode_file": (STD, "", rec("r1", pre(A), G60, G60) + TAIL),
    "both_empty": (STD, "", ""),
    "one_record": (STD, AB, rec("r1", pre(A), G60, G60, G60)),
    "one_record_no_barcode": (STD, AB, rec("r1", G60, G60)),
    "last_predecessor_shorter": (STD, AB, rec("r0", pre(A), G60) + rec("r1", pre(A), G60, G60, G60)),
    "last_predecessor_longer": (STD, AB, rec("r0", pre(A), G60, G60, G60, G60) + rec("r1", pre(A), G60)),
    "last_predecessor_longer_substring": (STD, AB, rec("r0", G60, G60, G60, G60) + rec("r1", G60, "GG" + pre(B, 58), G60, G60)),
    "last_substring_line1_short_predecessor": (STD, AB, rec("r0") + rec("r1", "GG" + pre(B, 58), G60, G60)),
    "last_line_is_0": (STD, AB, rec("r0", pre(A), G60) + ">r1\n" + pre(A) + "\n" + G60 + "\n0"),
    "crlf": (STD, AB.replace("\n", "\r\n"), (rec("r1", pre(A), G60, G60) + "\n" + rec("r2", G60, pre(B), G60) + TAIL).replace("\n", "\r\n")),
    "no_final_newline": (STD, AB[:-1], rec("r1", pre(A), G60, G60) + rec("r2", pre(B), G60, G60)[:-1]),
    "info_101_and_100": (STD, "H\tACG\nI\tTTG\nJ\tCCA\n", many("ACG", "h", 100) + many("TTG", "i", 101) + many("CCA", "j", 3) + TAIL),
    "info_min_is_a_line_count": (STD, AB, rec("r1", pre(A), G60, G60) + TAIL),
    "ten_barcodes": (STD, "".join("n%d\t%s\n" % (i, "ACGT"[i % 4] * 3 + "ACGT"[i // 4] * 3) for i in range(11)), rec("r1", pre("GGGTTT"), G60, G60) + TAIL),
    "name_with_blanks": (STD, "my sample \t%s\n" % A, rec("r1 desc", pre(A), G60, G60) + TAIL),
    "args_3": (["-s", "reads.fas", "-b"], AB, TAIL),
    "args_7": (STD + ["x"], AB, TAIL),
    "no_b_option": (["-s", "reads.fas", "-d", "d"], AB, TAIL),
    "flag_last": (["-b", "barcodes.txt", "-d", "d", "x", "-s"], AB, TAIL),
    "unopenable_s": (["-s", "absent.fas", "-b", "barcodes.txt", "-d", "d"], AB, None),
    "unopenable_b": (["-s", "reads.fas", "-b", "absent.txt", "-d", "d"], None, TAIL),
    # refused rather than guessed
    "refuse_no_d": (["-s", "reads.fas", "-b", "barcodes.txt"], AB, TAIL, "E_ARG"),
    "refuse_d_is_last_word": (["-s", "reads.fas", "-b", "barcodes.txt", "-d"], AB, TAIL, "E_ARG"),
    "refuse_line_without_tab": (STD, "A " + A + "\n", TAIL, "E_ARG"),
    "refuse_blank_line_in_barcodes": (STD, AB + "\n", TAIL, "E_ARG"),
    "refuse_empty_name": (STD, "\t" + A + "\n", TAIL, "E_ARG"),
    "refuse_empty_letters": (STD, "A\t \n", TAIL, "E_ARG"),
    "refuse_letters_not_alphabetic": (STD, "A\tAC.T\n", TAIL, "E_ARG"),
    "refuse_second_tab": (STD, "A\tACGT\tx\n", TAIL, "E_ARG"),
    "refuse_name_with_slash": (STD, "a/b\t" + A + "\n", TAIL, "E_ARG"),
    "refuse_name_with_nul": (STD, "a\0b\t" + A + "\n", TAIL, "E_ARG"),
    "refuse_name_twice": (STD, "A\t%s\nA\t%s\n" % (A, B), TAIL, "E_ARG"),
    "refuse_text_before_first_header": (STD, AB, "stray\n" + TAIL, "E_ARG"),
    "refuse_65_letters": (STD, "A\t" + "ACGTA" * 13 + "\n", TAIL, "E_LIMIT"),
    "refuse_last_prefix_behind_stale_count": (STD, AB, rec("r1", G60, G60, pre(A), G60), "E_REFHANG", True),
    "refuse_last_second_prefix": (STD, AB, rec("r0", "CCCC") + rec("r1", pre(A), G60, G60, pre(B), G60), "E_REFHANG", True),
}


def run_perl(script, argv, cwd, timeout=60):
    """(stdout, status), or None when the script is still running after `timeout` seconds"""
    try:
        p = subprocess.run(["perl", script] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=timeout)
    except subprocess.TimeoutExpired:
        return None
    return p.stdout, p.returncode


def write_inputs(d, bars, fasta):
    if bars is not None:
        with open(os.path.join(d, "barcodes.txt"), "wb") as f:
            f.write(bars.encode("latin-1"))
    if fasta is not None:
        with open(os.path.join(d, "reads.fas"), "wb") as f:
            f.write(fasta.encode("latin-1"))
    os.makedirs(os.path.join(d, "d"))


def files_in(d):
    made = {os.fsencode(f): open(os.path.join(d, "d", f), "rb").read() for f in os.listdir(os.path.join(d, "d"))}
    return made or None


def goldens(script):
    import barcode_rule
    if os.path.isdir(GOLD):
        shutil.rmtree(GOLD)
    bad = 0
    for name, case in CASES.items():
        argv, bars, fasta = case[:3]
        refusal = case[3] if len(case) > 3 else ""
        hangs = len(case) > 4 and case[4]
        d = os.path.join(GOLD, name)
        os.makedirs(d)
        write_inputs(d, bars, fasta)
        want = barcode_rule.run(argv, cwd=d)
        with open(os.path.join(d, "argv.txt"), "w") as f:
            f.write("".join(a + "\n" for a in argv))
        if refusal:
            ok = want == (b"", refusal, None) and (not hangs or run_perl(script, argv, d, timeout=5) is None)
            shutil.rmtree(os.path.join(d, "d"))
            with open(os.path.join(d, "status.txt"), "w") as f:
                f.write(refusal + "\n")
            print("%-40s refused %-8s%s   rule %s" % (name, refusal, " (the Perl never ends)" if hangs else "", "agrees" if ok else "DIFFERS"))
        else:
            out, status = run_perl(script, argv, d)
            with open(os.path.join(d, "stdout.bin"), "wb") as f:
                f.write(out)
            with open(os.path.join(d, "status.txt"), "w") as f:
                f.write("%d\n" % status)
            got = (out, status, files_in(d))
            if not got[2]:
                os.rmdir(os.path.join(d, "d"))
            ok = got == want
            print("%-40s status %d, %4d bytes of stdout, %2d files   rule %s" % (
                name, status, len(out), len(got[2] or ()), "agrees" if ok else "DIFFERS"))
        bad += not ok
    return bad


def random_case(rng):
    """(barcode file text, sequence file text) as the issue lists: barcodes of 3-12 letters, some in lower case in the file;
    1-8 records of 0-300 letters at widths 50 / 60 / 70; a barcode planted at the start, inside and at the end of line 1,
    at the start and inside of lines 2 and 3, across a line break, or nowhere; blank lines, CRLF, no final line end; the
    planted read is the last record half of the time."""
    nb = rng.randrange(1, 7)
    bars, seen = [], set()
    while len(bars) < nb:
        s = "".join(rng.choice("ACGT") for _ in range(rng.randrange(3, 13)))
        if s not in seen:
            seen.add(s)
            bars.append(s)
    btext = "".join("s%d\t%s%s\n" % (i, s.lower() if rng.random() < 0.25 else s, rng.choice(["", "", " ", "\r"])) for i, s in enumerate(bars))
    if rng.random() < 0.15:
        btext = btext[:-1]
    width = rng.choice([50, 60, 70])
    nrec = rng.randrange(1, 9)
    planted = nrec - 1 if rng.random() < 0.5 else rng.randrange(nrec)
    alphabet = "ACGT" if rng.random() < 0.5 else "GGGGGGC"  # random ACGT meets the short barcodes by itself; G/C rarely
    recs = []
    for r in range(nrec):
        n = rng.randrange(0, 301)
        s = [rng.choice(alphabet) for _ in range(n)]
        if rng.random() < 0.1:
            s = [c.lower() for c in s]
        if r == planted or rng.random() < 0.3:
            bc = rng.choice(bars)
            L = len(bc)
            where = rng.choice(["l1_start", "l1_inside", "l1_end", "l2_start", "l2_inside", "l3_start", "l3_inside", "break", "none"])
            off = {"l1_start": 0, "l1_inside": rng.randrange(1, width - L), "l1_end": width - L, "l2_start": width,
                   "l2_inside": width + rng.randrange(1, width - L), "l3_start": 2 * width, "l3_inside": 2 * width + rng.randrange(1, width - L),
                   "break": rng.choice([1, 2]) * width - rng.randrange(1, L), "none": None}[where]
            if off is not None and off + L <= n:
                s[off:off + L] = list(bc)
        s = "".join(s)
        lines = [s[i:i + width] for i in range(0, len(s), width)]
        body = []
        for ln in lines:
            body.append(ln)
            if rng.random() < 0.05:
                body.append("")
        head = ">r%d%s" % (r, rng.choice(["", "", " length=%d" % n, " x>y"]))
        recs.append("".join(x + "\n" for x in [head] + body))
        if rng.random() < 0.1:
            recs.append("\n")
    text = "".join(recs)
    if rng.random() < 0.1:
        text = text.replace("\n", "\r\n")
    if rng.random() < 0.15:
        text = text[:-1]
    return btext, text


def one_sweep_case(args):
    import barcode_rule
    script, work, i, btext, text = args
    d = os.path.join(work, "c%d" % i)
    os.makedirs(d)
    write_inputs(d, btext, text)
    want = barcode_rule.run(STD, cwd=d)
    if want[1] == "E_REFHANG":  # the never-ending last record
        ok = run_perl(script, STD, d, timeout=2) is None
        got = "still running after 2 s" if ok else "ended"
    else:
        r = run_perl(script, STD, d)
        got = (r[0], r[1], files_in(d)) if r else "still running after 60 s"
        ok = got == want
    shutil.rmtree(d)
    return None if ok else "case %d differs:\n barcodes %r\n reads %r\n perl %r\n rule %r" % (i, btext, text, got, want), want[1] == "E_REFHANG"


def sweep(script, n, seed, jobs):
    rng = random.Random(seed)
    bad = hangs = 0
    with tempfile.TemporaryDirectory(prefix="pgx_barcode_") as work:
        todo = [(script, work, i) + random_case(rng) for i in range(n)]
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            for msg, hang in pool.map(one_sweep_case, todo):
                hangs += hang
                if msg:
                    bad += 1
                    if bad <= 10:
                        print(msg)
    print("sweep: %d inputs (seed %d), %d on which the Perl never ends, %d differ" % (n, seed, hangs, bad))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="the reference tree")
    ap.add_argument("--sweep", type=int, default=0)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    script = os.path.join(a.root, "Barcode", "barcode.pl")
    if not (os.path.exists(script) and shutil.which("perl")):
        sys.exit("gen_goldens_barcode: perl or %s is missing" % script)
    if a.sweep:
        sys.exit(1 if sweep(script, a.sweep, a.seed, a.jobs) else 0)
    sys.exit(1 if goldens(script) else 0)


if __name__ == "__main__":
    main()
