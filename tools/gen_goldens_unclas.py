"""Golden vectors for Unclas_Sel/unclassified_selector.pl, printed by the reference's own Perl script, and a sweep of
tests/unclas_rule.py against it.

Runs on a machine that holds the reference tree and perl; no test imports it.  Each case is a directory
tests/golden/unclas/<case>/ with
  argv.txt    the script's @ARGV, one word per line (an empty line is an empty word)
  m.tsv s.fas the two inputs, where the case has them (file names in argv.txt are relative to the case directory)
  stdout.bin  what the script printed on stdout      status.txt  its exit status
  out.fas     the -o file, where the script made one
usage: python3 tools/gen_goldens_unclas.py --root REFERENCE [--sweep N [--seed S]]
  --sweep N: N random damaged tables / FASTAs with random option mixes through the Perl and through the rule; both must
  agree byte for byte (stdout, status, output file).  Writes no golden.
"""
import argparse
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "..", "tests", "golden", "unclas")
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

STD = ["-m", "m.tsv", "-s", "s.fas", "-o", "out.fas"]


def row(name, pid="99.00", ev="1e-50", bits="250", sep="\t"):
    return sep.join([name, "gi|1|x", pid, "150", "1", "0", "1", "150", "1", "150", ev, bits]) + "\n"


FAS = ">r1\nACGT\nAC\n>r2\nGGGG\n>r3\nTTTT\n>r4\nCCCC\n"
T4 = row("r1") + row("r2", pid="94.99") + row("r3", ev="1e-5") + row("r4", bits="199")

# case -> (argv, table text or None, FASTA text or None)
CASES = {
    "defaults": (STD, T4 + row("r5"), FAS + ">r5\nAAAA\n>r6\nGATC\n"),
    "t_equal": (STD + ["-t", "97.5"], row("r1", pid="97.50") + row("r2", pid="97.49"), FAS),
    "e_equal": (STD + ["-e", "0"], row("r1", ev="1") + row("r2", ev="1.0000001") + row("r3", ev="1e+00"), FAS),
    "b_equal": (STD + ["-b", "200"], row("r1", bits="200") + row("r2", bits="199.9") + row("r3", bits="2e2"), FAS),
    "num_blank_bits": (STD, row("r1", bits=" 200") + row("r2", bits=" 199"), FAS),
    "num_exponent_bits": (STD + ["-b", "12000"], row("r1", bits="1.2e+04") + row("r2", bits="1.1e+04"), FAS),
    "num_text_is_zero": (STD + ["-b", "0"], row("r1", bits="abc") + row("r2", ev="text") + row("r3", pid="high"), FAS),
    "num_trailing_text": (STD, row("r1", pid="96.5%", bits="250bits") + row("r2", pid="%96.5"), FAS),
    "rows_apart_pass_last": (STD, row("r1", pid="50") + row("r2") + row("r3", pid="50") + row("r1"), FAS),
    "rows_apart_pass_first": (STD, row("r1") + row("r2", pid="50") + row("r1", pid="50"), FAS),
    "blank_line_mid": (STD, row("r1") + "\n" + row("r2"), FAS),
    "tabs_0": (STD + ["-t", "0", "-b", "0", "-e", "0"], "r1x\nr22\n", FAS),
    "tabs_1": (STD + ["-t", "0", "-b", "0", "-e", "0"], "r1\t99\n3\tr2\n", FAS),
    "tabs_2": (STD + ["-t", "0", "-b", "50", "-e", "0"], "r1\tx\t99\nr2\t0.5\t40\nr3\t7\t60\n", FAS),
    "tabs_11": (STD, row("r1") + row("r2"), FAS),
    "empty_e_field": (STD, row("r1", ev="") + row("r2", ev="", bits="20"), FAS),
    "short_lines": (STD + ["-t", "0", "-b", "0"], "\t\n\t\t\nr\n\tr2\t\n", FAS + ">\nAC\n"),
    "header_description": (STD, row("r1") + row("r2 second read"), ">r1 first read\nACGT\n>r2 second read\nGGGG\n>r3\nTT\n"),
    "header_trailing_blanks": (STD, row("r1") + row("r2"), ">r1 \t \nACGT\n>r2\x0b\x0c\nGGGG\n> r3\nTT\n"),
    "dup_classified": (STD, row("r1"), ">r1\nAAAA\n>r2\nCC\n>r1\nGGGG\n>r1\nTTTT\n"),
    "dup_rejected": (STD, row("r2", pid="50"), ">r2\nAAAA\n>r1\nCC\n>r2\nGGGG\n"),
    "gt_inside_sequence": (STD, row("C>CC"), ">r1\nAC\nCC>CC\nGG\n>r2\nTT\nCC>CC\nAA\n"),
    "text_before_header": (STD, row("r2"), "stray\nACGT\n\n>r1\nAC\n>r2\nGG\n"),
    "crlf": (STD, (row("r1") + row("r2", bits="150") + row("r3")).replace("\n", "\r\n"),
             (FAS + ">r5\r\nAC\n").replace("\n", "\r\n")),
    "crlf_blank_line": (STD, row("r1") + "\r\n" + row("r2"), FAS),
    "no_final_newline": (STD, row("r1") + row("r2")[:-1], FAS + ">r5\nACGT"),
    "empty_table": (STD, "", FAS),
    "empty_fasta": (STD, T4, ""),
    "flag_as_value": (STD + ["-t", "-b", "150"], row("r1", pid="1", bits="160") + row("r2", bits="140"), FAS),
    "flag_last": (STD + ["-t"], row("r1", pid="0.5") + row("r2", pid="-1"), FAS),
    "flag_last_required": (["-s", "s.fas", "-o", "out.fas", "-x", "y", "-m"], T4, FAS),
    "value_at_twelve": (["-t", "96", "-b", "10", "-e", "-1", "-m", "m.tsv", "-s", "s.fas", "-o", "out.fas"], T4, FAS),
    "args_5": (["-m", "m.tsv", "-s", "s.fas", "-o"], T4, FAS),
    "args_13": (STD + ["-t", "95", "-e", "-20", "-b", "200", "x"], T4, FAS),
    "no_output_option": (["-m", "m.tsv", "-s", "s.fas", "-t", "95"], T4, FAS),
    "unopenable_m": (["-m", "absent.tsv", "-s", "s.fas", "-o", "out.fas"], None, FAS),
    "unopenable_s": (["-m", "m.tsv", "-s", "absent.fas", "-o", "out.fas"], T4, None),
    "unopenable_o": (["-m", "m.tsv", "-s", "s.fas", "-o", "nodir/out.fas"], T4, FAS),
    "e_abc": (STD + ["-e", "abc"], row("r1", ev="1") + row("r2", ev="1.5"), FAS),
    "e_large": (STD + ["-e", "700", "-t", "0", "-b", "0"], row("r1", ev="1e300") + row("r2", ev="1e308") + row("r3", ev="inf"), FAS),
    "t_empty": (STD + ["-t", ""], row("r1", pid="0") + row("r2", pid="-0.01"), FAS),
    "b_huge": (STD + ["-b", "1e9"], T4, FAS),
}


def run_perl(script, argv, cwd):
    p = subprocess.run(["perl", "-w", script] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=60)
    return p.stdout, p.returncode


def write_inputs(d, table, fasta):
    if table is not None:
        with open(os.path.join(d, "m.tsv"), "wb") as f:
            f.write(table.encode("latin-1"))
    if fasta is not None:
        with open(os.path.join(d, "s.fas"), "wb") as f:
            f.write(fasta.encode("latin-1"))


def goldens(script):
    import unclas_rule
    if os.path.isdir(GOLD):
        shutil.rmtree(GOLD)
    for name, (argv, table, fasta) in CASES.items():
        d = os.path.join(GOLD, name)
        os.makedirs(d)
        write_inputs(d, table, fasta)
        want = unclas_rule.run(argv, cwd=d)
        out, status = run_perl(script, argv, d)
        with open(os.path.join(d, "argv.txt"), "w") as f:
            f.write("".join(a + "\n" for a in argv))
        with open(os.path.join(d, "stdout.bin"), "wb") as f:
            f.write(out)
        with open(os.path.join(d, "status.txt"), "w") as f:
            f.write("%d\n" % status)
        made = os.path.join(d, "out.fas")
        got = (out, status, open(made, "rb").read() if os.path.exists(made) else None)
        print("%-24s status %d, %4d bytes of stdout, %s   rule %s" % (
            name, status, len(out), "%4d bytes written" % len(got[2]) if got[2] is not None else "no output file",
            "agrees" if got == want else "DIFFERS"))


NAMES = ["r1", "r2", "r3", "r 4", "r5 d", "R1", "", "x>y"]
NUMS = ["0", "1", "94.99", "95", "95.00", "96.5", "100", "200", "199", "250", " 200", "2e2", "1e-50", "1e-5", "2.1e-09", "2e-09", "",
        "abc", "-3", "+7", "1e", ".5", "5.", "1e400", "-1e400", "0x10", "1_000", "12 3", "nan", "1.2e+04"]


def random_case(rng):
    lines = []
    for _ in range(rng.randrange(0, 12)):
        cols = [rng.choice(NAMES), "s"] + [rng.choice(NUMS) for _ in range(10)]
        k = rng.random()
        if k < 0.15:
            cols = cols[:rng.randrange(0, 12)]
        elif k < 0.2:
            cols += ["extra"]
        line = "\t".join(cols)
        if rng.random() < 0.08:
            line = line.replace("\t", " ", 1)
        lines.append(line + ("\r\n" if rng.random() < 0.1 else "\n"))
    if rng.random() < 0.15 and lines:
        lines.insert(rng.randrange(len(lines)), "\n")
    table = "".join(lines)
    if rng.random() < 0.2:
        table = table[:-1]
    recs = []
    if rng.random() < 0.2:
        recs.append("before\n")
    for _ in range(rng.randrange(0, 9)):
        nm = rng.choice(NAMES)
        recs.append(">" + nm + rng.choice(["", "", " ", "\t", " desc", "\r"]) + "\n")
        for _ in range(rng.randrange(0, 3)):
            recs.append(rng.choice(["ACGT", "NNNN", "", "AC>GT", "acgt\r"]) + "\n")
    fasta = "".join(recs)
    if rng.random() < 0.2:
        fasta = fasta[:-1]
    argv = []
    parts = [["-m", "m.tsv"], ["-s", "s.fas"], ["-o", "out.fas"]]
    for flag in ("-t", "-e", "-b"):
        if rng.random() < 0.5:
            parts.append([flag, rng.choice(NUMS + ["-20", "-5", "0", "700", "710", "-b", "-t"])])
    rng.shuffle(parts)
    for p in parts:
        argv += p
    k = rng.random()
    if k < 0.05:
        argv = argv[:-1]
    elif k < 0.1:
        argv += [rng.choice(["-t", "-b", "-e", "-m", "zz"])]
    elif k < 0.13:
        argv[argv.index("m.tsv")] = "absent"
    elif k < 0.16:
        argv[argv.index("s.fas")] = "absent"
    elif k < 0.19:
        argv[argv.index("out.fas")] = "nodir/out.fas"
    return argv, table, fasta


def sweep(script, n, seed):
    import unclas_rule
    rng = random.Random(seed)
    bad = 0
    with tempfile.TemporaryDirectory(prefix="pgx_unclas_") as work:
        for i in range(n):
            d = os.path.join(work, "c%d" % i)
            os.makedirs(d)
            argv, table, fasta = random_case(rng)
            write_inputs(d, table, fasta)
            want = unclas_rule.run(argv, cwd=d)
            out, status = run_perl(script, argv, d)
            made = os.path.join(d, "out.fas")
            got = (out, status, open(made, "rb").read() if os.path.exists(made) else None)
            if got != want:
                bad += 1
                print("case %d differs: argv %r\n table %r\n fasta %r\n perl %r\n rule %r" % (i, argv, table, fasta, got, want))
    print("sweep: %d inputs, %d differ" % (n, bad))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="the reference tree")
    ap.add_argument("--sweep", type=int, default=0)
    ap.add_argument("--seed", type=int, default=20261017)
    a = ap.parse_args()
    script = os.path.join(a.root, "Unclas_Sel", "unclassified_selector.pl")
    if not (os.path.exists(script) and shutil.which("perl")):
        sys.exit("gen_goldens_unclas: perl or %s is missing" % script)
    if a.sweep:
        sys.exit(1 if sweep(script, a.sweep, a.seed) else 0)
    goldens(script)


if __name__ == "__main__":
    main()
