"""`perl Unclas_Sel/unclassified_selector.pl -m TABLE -s READS.fas -o OUT [-t PCT] [-e LN_EVALUE] [-b BITS]`, restated in
plain Python: what the script computes (not what its header comment says), line numbers of unclassified_selector.pl cited.

`run(argv, cwd)` returns (stdout bytes, exit status, output file bytes or None) and writes nothing; `select(table, fasta,
t, e, b)` is the part after the option walk, on bytes.  Pinned byte for byte by tests/golden/unclas/ (printed by the
reference's own Perl, tools/gen_goldens_unclas.py) and by that tool's sweep.

Left out, and kept out of the goldens: Perl's two-argument open() reads more than a file name out of a path that begins or
ends with blanks or with one of `<>|+&-`.
"""
import math
import os
import re

_SPACE = b" \t\n\r\f\v"
_NUM = re.compile(rb"[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?)")


def perl_num(s):
    """What `<`, `>` and exp() make of a string (perlnumber): blanks, sign, Inf / NaN, decimal digits with optional
    fraction and exponent; any other text counts as 0, text behind the number is ignored.  None is undef: 0."""
    if s is None:
        return 0.0
    if isinstance(s, str):
        s = s.encode("latin-1")
    s = s.lstrip(_SPACE)
    body = s[1:] if s[:1] in (b"+", b"-") else s
    low = body[:3].lower()
    if low == b"inf":
        return -math.inf if s[:1] == b"-" else math.inf
    if low == b"nan":
        return math.nan
    m = _NUM.match(s)
    return float(m.group(0)) if m else 0.0


def perl_exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def p_index(s, sub, pos=0):
    return s.find(sub, min(max(pos, 0), len(s)))


def p_rindex(s, sub, pos=None):
    if pos is None:
        return s.rfind(sub)
    pos = min(max(pos, 0), len(s))
    return s.rfind(sub, 0, pos + len(sub))


def p_substr(s, off, length=None):
    """substr with off >= 0 (all the script ever passes); a negative length leaves that many characters off the end; an
    offset behind the end gives undef, which the script then uses as "" (hash key) or 0 (number)."""
    if off > len(s):
        return b""
    if length is None:
        return s[off:]
    end = off + length if length >= 0 else len(s) + length
    return s[off:max(end, off)]


def cut_columns(line):
    """(name, percent, E, B) of a chomped table line: unclassified_selector.pl:85-95"""
    start = p_index(line, b"\t") + 1
    start = p_index(line, b"\t", start) + 1
    end = p_index(line, b"\t", start)
    percent = p_substr(line, start, end - start)
    bstart = p_rindex(line, b"\t") + 1
    b = p_substr(line, bstart)
    estart = p_rindex(line, b"\t", bstart - 3) + 1
    eend = bstart - 1
    e = p_substr(line, estart, eend - estart)
    name = p_substr(line, 0, p_index(line, b"\t"))
    return name, percent, e, b


def lines_of(text):
    """<FH> in a loop: pieces ending in "\\n", and the rest of the file when it does not end in one"""
    out = text.split(b"\n")
    last = out.pop()
    out = [x + b"\n" for x in out]
    if last:
        out.append(last)
    return out


def classified_names(table, t, e, b):
    """:78-111: the names with at least one row that passes (the script's second hash only ever holds the others)"""
    names = set()
    for line in lines_of(table):
        if line == b"\n":  # :80
            break
        if line.endswith(b"\n"):
            line = line[:-1]
        name, percent, ev, bits = cut_columns(line)
        if not (perl_num(percent) < t or perl_num(ev) > e or perl_num(bits) < b):  # :96
            names.add(name)
    return names


def select(table, fasta, t, e, b):
    """(output file bytes, headers printed): :78-166 for numeric thresholds (e is the e-value itself, not its logarithm)"""
    left = classified_names(table, t, e, b)
    out, count, found = [], 0, False
    for line in lines_of(fasta):
        if b">" in line:  # :128
            name = line[1:].rstrip(_SPACE)
            if name in left:  # :143-153: the first header of a classified name is dropped, and the name forgotten
                left.discard(name)
                found = False
            else:
                out.append(b">" + name + b" \n")
                count += 1
                found = True
        elif found:
            out.append(line)
    return b"".join(out), count


def keep_mask(table, fasta, t, e, b):
    """per FASTA record (header line), in file order: 1 when the script prints it"""
    left = classified_names(table, t, e, b)
    mask = []
    for line in lines_of(fasta):
        if b">" in line:
            name = line[1:].rstrip(_SPACE)
            mask.append(0 if name in left else 1)
            left.discard(name)
    return mask


def thresholds(t=None, e=None, b=None):
    """the three numbers the option texts stand for (None: the script's default), :28-30, :44-53"""
    return (95.0 if t is None else perl_num(t), math.exp(-20) if e is None else perl_exp(perl_num(e)),
            200.0 if b is None else perl_num(b))


def run(argv, cwd="."):
    """The whole script on @ARGV (a list of bytes): (stdout, exit status, output file bytes or None).  The caller writes
    the output file; the status is 0, or errno when `-o` cannot be created (`die $!`, :123)."""
    argv = [os.fsencode(a) for a in argv]
    if len(argv) < 6 or len(argv) > 12:  # :21
        return (b"Please enter the -m megablast, -s sequences, -t threshold, -e e-value upper threshold, -b bitscore lower "
                b"threshold, and -o output file.\n"), 0, None
    arg = lambda i: argv[i] if i < len(argv) else None  # noqa: E731
    t, e, b = 95.0, math.exp(-20), 200.0
    mega = sequ = outp = None
    for a in range(12):  # :32-59: every position, values included
        w = arg(a)
        if w == b"-m":
            mega = arg(a + 1)
        elif w == b"-s":
            sequ = arg(a + 1)
        elif w == b"-t":
            t = perl_num(arg(a + 1))
        elif w == b"-e":
            e = perl_exp(perl_num(arg(a + 1)))
        elif w == b"-b":
            b = perl_num(arg(a + 1))
        elif w == b"-o":
            outp = arg(a + 1)
    if mega is None or sequ is None or outp is None:
        return b"Must have at least -m megablast -s sequences -o output file.\n", 0, None
    at = lambda p: os.path.join(os.fsencode(cwd), p)  # noqa: E731
    hint = b"\nMake sure you entered the extension when entering the file name."
    log = b"Opening " + mega + b"..."
    try:
        table = open(at(mega), "rb").read()
    except OSError:
        return log + b"Unable to open " + mega + hint, 0, None
    log += b"successful.\nRejecting...successful.\nOpening " + sequ + b"..."
    try:
        fasta = open(at(sequ), "rb").read()
    except OSError:
        return log + b"Unable to open " + sequ + hint, 0, None
    log += b"successful.\nCreating " + outp + b"..."
    try:  # (probed without leaving a file behind)
        existed = os.path.exists(at(outp))
        open(at(outp), "ab").close()
        if not existed:
            os.remove(at(outp))
    except OSError as err:
        return log, err.errno, None
    text, count = select(table, fasta, t, e, b)
    log += b"successful.\nPrinting...successful.\nRejected %d sequence(s).\nFinished!\n" % count
    return log, 0, text
