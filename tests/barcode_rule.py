"""`perl Barcode/barcode.pl -s READS.fas -b BARCODES.txt -d DIR`, restated in plain Python over bytes: what the script
computes (its accidents included), line numbers of barcode.pl cited.

`run(argv, cwd)` returns (stdout bytes, status, files) and writes nothing: status is the exit status (0), or "E_ARG" /
"E_LIMIT" / "E_REFHANG" where the project refuses the input, and files maps each name the script leaves in DIR to
its bytes (None when it creates none).  `demux(barcodes, text)` is the part after the files are open; `fates(...)` gives
one tuple per record.  Pinned byte for byte by tests/golden/barcode/ (printed by the reference's own Perl,
tools/gen_goldens_barcode.py) and by that tool's sweep.

Three globals of the script decide bytes of its output and are restated literally:
  * `$first` is never cleared (:195), so every sequence line is tried as a prefix line, and a prefix match sets
    `place = 1` whatever line it was found on;
  * return_bases (:258-268) walks the *shared* loop variable `$b` to the end of the record, which ends the search;
  * return_bases reads the *global* `$storeSize` (:99), not find_and_store_barcode's own.  For every record but the last
    the two are equal.  The last record is processed after the loop (:116) with the global still holding the line count
    of the record before it (0 in a one-record file): its sum of line lengths runs to that stale count (lines that do
    not exist count 0), and the search resumes at line max(place + 1, stale) + 1.  From there on only a prefix match can
    fire (`$thisBar` is set); it overrides the barcode, recomputes `bases` with place = 1, and sets `$b` back to
    max(2, stale) -- at or before the line it matched on, so the script meets the same line again and never ends.  The
    same happens when the last record's first match is a prefix match on a line behind max(2, stale).  Perl printed
    nothing in these cases (it was killed); the project refuses them: "E_REFHANG".
"""
import os

_SPACE = b" \t\n\r\f\v"
MAX_BARCODES = 2048   # refused above: E_LIMIT
MAX_LETTERS = 64

NOBAR, THROWN, KEPT = 0, 1, 2


class Refused(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


def lines_of(text):
    """<FH> in a loop: pieces ending in "\\n", and the rest of the file when it does not end in one"""
    out = text.split(b"\n")
    last = out.pop()
    out = [x + b"\n" for x in out]
    if last:
        out.append(last)
    return out


def parse_barcodes(text):
    """[(name, LETTERS)] in file order, :84-93; Refused for what the project does not guess at"""
    bars, seen = [], set()
    for line in lines_of(text):
        tab = line.find(b"\t")
        if tab < 0:
            raise Refused("E_ARG")
        name = line[:tab]
        letters = line.rstrip(_SPACE)[tab + 1:].upper()  # (empty when the tab itself was trailing white space)
        if not name or not letters or not letters.isalpha():  # bytes.isalpha: A-Z and a-z only
            raise Refused("E_ARG")
        if b"/" in name or b"\0" in name or name in seen:
            raise Refused("E_ARG")
        if len(letters) > MAX_LETTERS:
            raise Refused("E_LIMIT")
        seen.add(name)
        bars.append((name, letters))
    if len(bars) > MAX_BARCODES:
        raise Refused("E_LIMIT")
    return bars


def records_of(text):
    """(records, count): each record a list of lines, header first, :94-116.  Text before the first header: Refused."""
    recs = []
    for line in lines_of(text):
        if b">" in line:
            recs.append([line])
        elif line != b"\n":
            if not recs:
                raise Refused("E_ARG")
            recs[-1].append(line)
    return recs


def _bases(lines, letters, place, upto):
    """return_bases, :258-268: `upto` is the global $storeSize"""
    n = 60 - (lines[place].find(letters) + len(letters))
    for k in range(place + 1, upto):
        if k < len(lines):
            n += len(lines[k])
    return n


def search(lines, bars, stale=None):
    """(barcode index or -1, place, bases) of one record, :164-211.  stale=None: any record but the last."""
    S = len(lines)
    G = S if stale is None else stale
    this, place, bases = -1, 0, 0
    b = 1
    while b < S:
        line = lines[b]
        hit = False
        for a, (_, letters) in enumerate(bars):  # :185-194, $first is always 1
            if line.startswith(letters):
                this, place, hit = a, 1, True
                bases = _bases(lines, letters, 1, G)
                nb = max(2, G)
                if nb + 1 <= b:
                    raise Refused("E_REFHANG")  # the script meets line b again and again
                b = nb
                break
        if this == -1 and not hit:
            for a, (_, letters) in enumerate(bars):  # :199-208
                if letters in line:
                    this, place = a, b
                    bases = _bases(lines, letters, b, G)
                    b = max(b + 1, G)
                    break
        b += 1
    return this, place, bases


def _shift_all(lines):
    """`while($temp = shift(@storedLines))`: ends at a false line, and only "0" (a last line with no line end) is one"""
    for ln in lines:
        if ln == b"0":
            return
        yield ln


def demux(bars, text):
    """The script after its opens: (counts dict, files dict), :94-160"""
    recs = records_of(text)
    out = [[] for _ in bars]
    bar_count = [0] * len(bars)
    nobar, n_nobar, n_thrown, n_norm = [], 0, 0, 0
    fate_list = []
    todo = [(r, None) for r in recs[:-1]]
    if recs:
        todo.append((recs[-1], len(recs[-2]) if len(recs) > 1 else 0))
    else:
        todo.append(([], 0))  # :116 runs on the empty list: $thisBar is still 0, $bases 0 -- "thrown out"
    for lines, stale in todo:
        if not lines:
            this, place, bases = 0, 0, 0
        else:
            this, place, bases = search(lines, bars, stale)
        if this == -1:  # :212-220
            n_nobar += 1
            nobar.extend(_shift_all(lines))
            nobar.append(b"\n")
            fate_list.append((NOBAR, -1, 0, 0))
        elif bases < 100:  # :221-225
            n_thrown += 1
            fate_list.append((THROWN, this, place, bases))
        else:  # :226-255
            name, letters = bars[this]
            bar_count[this] += 1
            n_norm += 1
            o = out[this]
            rest = _shift_all(lines)
            o.append(b">" + name + b"_" + next(rest)[1:])
            skip, trimmed = place - 1, False
            for ln in rest:
                if skip:
                    skip -= 1
                elif not trimmed:
                    o.append(ln[ln.find(letters) + len(letters):])
                    trimmed = True
                else:
                    o.append(ln)
            o.append(b"\n")
            fate_list.append((KEPT, this, place, bases))
    files = {b"nobar.fas": b"".join(nobar)}
    mn = len(out[0]) if bars else 0  # :119, a count of pushed lines
    count_txt = []
    for a, (name, letters) in enumerate(bars):
        count_txt.append(b"%02d\t%s\t%d\n" % (a + 1, letters, bar_count[a]))
        files[b"bar" + name + b".fas"] = b"".join(out[a])
        if 100 < bar_count[a] < mn:
            mn = bar_count[a]
    files[b"barcode_count.txt"] = b"".join(count_txt)
    files[b"info.txt"] = b"%d" % mn
    counts = {"count": len(recs), "norm": n_norm, "nobar": n_nobar, "thrown": n_thrown, "bar_count": bar_count,
              "fates": fate_list}
    return counts, files


def fates(bars, text):
    """one (fate, barcode, place, bases) per record in file order (one "thrown" entry for a file with no record)"""
    return demux(bars, text)[0]["fates"]


def run(argv, cwd="."):
    """The whole script on @ARGV: (stdout, status, files or None)"""
    argv = [os.fsencode(a) for a in argv]
    if len(argv) < 4:  # :18
        return b"Please enter the -s sequences and -b barcodes.\n", 0, None
    if len(argv) > 6:  # :23
        return b"Too many inputs\n", 0, None
    arg = lambda i: argv[i] if i < len(argv) else None  # noqa: E731
    seq = bar = dirn = None
    for a in range(len(argv)):  # :29-43: every position, values included
        if argv[a] == b"-s":
            seq = arg(a + 1)
        elif argv[a] == b"-b":
            bar = arg(a + 1)
        elif argv[a] == b"-d":
            dirn = arg(a + 1)
    if seq is None or bar is None:
        return b"Must enter at least -s sequences and -b barcodes.\n", 0, None
    if dirn is None:
        return b"", "E_ARG", None
    at = lambda p: os.path.join(os.fsencode(cwd), p)  # noqa: E731
    hint = b"\nMake sure you entered the extension when entering the file name."
    log = b"Opening " + seq + b"..."
    try:
        text = open(at(seq), "rb").read()
    except OSError:
        return log + b"Unable to open " + seq + hint, 0, None
    log += b"Successful.\nOpening " + bar + b"..."
    try:
        btext = open(at(bar), "rb").read()
    except OSError:
        return log + b"Unable to open " + bar + hint, 0, None
    log += b"Successful.\nCreating Files...\n"
    try:
        bars = parse_barcodes(btext)
        c, files = demux(bars, text)
    except Refused as r:
        return b"", r.status, None
    log += (b"Found %d sequences.\nFound %s barcodes at the beginning.\nFound no barcodes in %d sequences.\n"
            b"Threw out %d barcodes based on length.\nWriting Files...Successful.\nFinished!\n"
            % (c["count"], b"%d" % c["norm"] if c["norm"] else b"", c["nobar"], c["thrown"]))
    return log, 0, files
