"""Consensus_BLAST_SOAP_RDP-1.1.pl:86-234 restated in plain Python, line by line, on bytes.

`consensus(blast, rdp)` returns the output text, the log and one Record per printed read (the winning row and its
match count).  Each record also carries what the device will do with that read (`Record.group`, `.form`, `.grid`), so
a test can count which forms a set of inputs reaches.  The `Variant` switches give likely wrong restatements; a test
that cannot tell them from the script proves nothing about a kernel that makes the same mistake.
"""
import re
from dataclasses import dataclass, field

RDP_RANKS = [b"domain", b"phylum", b"class", b"order", b"family", b"genus", b"species"]   # Consensus:64-72
BLAST_RANKS = [b"0", b"1", b"2", b"3", b"4", b"5", b"6"]                                  # Consensus:74-82


@dataclass(frozen=True)
class Variant:
    rm_numeric: bool = False        # `$rankmatches gt/eq $maxrankmatches` as numbers
    count_numeric: bool = False     # `$blastcount gt $maxblastcount` as numbers
    sim_numeric: bool = False       # `$blastsim lt $blastline[2]` as numbers
    last_tie: bool = False          # `le` for `lt`: the last of tied hits wins, not the first
    keep_maxcount: bool = False     # a later replacement leaves $maxblastcount at the first pick's count
    no_undef_rank: bool = False     # undef index on both sides does not count as equal


PERL = Variant()


@dataclass
class Record:
    read: bytes
    row: int            # index of the winning row among the read's rows (table order)
    matches: int
    rows: list = field(default_factory=list)   # per row: (token count, agreement count, pident text)
    ntrip: int = 0      # RDP triplets of the read's line
    group: str = ""     # device labels, filled by label()
    form: str = ""
    grid: str = ""


class ReferenceHang(RuntimeError):
    """The script never terminates on this input (the cursor runs past the BLAST table forever)."""


def perl_split(pattern, s):
    """split(/pattern/, s): trailing empty fields removed, an undef or empty string gives no fields."""
    if not s:
        return []
    f = re.split(pattern, s)
    while f and f[-1] == b"":
        f.pop()
    return f


def lineage_tokens(tax):
    """Consensus:116-122: split on `[`, `]`, `;`, join with ' ', split ' '."""
    return b" ".join(perl_split(rb"\[|\]|;", tax or b"")).split()


def clean_rdp_name(name):
    r"""Consensus:159-160: s/"|\\//g then s/[\W\d_]//g -- ASCII letters stay."""
    name = re.sub(rb'"|\\', b"", name)
    return re.sub(rb"[^A-Za-z]", b"", name)


def _idx(table, tok):
    try:
        return table.index(tok)
    except ValueError:
        return None         # undef


def _text(v):
    return b"" if v is None else (str(v).encode() if isinstance(v, int) else v)


def _num(t):
    m = re.match(rb"\s*[-+]?(\d+\.?\d*|\.\d+)", t or b"")
    return float(m.group(0)) if m else 0.0


def rdp_triplets(rdptax):
    """(cleaned name, rank index or None) of every triplet: what Consensus:159-170 compares (the cleaning is idempotent,
    so doing it once per line gives what the script's repeated in-place cleaning gives)."""
    return [(clean_rdp_name(rdptax[b]), _idx(RDP_RANKS, rdptax[b + 1]) if b + 1 < len(rdptax) else None)
            for b in range(0, len(rdptax), 3)]


def rank_matches(tokens, trips, v=PERL):
    """Consensus:154-184: every (rank, name) pair of the lineage against every RDP triplet."""
    rm = 0
    for a in range(0, len(tokens), 2):
        name = tokens[a + 1] if a + 1 < len(tokens) else b""
        i1 = _idx(BLAST_RANKS, tokens[a])
        for clean, i2 in trips:
            if v.no_undef_rank and (i1 is None or i2 is None):
                continue
            if name == clean and i1 == i2:
                rm += 1
    return rm


def consensus(blast, rdp, out_name=b"@OUT@", v=PERL):
    """The script on two texts: (output, log, [Record]).  Raises ReferenceHang where the Perl loops forever."""
    lines = blast.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    rdp_lines = rdp.split(b"\n")
    if rdp_lines and rdp_lines[-1] == b"":
        rdp_lines.pop()
    out, log, recs = [], [b"\nLoading input files...\n", out_name + b"\n"], []
    i = 0
    found = None
    maxblastcount = maxrankmatches = 0
    tempresult = blastsim = None
    pick = None             # index among the read's rows of $tempresult
    rows = []
    for rdpline in rdp_lines:
        rdpf = perl_split(rb"\t\t\t\t\t", rdpline)
        rid = rdpf[0] if rdpf else b""
        rdptax = perl_split(rb"\t", rdpf[1] if len(rdpf) > 1 else b"")
        trips = rdp_triplets(rdptax)
        while True:     # GETBLAST
            bline = lines[i] if i < len(lines) else None
            bf = perl_split(rb"\t\t|\t", bline)
            bid = bf[0] if bf else b""
            if bid == rid:
                if bline is None:
                    raise ReferenceHang("an empty RDP read name after the BLAST table ends")
                found = 1
                tokens = lineage_tokens(bf[1] if len(bf) > 1 else b"")
                sim = bf[2] if len(bf) > 2 else b""
                rm = rank_matches(tokens, trips, v)
                blastcount = len(tokens)
                had_pick = pick is not None
                if (rm > maxrankmatches) if v.rm_numeric else (_text(rm) > _text(maxrankmatches)):      # Consensus:191
                    maxrankmatches = rm
                    tempresult = bline
                    blastsim = sim
                    pick = len(rows)
                more = blastcount > maxblastcount if v.count_numeric else _text(blastcount) > _text(maxblastcount)
                if v.sim_numeric:
                    better = _num(blastsim) < _num(sim)
                else:
                    better = _text(blastsim) <= sim if v.last_tie else _text(blastsim) < sim
                if (more or better) and rm == maxrankmatches:                                              # Consensus:199
                    if not (v.keep_maxcount and had_pick):
                        maxblastcount = blastcount
                    tempresult = bline
                    blastsim = sim
                    pick = len(rows)
                rows.append((blastcount, rm, sim))
                i += 1
                continue
            if found == 0:      # Consensus:216-220
                log.append(b"not found: " + bid + b"\t " + rid + b"\n")
                if bline is None:
                    raise ReferenceHang("RDP read %r has no BLAST rows at or after the cursor" % rid)
                i += 1
                continue
            if found == 1:      # Consensus:223-234
                out.append(_text(tempresult) + b"\n#Matches found: " + _text(maxrankmatches) + b"\n")
                recs.append(Record(rid, pick if pick is not None else -1, maxrankmatches, rows, (len(rdptax) + 2) // 3))
                found = 0
                maxblastcount = maxrankmatches = 0
                blastsim = b"0"
            pick = None
            rows = []
            break
    log.append(b"\nDone!\n")
    return b"".join(out), b"".join(log), recs


def hit_group(n_rows):
    """k_sort_consensus<32> (two reads per wavefront), k_sort_consensus<64>, or sort_big_reads + k_consensus_serial."""
    return "le32" if n_rows <= 32 else ("le64" if n_rows <= 64 else "big")


def selection_form(rows):
    """Which form of Consensus:186-204 k_sort_consensus takes (classify.hip): every row with the same token count c >= 1
    -> the closed form; otherwise no agreement anywhere -> the chain's all-zero start; the top row holding the text-order
    largest agreement -> the successor chain; else the literal walk on 32-bit text keys.  Counts of 10^8 and more (the
    64-bit walk) are out of reach: lineages hold far fewer tokens than that and pident has about 10 000 texts."""
    counts = {c for c, _, _ in rows}
    assert all(c < 10 ** 8 and rm < 10 ** 8 for c, rm, _ in rows)
    if len(counts) == 1 and 0 not in counts:
        return "closed"
    if all(rm == 0 for _, rm, _ in rows):
        return "zero"
    if _text(rows[0][1]) == max(_text(rm) for _, rm, _ in rows):
        return "chain"
    return "walk"


def record_pairs(ntok):
    """Pairs of a subject's pair record (annotate.hip): None where the record escapes to the general count."""
    np_ = (ntok + 1) // 2
    return None if np_ > 15 or ntok > 0xFFFF else np_


def max_pairs(token_counts):
    """The database's widest pair record (escaped records skipped): <= 7 -> 32-byte records, else 64-byte ones."""
    return max([p for p in map(record_pairs, token_counts) if p is not None] + [0])


def label(recs, db_max_pairs, nr_max):
    """Fill the device labels of every record.  `nr_max` = the batch's largest triplet count, capped at 8 (the RDP
    import's max_trip).  The grid is what pair_matches runs for a read in the wavefront kernels; the big reads always
    take the general count."""
    for r in recs:
        r.group = hit_group(len(r.rows))
        r.form = selection_form(r.rows) if r.rows else "none"
        if r.group == "big" or r.ntrip > 8:
            r.grid = "general"
        elif any(record_pairs(c) is None for c, _, _ in r.rows):
            r.grid = "escape"
        elif db_max_pairs <= 7 and nr_max <= 6:
            r.grid = "7x6"
        else:
            r.grid = "15x8"
    return recs
