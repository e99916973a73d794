"""`soap -a reads -D ref.index -o out [-u unmapped] -M m -r r -n n [-t] [-l L -v V]`, single-end, restated in plain Python.

The reference ships soap only as a closed ELF (Classify/Runsoap/soap2.21release); every rule below was observed from that
binary and is pinned by tests/golden/soap/ (no -l / -v) and tests/golden/soap_seed/ (DESIGN section 10 states them in
prose).  `soap_single()` returns the rows text and the unmapped text; row order inside a read is this project's documented
(subject, position, strand) order, the ELF's is its suffix array's, so tests compare rows as sets per read.

Without -l / -v (or when the seed would not be shorter than the read) a read is placed whole: every ungapped placement
with at most 2 mismatches counts, and -M picks among them by mismatch count.  With a seed of `l` bases (the read's first
`l` bases; on the '-' strand the last `l` of the reverse complement) a read that has no whole-read placement is placed by
its seed: the seed has at most 2 mismatches, the bases outside it at most `v`, -M picks by the seed's mismatches, and the
row's mismatch column and entries describe the seed only.
"""

from dataclasses import dataclass

import numpy as np

MIN_READ = 27       # shorter reads are never placed
MIN_SEED = 27       # -l below this: as if no -l had been given
MAX_V = 20          # -v above this counts as 20 (the ELF's -v 50 prints the rows of -v 20)
_CODE = np.full(256, 2, dtype=np.int8)          # every letter other than ACGT reads as G
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i
_ACGT = b"ACGT"


def _fasta(path):
    name, buf = None, []
    for line in open(path, "rb"):
        line = line.rstrip(b"\r\n")
        if line.startswith(b">"):
            if name is not None:
                yield name, b"".join(buf)
            name, buf = line[1:], []
        elif name is not None:
            buf.append(line.strip())
    if name is not None:
        yield name, b"".join(buf)


@dataclass
class Ref:
    ids: list           # subject ids (first word of the header)
    off: np.ndarray     # global start of each subject, n + 1 entries
    base: np.ndarray    # all subjects back to back, 0..3, ambiguity codes as G
    seg_of: np.ndarray  # per global position: index of its segment, -1 inside a cut run
    seg_hi: np.ndarray  # end of each segment
    index: dict         # k -> {k-mer bytes: [global positions]}


def load_ref(path):
    ids, parts, amb = [], [], []
    for name, seq in _fasta(path):
        ids.append(name.split()[0].decode() if name.split() else "")
        a = np.frombuffer(seq, dtype=np.uint8)
        parts.append(_CODE[a].astype(np.uint8))
        up = a & 0xDF
        amb.append(~np.isin(up, np.frombuffer(b"ACGT", dtype=np.uint8)))
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    base = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    seg_of = np.full(len(base), -1, dtype=np.int64)
    seg_hi = []
    # segments: the stretches between runs of >= 10 ambiguity codes (what 2bwt-builder cuts out)
    for s, am in enumerate(amb):
        start, k, e = 0, 0, len(am)
        while k <= e:
            r = k
            while r < e and am[r]:
                r += 1
            if k == e or r - k >= 10:
                if k > start:
                    seg_of[off[s] + start:off[s] + k] = len(seg_hi)
                    seg_hi.append(int(off[s] + k))
                start = r
            k = r if r > k else k + 1
    return Ref(ids, off, base, seg_of, np.array(seg_hi, dtype=np.int64), {})


def load_reads(path):
    """(name, bases 0..3, number of non-ACGT letters) per record; the name is the header's first word"""
    out = []
    for name, seq in _fasta(path):
        a = np.frombuffer(seq, dtype=np.uint8)
        n_amb = int((~np.isin(a & 0xDF, np.frombuffer(b"ACGT", dtype=np.uint8))).sum())
        words = name.split()
        out.append((words[0].decode() if words else "", _CODE[a].astype(np.uint8), n_amb))
    return out


def _kmers(ref, k):
    idx = ref.index.get(k)
    if idx is None:
        idx = {}
        b = ref.base.tobytes()
        for p in range(len(b) - k + 1):
            idx.setdefault(b[p:p + k], []).append(p)
        ref.index[k] = idx
    return idx


def _candidates(ref, q, a, w):
    """placements (global start of the read) where read bases [a, a + w) have at most 2 mismatches: one of three disjoint
    pieces of the window matches exactly (pigeonhole)"""
    k = w // 3
    idx = _kmers(ref, k)
    out = set()
    for j in range(3):
        o = a + j * k
        for p in idx.get(q[o:o + k].tobytes(), ()):
            out.add(p - o)
    return out


def _fits(ref, gp, L):
    """inside one segment and ending before its last base"""
    if gp < 0 or gp >= len(ref.base):
        return False
    s = ref.seg_of[gp]
    return s >= 0 and gp + L < ref.seg_hi[s]


@dataclass
class Hit:
    subject: int
    pos: int            # 0-based, in the subject
    strand: int         # 0 '+', 1 '-'
    nmis: int           # mismatches printed in column 10 (whole read, or the seed)
    mis: list           # their reference-oriented offsets, ascending
    seeded: bool


def _place(ref, q, strand, a, w, L, rest_cap):
    """placements of the reference-oriented read q whose bases [a, a + w) have <= 2 mismatches and whose other bases have
    at most rest_cap"""
    hits = []
    for gp in _candidates(ref, q, a, w):
        if not _fits(ref, gp, L):
            continue
        diff = np.nonzero(ref.base[gp:gp + L] != q)[0]
        inside = [int(d) for d in diff if a <= d < a + w]
        if len(inside) > 2 or len(diff) - len(inside) > rest_cap:
            continue
        s = int(np.searchsorted(ref.off, gp, side="right") - 1)
        hits.append(Hit(s, int(gp - ref.off[s]), strand, len(inside), inside, w < L))
    return hits


def _pick(hits, mode):
    """-M 4: the fewest mismatches any placement has; -M 0 / 1 / 2: the placements with exactly that many"""
    if not hits:
        return []
    best = min(h.nmis for h in hits) if mode == 4 else mode
    return sorted((h for h in hits if h.nmis == best), key=lambda h: (h.subject, h.pos, h.strand))


def search(ref, q_fwd, mode=4, seed_len=None, max_rest=None):
    """the read's rows (before -r): whole-read placements, else (seed_len < read length) seed placements"""
    L = len(q_fwd)
    q_rc = (3 - q_fwd[::-1]).astype(np.uint8)
    whole = _place(ref, q_fwd, 0, 0, L, L, 0) + _place(ref, q_rc, 1, 0, L, L, 0)
    rows = _pick(whole, mode)
    if rows or seed_len is None or seed_len < MIN_SEED or seed_len >= L:
        return rows
    v = min(max_rest, MAX_V)
    seeded = _place(ref, q_fwd, 0, 0, seed_len, L, v) + _place(ref, q_rc, 1, L - seed_len, seed_len, L, v)
    return _pick(seeded, mode)


def _entries(h, L, l):
    """column 10's entries as (offset printed, reference-oriented offset, quality)"""
    if not h.seeded:
        m = list(h.mis)
        if h.nmis == 2 and m[1] >= L - 13:
            m.reverse()   # entries descend when one lies in the last 13 bases
        return [(x, x, -64 if h.nmis == 1 and h.strand and x == 0 else 40) for x in m]
    a = L - l if h.strand else 0      # where the seed starts, reference-oriented
    rel = [x - a for x in h.mis]
    if h.nmis == 1:
        # one mismatch: counted from the seed's start in the seed's first half, else from the read's
        p = rel[0] if rel[0] < l // 2 else h.mis[0]
        return [(p, h.mis[0], -64 if h.strand and rel[0] == 0 else 40)]
    if h.nmis == 2:
        if rel[1] >= l - 13:          # descending when one lies in the seed's last 13 bases, both from the read's start
            return [(h.mis[1], h.mis[1], 40), (h.mis[0], h.mis[0], 40)]
        return [(rel[0], h.mis[0], 40), (h.mis[1], h.mis[1], 40)]   # the first from the seed's start
    return []


def row(name, q, h, nbest, ref, repeat, l, seeded_run=False):
    """one output row; q = the read in the row's orientation.  A run without -l / -v keeps this project's earlier -r 0
    rendering (a trailing 0 in the last column); a seeded run renders -r 0 as the ELF does"""
    L = len(q)
    g0 = int(ref.off[h.subject]) + h.pos
    rb = ref.base[g0:g0 + L]
    out = [name, bytes(_ACGT[b] for b in q).decode(), "h" * L, str(nbest), "a", str(L), "-" if h.strand else "+",
           ref.ids[h.subject], str(h.pos + 1), str(h.nmis)]
    for p, x, qual in _entries(h, L, l):
        # the ELF fetches the read base through the printed offset, kept in 8 bits
        out.append("%s->%d%s%d" % (chr(_ACGT[rb[x]]), p & 255, chr(_ACGT[q[p & 255]]), qual))
    out.append("%dM" % L)
    md, run, first = [], 0, True
    for k in range(L):
        if q[k] == rb[k]:
            run += 1
            continue
        if first or run > 0:
            md.append(str(run))
        md.append(chr(_ACGT[rb[k]]))
        run, first = 0, False
    if run > 0 or first or (repeat == 2 if seeded_run else repeat != 1):
        md.append(str(run))
    out.append("".join(md))
    return "\t".join(out) + "\n"


def soap_single(ref, reads, M=4, r=1, n=5, t=False, l=None, v=None):
    """(rows text, unmapped text) of a single-end run; l / v = None: the option was not given (the seed then spans the
    whole read, soap.man:59-72: -l defaults to 256 and -v to 5, which this restatement does not apply without them)"""
    seed_len = None
    if l is not None or v is not None:
        seed_len = 256 if l is None else l
        v = 5 if v is None else v
    out, unm = [], []
    for i, (name, q, n_amb) in enumerate(reads):
        rows = [] if len(q) < MIN_READ or n_amb > n else search(ref, q, M, seed_len, v)
        nb = len(rows)
        if nb and not (r == 0 and nb > 1):
            q_rc = (3 - q[::-1]).astype(np.uint8)
            for h in rows[:nb if r == 2 else 1]:
                out.append(row(str(i) if t else name, q_rc if h.strand else q, h, nb, ref, r, seed_len or len(q),
                               seed_len is not None))
        elif nb <= 1 or seed_len is not None:   # seeded runs: -r 0 sends a read with several placements here too
            unm.append(">%s\n%s\n" % (name, bytes(_ACGT[b] for b in q).decode()))
    return "".join(out), "".join(unm)


def rows_by_read(text):
    out = {}
    for line in text.splitlines():
        f = line.split("\t")
        out.setdefault(f[0], set()).add(tuple(f[1:]))
    return out


__all__ = ["load_ref", "load_reads", "soap_single", "search", "rows_by_read", "Ref", "Hit"]

