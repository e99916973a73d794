"""Spec pgx-blastn v2, S3d (`blastn -dust "20 64 1"`), restated in plain Python: the mask and the window bits.

`dust_mask` is the DEFINITION of symmetric DUST (Morgulis, Gertz, Schaffer, Agarwala 2006) with exact fractions;
oracle/o_dust.c's `o_dust_mask` is the same in C (tests/test_oracle_classify.py proves the two equal) and serves where
volume is needed.  `window_bits` states what the seed stage reads, per strand one bit per read position:
    win_f[i] = (i + 28 <= L) and no masked base in [i, i + 28)
    win_r[i] = win_f[L - 28 - i]          (the reverse-complement strand: its mask is the forward mask reversed)
and every bit at or beyond L - 27 in the read's (L + 63) // 64 words is zero.
`crafted_reads` are the reads built to sit on the edges of the device's bookkeeping (csrc/dust.hip); tests/test_gpu_dust.py
compares the device's bits with the rule on them, oracle/fuzz_dust.c checks the first pass's range cut on them.
"""
import random

WORD = 28           # seed window (bases)
DUST_WINDOW = 64
DUST_LEVEL = 20


def dust_mask(seq, W=64, level=20):
    """S3d: the definition of symmetric DUST (Morgulis et al. 2006): triplet intervals of at most W - 2 triplets whose score
    (sum of c(c-1)/2 over triplet values, divided by triplets - 1) exceeds level / 10 and is not beaten by a sub-interval."""
    from fractions import Fraction
    n, nt = len(seq), len(seq) - 2
    mask = [False] * n
    if nt < 2:
        return mask
    trip = [seq[i:i + 3] if all(c in "ACGT" for c in seq[i:i + 3]) else None for i in range(nt)]
    best = {}   # (a, b) -> highest score of any sub-interval of [a, b] with at least two triplets, or None
    for a in range(nt - 1, -1, -1):
        cnt, r = {}, 0
        for b in range(a, min(nt, a + W - 2)):
            if trip[b] is None:
                break
            r += cnt.get(trip[b], 0)
            cnt[trip[b]] = cnt.get(trip[b], 0) + 1
            s = Fraction(r, b - a) if b > a else None
            subs = [x for x in (best.get((a + 1, b)), best.get((a, b - 1))) if x is not None]
            sub = max(subs) if subs else None
            if s is not None and s * 10 > level and (sub is None or sub <= s):
                for k in range(a, b + 3):
                    mask[k] = True
            cands = [x for x in (s, sub) if x is not None]
            best[(a, b)] = max(cands) if cands else None
    return mask


def canonical(seq):
    """The letters as the importer reads them: A C G T (U) in either case are bases, everything else is no base."""
    return "".join({"A": "A", "C": "C", "G": "G", "T": "T", "U": "T"}.get(c.upper(), "N") for c in seq)


def window_bits(mask):
    """(win_f, win_r) of a read from its mask (list of bool, one per base): lists of bool over all 64 * ((L + 63) // 64)
    positions of the read's words, False at and beyond L - 27."""
    L = len(mask)
    n_pos = 64 * ((L + 63) // 64)
    win_f = [False] * n_pos
    for i in range(L - WORD + 1):
        win_f[i] = not any(mask[i:i + WORD])
    win_r = [False] * n_pos
    for i in range(L - WORD + 1):
        win_r[i] = win_f[L - WORD - i]
    return win_f, win_r


def runs(mask):
    """Maximal masked stretches as (first, last) base."""
    out, i, n = [], 0, len(mask)
    while i < n:
        if mask[i]:
            j = i
            while j + 1 < n and mask[j + 1]:
                j += 1
            out.append((i, j))
            i = j + 1
        else:
            i += 1
    return out


def crafted_reads(seed=20):
    """[(name, letters)]: the reads of the issue's list.  Flanks are random bases (fixed seed) whose letter next to a
    repeat differs from the repeat's own continuation, so a stretch ends where it was put (the definition decides in the
    end: every test takes the mask from `dust_mask` / `o_dust_mask`, never from the construction)."""
    rng = random.Random(seed)
    out = []

    def rnd(n, not_first=None, not_last=None):
        s = [rng.choice("ACGT") for _ in range(n)]
        if n and not_first:
            s[0] = rng.choice([c for c in "ACGT" if c not in not_first])
        if n and not_last:
            s[-1] = rng.choice([c for c in "ACGT" if c not in not_last])
        return "".join(s)

    def rep(unit, n):
        return (unit * (n // len(unit) + 1))[:n]

    def embed(pre, body, post):
        """random pre / post flanks of the given lengths around `body`, not continuing its period"""
        core = "".join(c for c in body.upper() if c in "ACGTU")
        p = next(p for p in range(1, len(core) + 1) if core[p:] == core[:-p])
        return rnd(pre, not_last=core[p - 1]) + body + rnd(post, not_first=core[len(core) - p])

    def add(name, s):
        out.append((name, s))

    # lengths with no triplet pair, no valid window, exactly one valid window
    for L in (1, 2, 3, 4, 6, 7, 8, 27, 28, 29):
        add("homo_len%d" % L, "A" * L)
        add("rand_len%d" % L, rnd(L))
    # the level's edge: six of one letter (4 triplets, 6 / 3 = 2.0, not above), seven (10 / 4)
    for n in (6, 7, 8):
        add("homo%d_embedded" % n, embed(50, "C" * n, 60))
        add("homo%d_at_start" % n, embed(0, "G" * n, 60))
        add("homo%d_at_end" % n, embed(60, "T" * n, 0))
    # repeats of unit 1 .. 6
    for unit in ("A", "AC", "ACG", "ACGT", "AACGT", "AACCGT", "TTAGGG"):
        for n in (12, 40, 90):
            add("unit%s_x%d" % (unit, n), embed(45, rep(unit, n), 50))
    # a repeat of exactly k triplets (k + 2 bases): window full / leaving triplet (62), 64 interval starts (a chunk of
    # the second pass), two and three chunks
    for k in (61, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193):
        for unit in ("A", "ACG"):
            add("trip%d_%s_alone" % (k, unit), rep(unit, k + 2))
            add("trip%d_%s_embedded" % (k, unit), embed(33, rep(unit, k + 2), 31))
    # one repeat from end to end: about twenty chunks
    for unit in ("T", "AG", "AGC", "AAGTC"):
        add("all_repeat_1400_%s" % unit, rep(unit, 1400))
    add("all_repeat_1500_noisy", "".join(c if rng.random() > 0.02 else rng.choice("ACGT") for c in rep("CT", 1500)))
    # a triplet value recurring at a fixed distance d (exact period d), and five copies of one triplet whose first and
    # fifth lie d apart: the word of four positions mod 64 (d = 61: the fifth-most-recent is the window's oldest triplet;
    # 62, 63: it has just left)
    for d in (4, 5, 6, 31, 32, 33, 60, 61, 62, 63, 64, 65):
        unit = "CAG" + rnd(d - 3, not_first="C", not_last="C")
        add("period%d" % d, embed(20, rep(unit, 6 * d + 3), 20))
    for d in (12, 59, 60, 61, 62, 63, 64):
        s = list(rnd(40 + d + 83).replace("CAG", "CTG"))
        for p in sorted({0, d // 4, d // 2, 3 * d // 4, d, d + 30, d + 50}):
            s[40 + p:40 + p + 3] = "CAG"
        add("five_copies_span%d" % d, "".join(s))
    # masked stretches that start / end at the seams of the 64-bit words (the 28-wide OR across a word pair, the reverse
    # strand's funnel shift)
    for unit in ("A", "GT"):
        for e in (61, 62, 63, 64, 65, 66, 125, 126, 127, 128, 129, 130):
            n = 36
            add("ends_at%d_%s" % (e, unit), embed(e + 1 - n, rep(unit, n), 200 - e - 1))
            add("starts_at%d_%s" % (e, unit), embed(e, rep(unit, n), 230 - e - n))
    # ... and at the seams of the reverse strand: reads whose length moves the seam
    for L in (91, 92, 119, 120, 127, 128, 129, 155, 156, 157, 191, 192, 193, 219, 220, 221):
        add("len%d_masked_middle" % L, embed(L // 2 - 10, "A" * 20, L - L // 2 - 10))
        add("len%d_masked_start" % L, embed(0, rep("AC", 24), L - 24))
        add("len%d_masked_end" % L, embed(L - 24, rep("TG", 24), 0))
    # two masked stretches 27, 28, 29 free bases apart (26 and 30: should a flank letter join a stretch)
    for gap in (26, 27, 28, 29, 30):
        for pre in (10, 36, 37, 38, 50):
            a, b = rep("AC", 30), rep("GGT", 30)
            add("two_stretches_gap%d_at%d" % (gap, pre), rnd(pre, not_last="AC") + a + rnd(gap, not_first="AC", not_last="GT") + b +
                rnd(40, not_first="GT"))
    # letters that are no base: inside, just before and just after a repeat; IUPAC letters; lower case
    for x in "NRYKMSWBDHVn":
        add("amb_%s_inside" % x, embed(30, "A" * 20 + x + "A" * 20, 30))
        add("amb_%s_inside_short_halves" % x, embed(30, "A" * 6 + x + "A" * 7, 30))
        add("amb_%s_before" % x, rnd(30) + x + rep("AC", 40) + rnd(30, not_first="AC"))
        add("amb_%s_after" % x, rnd(30, not_last="AC") + rep("AC", 40) + x + rnd(30))
    add("amb_two_N_around", rnd(40) + "N" + rep("ACG", 70) + "N" + rnd(40))
    add("amb_N_first_and_last", "N" + rep("AT", 100) + "N")
    add("amb_N_runs_of_five", rnd(20) + "NNNNN" + "T" * 40 + "NNNNN" + rep("CA", 50) + "NNNNN")
    add("amb_long_read", embed(400, rep("AG", 100) + "N" + rep("AG", 100), 600))
    add("lower_case", embed(50, "a" * 30, 50).lower())
    add("mixed_case", "".join(c.lower() if i % 3 else c for i, c in enumerate(embed(50, rep("ct", 60).upper(), 50))))
    add("uracil", embed(50, "U" * 30, 50).replace("T", "U"))
    return out
