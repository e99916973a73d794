"""Spec pgx-blastn v2, S3d: the table word and the order of LDS operations of the first DUST pass's register form
(csrc/dust.hip: dust_scan_regs), on the CPU, no device.

One 32-bit word per triplet value: bits 24-29 the value's count in the window of the last 62 triplets, bits 30-31 the
number of its occurrences so far mod 4, bits 0-23 four slots of six bits with the positions (mod 64) of its last four
occurrences, occurrence n in slot n mod 4.  The kernel changes a word by atomics only and issues them in this order:
    ... sub(b), add(b), xor(b - 1), sub(b + 1), add(b + 1), xor(b), ...
(the leaving triplet's count down, the entering one's count and occurrence number up, and -- one position late -- the
entering position into the slot of its fifth-most-recent occurrence).  The model below runs exactly that sequence, every
read of a batch at once, with the kernel's arithmetic on what the two returning atomics gave, and must hand over what the
plain statement of the first pass (tests/test_dust_cut.py: first_pass, every position's window counted from scratch)
hands over: first, last, P and e0 of every listed read, and the same set of listed reads.  There is no tolerance.

The register form runs reads without ambiguity letters only, and every lane runs to the longest read's end on whatever
letters follow its own read: the model does too (zeros), and masks the test with the read's own length as the kernel does.
"""
import numpy as np
import pytest

from test_dust_cut import first_pass, triplets
from test_gpu_dust import FUZZ_CLASSES, Ref, fuzz_codes, fuzz_lengths

MAXT = 62
LEAVE, ENTER, M32 = 1 << 24, (1 << 24) + (1 << 30), 0xFFFFFFFF
BIG = 0x7FFFFFFF


def scan_regs(trip, nt):
    """first, last, P, e0 per read as dust_scan_regs computes them.  trip: (n, T) triplet values, anything >= 0 inside a
    read; nt: triplets per read."""
    n, T = trip.shape
    t_all = np.maximum(trip, 0).astype(np.int64)
    rows = np.arange(n)
    tab = np.zeros((n, 65), dtype=np.int64)
    first, last = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    p_last, p_max, rw = (np.zeros(n, dtype=np.int64) for _ in range(3))
    L, e0 = np.full(n, -1, dtype=np.int64), np.full(n, BIG, dtype=np.int64)
    # position -1: no pairs, a leaving count of 1, the spare word
    pend = (np.full(n, LEAVE, dtype=np.int64), np.zeros(n, dtype=np.int64), np.full(n, 64, dtype=np.int64))

    def finish(b, old_s, old_t, at):
        nonlocal rw, L, e0, p_max, first, last, p_last
        cnt, cs = (old_t >> 24) & 63, (old_s >> 24) & 63
        rw = rw + cnt - cs + 1
        sh = (old_t >> 30) * 6
        o = (old_t >> sh) & 63
        tab[rows, at] ^= (o ^ (b & 63)) << sh
        five = cnt >= 4
        L = np.minimum(L + 1, np.where(five, (b - o) & 63, MAXT))
        e0 = np.minimum(e0, np.where(five, b, BIG))
        p_max = np.maximum(p_max, rw)
        mine = (rw > 2 * L) & (b < nt)
        first = np.where(mine & (first < 0), b, first)
        last = np.where(mine, b, last)
        p_last = np.where(mine, p_max, p_last)

    for b in range(int(nt.max())):
        ns = np.full(n, LEAVE, dtype=np.int64)
        if b >= MAXT:
            s0 = t_all[:, b - MAXT]
            ns = tab[rows, s0].copy()
            tab[rows, s0] = (ns - LEAVE) & M32
        t = t_all[:, b]
        nv = tab[rows, t].copy()
        tab[rows, t] = (nv + ENTER) & M32
        finish(b - 1, *pend)
        pend = (ns, nv, t)
    finish(int(nt.max()) - 1, *pend)
    return first, last, p_last, e0


def check(ref, what):
    trip = triplets(ref)
    nt = ref.lens.astype(np.int64) - 2
    want = first_pass(trip)
    got = scan_regs(trip, nt)
    listed = want[0] >= 0
    assert np.array_equal(got[0] >= 0, listed), "%s: other reads are listed" % what
    for name, g, w in zip(("first", "last", "P", "e0"), got, want):
        bad = np.flatnonzero(listed & (g != w))
        assert not len(bad), "%s: %s of read %d is %d, the plain statement says %d: %s" % (what, name, bad[0], g[bad[0]], w[bad[0]], ref.seq(int(bad[0])))
    return int(listed.sum())


@pytest.mark.parametrize("name,max_len,n", [(c[0], c[1], max(100, c[2] // 40)) for c in FUZZ_CLASSES if not c[3] and c[1] <= 512])
def test_fuzz_classes(oracle_bin, name, max_len, n):
    """The generator of tests/test_gpu_dust.py, the three length classes the register form serves (ragged lengths: lanes
    past their read's end run on)."""
    rng = np.random.default_rng([43, max_len])
    lens = fuzz_lengths(rng, n, max_len)
    ref = Ref(fuzz_codes(rng, lens, False), lens)
    assert check(ref, "fuzz class " + name) >= 0.25 * n


def test_uniform_reads(oracle_bin):
    """4 000 uniform random reads of 150 bases (bench.py's case): 5-9 % are listed."""
    rng = np.random.default_rng(151)
    n = 4000
    ref = Ref(rng.integers(0, 4, n * 150).astype(np.uint8), np.full(n, 150))
    assert 0.05 * n <= check(ref, "uniform 150-base reads") <= 0.09 * n


def test_one_value_and_short_reads(oracle_bin):
    """Homopolymers (one word takes every atomic: the slot a position reads is never one a late XOR still has to write),
    period-2 to period-4 repeats, and reads shorter than one block of 16 positions and than the window."""
    seqs = ["A" * L for L in (3, 4, 7, 17, 18, 19, 63, 64, 65, 66, 80, 150, 192)]
    seqs += [(u * 200)[:L] for u in ("AC", "ACG", "ACGT", "AAC", "AACC") for L in (20, 66, 67, 130, 192)]
    ref = Ref.from_seqs(seqs)
    assert check(ref, "repeats") > len(seqs) // 2
