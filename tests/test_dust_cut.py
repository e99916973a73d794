"""Spec pgx-blastn v2, S3d: the cuts the second DUST pass makes (csrc/dust.hip: k_dust_perfect), on the CPU, no device.

The first pass (k_dust_scan) is stated here plainly -- per position the window of the last at most 62 triplets counted from
scratch, as oracle/fuzz_dust.c states it -- with what it hands over for a listed read:
    first, last   the first and the last position at which the test 10 r_w > 20 L passes
    P             the largest window pair count r_w of any position 0 .. last
    e0            the first position at which a triplet value stood five times in the window
The second pass is the definition's recurrence as the kernel runs it: one lane per interval start, one step per interval
LENGTH, a lane reading its upper neighbour's pair counts and best score of the steps before, and a lane that is not
there read as zero pairs and no score.  It runs on
    existing cut   a >= first - 61, b <= last                     (pinned by oracle/fuzz_dust.c as well)
    length cap     l <= cap = min(62, (P - 1) // 2 + 1)           (pairs(a, b) <= r_w(b) <= P; a score above 2 needs 2 (l - 1) < P)
    lower start    a >= e0 - cap + 1                              (an interval above the level holds a value five times, so
                                                                  it ends at or after e0, and it is at most cap long)
and its mask must equal the definition's (o_dust_mask; tests/test_oracle_classify.py proves that equal to dust_rule.dust_mask)
exactly, as must the same recurrence under the existing cut alone.  There is no tolerance in this operation.

A bound on the start from ABOVE (a <= start(last) - 1, the suffix start at `last`: every interval above the level starts
at or before it) holds for the definition but saves the recurrence nothing: lane a takes pairs(a + 1, b) from lane a + 1,
so the lanes a <= a_hi are right up to length cap only when the lanes up to a_hi + cap - 2 run too, and
start(last) + cap - 3 >= last - 1 always (the test passed at `last`: P >= r_w > 2 L, so cap >= L + 1).  The kernel does
not make that cut; `test_a_missing_upper_lane_spoils_the_pair_counts` puts the reason on record.

The last test counts, on uniform random 150-base reads (bench.py's case), what the estimate of the gain rests on: the
share of listed reads and the steps of the second pass per listed read under the old and the new bounds.
"""
import numpy as np
import pytest

import dust_rule as R
from test_gpu_dust import FUZZ_CLASSES, Ref, fuzz_codes, fuzz_lengths

MAXT = 62
LEVEL = 20


# ------------------------------------------------------------------------------------------------ the first pass, plainly
def triplets(ref):
    """(n, T) triplet values of a batch (test_gpu_dust.Ref), -1 where a triplet holds a letter that is no base or lies
    beyond the read."""
    T = max(1, int(ref.lens.max()) - 2)
    trip = np.full((ref.n, T), -1, dtype=np.int16)
    for i in range(ref.n):
        c = ref.codes[ref.off[i]:ref.off[i + 1]].astype(np.int16)
        if len(c) >= 3:
            t = c[:-2] * 16 + c[1:-1] * 4 + c[2:]
            t[(c[:-2] > 3) | (c[1:-1] > 3) | (c[2:] > 3)] = -1
            trip[i, :len(t)] = t
    return trip


def first_pass(trip):
    """first, last, P, e0 per read (-1: never); every read of the batch at once, every position's window from scratch."""
    n, T = trip.shape
    first, last, e0 = (np.full(n, -1, dtype=np.int64) for _ in range(3))
    P, p_max, clean = (np.zeros(n, dtype=np.int64) for _ in range(3))
    pad = np.concatenate([np.full((n, MAXT - 1), -1, dtype=np.int16), trip], axis=1)
    values, ages = np.arange(64, dtype=np.int16)[None, None, :], np.arange(MAXT)[None, :]
    for b in range(T):
        ok = trip[:, b] >= 0
        clean = np.where(ok, clean + 1, 0)   # triplets since the last one that holds a letter that is no base
        rows = np.flatnonzero(ok)
        if not len(rows):
            continue
        size = np.minimum(clean[rows], MAXT)
        W = pad[rows, b:b + MAXT][:, ::-1]                        # W[:, j] = the triplet at b - j
        one_hot = (W[:, :, None] == values) & (ages < size[:, None])[:, :, None]
        seen = one_hot.cumsum(axis=1, dtype=np.int8)              # copies of each value among b, b - 1, ..., b - j
        cnt = seen[:, -1, :].astype(np.int64)
        rw = (cnt * (cnt - 1) // 2).sum(axis=1)
        nth = np.take_along_axis(seen, np.maximum(W, 0).astype(np.int64)[:, :, None], axis=2)[:, :, 0]   # W[:, j] is the nth copy from b back
        fifth = (nth > 4) & (ages < size[:, None])
        L = np.where(fifth.any(axis=1), fifth.argmax(axis=1), size)   # longest suffix with no value more than 4 times
        p_max[rows] = np.maximum(p_max[rows], rw)
        five = rows[cnt[np.arange(len(rows)), trip[rows, b]] >= 5]
        e0[five] = np.where(e0[five] < 0, b, e0[five])
        passed = rows[10 * rw > LEVEL * L]
        first[passed] = np.where(first[passed] < 0, b, first[passed])
        last[passed] = b
        P[passed] = p_max[passed]
    return first, last, P, e0


# ------------------------------------------------------------------------------------------------ the second pass
def bounds(nt, first, last, P, e0, new):
    """(a_lo, b_hi, cap) of a listed read under the existing cut (`new` false) or with the length cap and the lower start."""
    b_hi = min(last, nt - 1)
    if not new:
        return max(0, first - (MAXT - 1)), b_hi, MAXT
    cap = min(MAXT, (P - 1) // 2 + 1)
    return max(0, first - (MAXT - 1), e0 - cap + 1), b_hi, cap


def steps(a_lo, b_hi, cap):
    """Steps of the kernel's loop: chunks of 64 starts from the top, each l = 2 .. min(cap, b_hi - a0 + 1)."""
    return sum(max(0, min(cap, b_hi - a0 + 1) - 1) for a0 in range(a_lo, b_hi + 1, 64))


def lanes_mask(trip, n_bases, a_lo, b_hi, cap, a_top=None):
    """The definition's recurrence over the interval length, one lane per start a_lo .. a_top (default b_hi), a missing
    lane read as zero pairs and no score; scores as exact fractions in integers.  Returns the masked bases."""
    a_top = b_hi if a_top is None else a_top
    mask = np.zeros(n_bases, dtype=np.uint8)
    if a_top < a_lo:
        return mask
    a = np.arange(a_lo, a_top + 1)
    far = np.concatenate([trip, np.full(MAXT + 1, -1, dtype=trip.dtype)]).astype(np.int64)
    ta = far[a]
    live = ta >= 0
    z = np.zeros(len(a), dtype=np.int64)
    P1, P2, Bn, Bq, end = z.copy(), z.copy(), z.copy(), z + 1, z - 1

    def up(x, none):
        return np.concatenate([x[1:], [none]])
    for l in range(2, min(cap, b_hi - a_lo + 1) + 1):
        nP1, nP2, nBn, nBq = up(P1, 0), up(P2, 0), up(Bn, 0), up(Bq, 1)
        tb = far[a + l - 1]
        live = live & (tb >= 0) & (a + l - 1 <= b_hi)
        Pl, q = P1 + nP1 - nP2 + (tb == ta), l - 1
        up_better = nBn * Bq > Bn * nBq
        sn, sq = np.where(up_better, nBn, Bn), np.where(up_better, nBq, Bq)
        lhs, rhs = sn * q, Pl * sq                     # a sub-interval beats the score <=> lhs > rhs
        end = np.where(live & (Pl * 10 > LEVEL * q) & (lhs <= rhs), a + l + 1, end)
        P2, P1 = P1, np.where(live, Pl, 0)
        Bn = np.where(live, np.where(rhs > lhs, Pl, sn), 0)
        Bq = np.where(live, np.where(rhs > lhs, q, sq), 1)
    for s, e in zip(a[end >= 0], end[end >= 0]):
        mask[s:e + 1] = 1
    return mask


def check_batch(ref, what):
    """Every read of `ref`: the recurrence under the old and under the new bounds gives the definition's mask; a read with a
    masked base is listed.  Returns (listed, old steps, new steps) per read."""
    trip = triplets(ref)
    first, last, P, e0 = first_pass(trip)
    listed = first >= 0
    assert not np.any((ref.any != 0) & ~listed), "%s: a read with a masked base is not listed" % what
    old_steps, new_steps = np.zeros(ref.n, dtype=np.int64), np.zeros(ref.n, dtype=np.int64)
    for i in np.flatnonzero(listed):
        L = int(ref.lens[i])
        nt, t = L - 2, trip[i, :L - 2]
        want = ref.mask[ref.off[i]:ref.off[i + 1]]
        f, la, p, e = int(first[i]), int(last[i]), int(P[i]), int(e0[i])
        assert 0 <= e <= f <= la and p > 2, (what, i, f, la, p, e)   # (no window count of 5: pairs <= 1.5 l, the test cannot pass)
        for new in (False, True):
            a_lo, b_hi, cap = bounds(nt, f, la, p, e, new)
            got = lanes_mask(t, L, a_lo, b_hi, cap)
            if not np.array_equal(got, want):
                k = int(np.flatnonzero(got != want)[0])
                raise AssertionError("%s: read %d (%s bounds: a >= %d, b <= %d, l <= %d; first %d last %d P %d e0 %d) differs at base %d: %s"
                                     % (what, i, "new" if new else "old", a_lo, b_hi, cap, f, la, p, e, k, ref.seq(i)))
            (new_steps if new else old_steps)[i] = steps(a_lo, b_hi, cap)
    return listed, old_steps, new_steps


def test_crafted_reads(oracle_bin):
    crafted = R.crafted_reads()
    ref = Ref.from_seqs([R.canonical(s) for _n, s in crafted])
    listed, old, new = check_batch(ref, "crafted reads")
    assert listed.sum() > 200 and np.all(new <= old)


@pytest.mark.parametrize("name,max_len,n,with_n", [(c[0], c[1], max(100, c[2] // 40), c[3]) for c in FUZZ_CLASSES])
def test_fuzz_classes(oracle_bin, name, max_len, n, with_n):
    """The generator of tests/test_gpu_dust.py, all five length classes (a fortieth of the device test's volume each)."""
    rng = np.random.default_rng([41, max_len, int(with_n)])
    lens = fuzz_lengths(rng, n, max_len)
    ref = Ref(fuzz_codes(rng, lens, with_n), lens)
    listed, old, new = check_batch(ref, "fuzz class " + name)
    assert 0.25 * n <= (ref.any != 0).sum() <= 0.75 * n and np.all(new <= old)
    if with_n:
        has_n = np.array([np.any(ref.codes[ref.off[i]:ref.off[i + 1]] == 4) for i in range(n)])
        assert np.sum(has_n & (ref.any != 0)) > 0


def test_a_missing_upper_lane_spoils_the_pair_counts(oracle_bin):
    """Why the second pass keeps the lanes up to `last`: a homopolymer run of 40 inside random flanks; with the lanes above
    the run's first triplet left out, the lane below them counts no pairs beyond its first and the mask is lost."""
    rng = np.random.default_rng(3)
    s = "".join("CGT"[x] for x in rng.integers(0, 3, 50)) + "A" * 40 + "".join("CGT"[x] for x in rng.integers(0, 3, 50))
    ref = Ref.from_seqs([s])
    trip = triplets(ref)
    first, last, P, e0 = (int(x[0]) for x in first_pass(trip))
    a_lo, b_hi, cap = bounds(len(s) - 2, first, last, P, e0, True)
    want = ref.mask[:len(s)]
    assert want[50:90].all()
    assert np.array_equal(lanes_mask(trip[0, :len(s) - 2], len(s), a_lo, b_hi, cap), want)
    assert not np.array_equal(lanes_mask(trip[0, :len(s) - 2], len(s), a_lo, b_hi, cap, a_top=50), want)


def test_uniform_reads_and_the_steps_the_estimate_rests_on(oracle_bin):
    """12 000 uniform random reads of 150 bases.  Asserted: masks equal under both bounds (check_batch); 5-9 % of the reads
    are listed (7 %); the new bounds run at most 0.4 of the old steps per listed read -- a random window
    of 62 triplets holds about 62 * 61 / 2 / 64 = 30 pairs and a listed read's 35-45, a cap of 18-23 of the 61 lengths
    (23 / 61 = 0.38), and the old bounds often run a second chunk on top.  Counted on this sample (printed below):
    7.35 % listed (2.65 % with a masked base), 62.7 steps per listed read under the old bounds (57 % of them in two
    chunks; a read whose test first passes near its start has a short one), 22.6 under the new (1 % in two chunks): a
    factor 2.78."""
    rng = np.random.default_rng(150)
    n = 12000
    ref = Ref(rng.integers(0, 4, n * 150).astype(np.uint8), np.full(n, 150))
    listed, old, new = check_batch(ref, "uniform 150-base reads")
    share, m_old, m_new = float(listed.mean()), float(old[listed].mean()), float(new[listed].mean())
    print("uniform reads: listed %.4f, masked %.4f, steps per listed read old %.2f new %.2f (factor %.2f), one chunk: old %.3f new %.3f"
          % (share, float((ref.any != 0).mean()), m_old, m_new, m_old / m_new, float((old[listed] <= 61).mean()), float((new[listed] <= 61).mean())))
    assert 0.05 <= share <= 0.09
    assert m_new <= 0.4 * m_old
