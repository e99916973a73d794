"""Spec pgx-blastn v2, S3d on the device (csrc/dust.hip: k_dust_scan<NW>, k_dust_perfect, k_dust_windows), bit for bit against
the definition: the per-read `any` flags, the masked bases and the window bits of both strands, read back whole with
pgx_reads_get_dust / pgx_db_get_dust and compared with tests/dust_rule.py's statement (the mask itself from `o_dust_mask` of
liboracle.so, which tests/test_oracle_classify.py proves equal to the Python definition; the crafted reads are compared with
the Python definition as well).  Exact equality: there is no tolerance in this operation.  The words of reads without a
masked base are undefined (the kernels never write them) and are not compared; their `any` flag is.

A BLAST table is nearly blind to a wrong window bit (every seed of a diagonal extends to the same HSP), so the last test
builds reads whose table does depend on one bit: exact copies of database stretches with 0, 1 or 2 unmasked windows.
"""
import concurrent.futures
import ctypes
import multiprocessing
import os

import numpy as np
import pytest

import dust_rule as R
from conftest import ORACLE_DIR, run_cmd

gpu = pytest.mark.gpu

# reads of the volume fuzz per seed and length class (five classes: up to 192, 320, 512, 1 500 bases, and up to 320 with an
# occasional N): 144 000 reads, 27 M bases a seed, two default seeds; `o_dust_mask` over 16 threads (ctypes releases the
# interpreter lock around the call) takes about 10 s a seed on 8 CPUs, the bit packing and comparison about as long.
FUZZ_CLASSES = (("le192", 192, 60000, False), ("le320", 320, 40000, False), ("le512", 512, 20000, False), ("le1500", 1500, 4000, False),
                ("le320_N", 320, 20000, True))
FUZZ_SEEDS = [int(x) for x in os.environ.get("PGX_DUST_BITS_SEEDS", "31,32").split(",")]
EDGE_LENGTHS = (1, 2, 3, 8, 27, 28, 29, 63, 64, 65, 66, 91, 92, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 383, 384, 385,
                511, 512, 513, 640, 1023, 1024, 1399, 1400)
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3
LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the reference side
class Ref:
    """Codes (0-3 bases, 4 none) of a batch's reads back to back, and the definition's mask of each (o_dust_mask)."""

    def __init__(self, codes, lens):
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.n = len(self.lens)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        assert self.off[-1] == len(self.codes)
        self.mask = np.zeros(max(1, len(self.codes)), dtype=np.uint8)
        lib = ctypes.CDLL(os.path.join(ORACLE_DIR, "liboracle.so"))
        lib.o_dust_mask.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        lib.o_dust_mask.restype = None
        src, dst, off, ln = self.codes.ctypes.data, self.mask.ctypes.data, self.off.tolist(), self.lens.tolist()

        def work(lo, hi):
            for i in range(lo, hi):
                lib.o_dust_mask(src + off[i], ln[i], dst + off[i])
        step = max(1, (self.n + 255) // 256)
        with concurrent.futures.ThreadPoolExecutor(max_workers=16) as ex:
            for f in [ex.submit(work, lo, min(self.n, lo + step)) for lo in range(0, self.n, step)]:
                f.result()
        self.mask = self.mask[:len(self.codes)]
        self.read_of = np.repeat(np.arange(self.n), self.lens)
        self.pos = np.arange(len(self.codes), dtype=np.int64) - self.off[self.read_of]
        self.any = np.zeros(self.n, dtype=np.uint8)
        self.any[self.read_of[self.mask != 0]] = 1

    @classmethod
    def from_seqs(cls, seqs):
        text = "".join(seqs).encode("latin-1")
        return cls(_CODE[np.frombuffer(text, dtype=np.uint8)] if text else np.zeros(0, np.uint8), [len(s) for s in seqs])

    def seq(self, i):
        return LETTERS[self.codes[self.off[i]:self.off[i + 1]]].tobytes().decode()

    def fasta(self):
        """FASTA text of the batch, names r0, r1, ... (one sequence line per read)."""
        n, total = self.n, int(self.off[-1])
        names = [b">r%d\n" % i for i in range(n)]
        name_len = np.array([len(x) for x in names], dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(name_len + self.lens + 1)])
        out = np.full(int(start[-1]), ord("\n"), dtype=np.uint8)
        nb = np.frombuffer(b"".join(names), dtype=np.uint8)
        n_off = np.concatenate([[0], np.cumsum(name_len)])
        out[np.repeat(start[:-1] - n_off[:-1], name_len) + np.arange(len(nb))] = nb
        out[np.repeat(start[:-1] + name_len - self.off[:-1], self.lens) + np.arange(total)] = LETTERS[self.codes]
        return out.tobytes()

    def runs(self):
        """(read, first, last) of every maximal masked stretch, as three arrays."""
        m = self.mask != 0
        prev = np.concatenate([[False], m[:-1]]) & (self.pos > 0)
        nxt = np.concatenate([m[1:], [False]]) & (self.pos + 1 < self.lens[self.read_of])
        s, e = np.flatnonzero(m & ~prev), np.flatnonzero(m & ~nxt)
        return self.read_of[s], self.pos[s], self.pos[e]

    def words(self, woff, n_words):
        """The rule's words at the device's offsets: (mask, win_f, win_r, own) -- `own`: words that belong to a read --
        and `in_read`, the bits below each read's length.  The window rule of dust_rule.window_bits, vectorised (the
        crafted-reads test compares the two statements)."""
        lens_at, g = self.lens[self.read_of], np.arange(len(self.codes), dtype=np.int64)
        c = np.concatenate([[0], np.cumsum(self.mask != 0)])
        valid = self.pos + R.WORD <= lens_at
        wf = valid & (c[np.minimum(g + R.WORD, len(self.codes))] - c[g] == 0)
        wr = np.zeros_like(wf)
        wr[valid] = wf[(self.off[self.read_of] + lens_at - R.WORD - self.pos)[valid]]
        bit = woff[self.read_of].astype(np.int64) * 64 + self.pos

        def pack(flags):
            b = np.zeros(n_words * 64, dtype=np.uint8)
            b[bit[flags]] = 1
            return np.packbits(b.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)
        nw = (self.lens + 63) // 64
        own = np.zeros(n_words, dtype=bool)
        own[np.repeat(woff[:-1].astype(np.int64) - np.concatenate([[0], np.cumsum(nw)])[:-1], nw) + np.arange(int(nw.sum()))] = True
        return pack(self.mask != 0), pack(wf), pack(wr), own, pack(np.ones(len(self.codes), dtype=bool))


def bits_text(word_array, w0, nw):
    return "".join("".join("1" if (int(w) >> k) & 1 else "." for k in range(64)) for w in word_array[w0:w0 + nw])


def assert_bits(ref, got, what):
    """The device's (any, woff, mask, win_f, win_r) equal the rule for every read of the batch."""
    any_d, woff, mask_d, wf_d, wr_d = got
    assert len(any_d) == ref.n and len(woff) == ref.n + 1, what
    nw = (ref.lens + 63) // 64
    assert np.all(np.diff(woff.astype(np.int64)) >= nw) and int(woff[-1]) == len(mask_d), what
    mask_r, wf_r, wr_r, own, in_read = ref.words(woff, len(mask_d))
    word_read = np.full(len(mask_d), -1, dtype=np.int64)
    word_read[own] = np.repeat(np.arange(ref.n), nw)
    compared = own & (ref.any[np.maximum(word_read, 0)] != 0)
    bad_read = None
    if not np.array_equal(any_d != 0, ref.any != 0):
        bad_read, field = int(np.flatnonzero((any_d != 0) != (ref.any != 0))[0]), "any"
    else:
        for field, d, r in (("mask", mask_d & in_read, mask_r), ("win_f", wf_d, wf_r), ("win_r", wr_d, wr_r)):
            bad = np.flatnonzero(compared & (d != r))
            if len(bad):
                bad_read = int(word_read[bad[0]])
                break
    if bad_read is None:
        return
    i, L = bad_read, int(ref.lens[bad_read])
    w0, n = int(woff[i]), int(nw[i])
    lines = ["%s: read %d of %d (%d bases) differs in `%s`; device any %d, rule any %d" % (what, i, ref.n, L, field, any_d[i], ref.any[i]),
             ref.seq(i)]
    for name, d, r in (("mask", mask_d, mask_r), ("win_f", wf_d, wf_r), ("win_r", wr_d, wr_r)):
        a, b = bits_text(d, w0, n), bits_text(r, w0, n)
        first = next((k for k in range(len(a)) if a[k] != b[k]), None)
        lines.append("%s: first differing position %s" % (name, first))
        if first is not None:
            lo = max(0, first - 40)
            lines += ["  device %5d: %s" % (lo, a[lo:first + 40]), "  rule   %5d: %s" % (lo, b[lo:first + 40])]
    print("\n".join(lines))
    raise AssertionError(lines[0])


# ------------------------------------------------------------------------------------------------ generators
def fuzz_codes(rng, lens, with_n):
    """oracle/fuzz_dust.c's kinds: uniform, AT-rich, noisy repeats of unit 1-6 (the first of a read up to 200 bases), and
    with `with_n` an N in one read of three."""
    lens = np.asarray(lens, dtype=np.int64)
    n, total = len(lens), int(lens.sum())
    off = np.concatenate([[0], np.cumsum(lens)])
    kind = rng.integers(0, 6, n)
    biased = (kind == 5) & (rng.integers(0, 4, n) != 0)
    codes = rng.integers(0, 4, total).astype(np.uint8)
    at = np.repeat(biased, lens) & (rng.random(total) < 0.8)
    codes[at] = (rng.integers(0, 2, int(at.sum())) * 3).astype(np.uint8)
    for i in np.flatnonzero((kind >= 2) & (kind <= 4)):
        L = int(lens[i])
        for r in range(int(rng.integers(1, 4))):
            unit, s0, noise = int(rng.integers(1, 7)), int(rng.integers(0, L)), int(rng.integers(0, 12))
            rl = min(L - s0, 4 + int(rng.integers(0, 197 if r == 0 else 60)))
            body = rng.integers(0, 4, unit).astype(np.uint8)[np.arange(rl) % unit]
            if noise >= 3:
                hit = rng.integers(0, 12, rl) < noise // 3
                body[hit] = rng.integers(0, 4, int(hit.sum()))
            codes[off[i] + s0:off[i] + s0 + rl] = body
    if with_n:
        for i in np.flatnonzero(rng.integers(0, 3, n) == 0):
            codes[off[i] + int(rng.integers(0, lens[i]))] = 4
    return codes


def fuzz_lengths(rng, n, max_len):
    """mostly the class's own upper range (so the batch's longest read picks the wanted kernel form), some short"""
    lo = {192: 20, 320: 100, 512: 200, 1500: 300}[max_len]
    lens = rng.integers(lo, max_len + 1, n)
    short = rng.integers(0, 8, n) == 0
    lens[short] = rng.integers(20, 150, int(short.sum()))
    lens[0] = max_len
    return lens


def fuzz_batch(seed, name, max_len, n, with_n):
    rng = np.random.default_rng([seed, max_len, int(with_n)])
    lens = fuzz_lengths(rng, n, max_len)
    return Ref(fuzz_codes(rng, lens, with_n), lens)


def honesty(ref):
    """What keeps a fuzz batch honest, counted from the reference alone."""
    rd, first, last = ref.runs()
    n_runs = np.bincount(rd, minlength=ref.n)
    long_run = np.zeros(ref.n, dtype=bool)
    long_run[rd[last - first + 1 >= 100]] = True
    has_n = np.zeros(ref.n, dtype=bool)
    has_n[ref.read_of[ref.codes == 4]] = True
    return dict(masked=float(np.mean(ref.any != 0)), long_run=float(np.mean(long_run)), two_runs=float(np.mean(n_runs >= 2)),
                n_and_masked=int(np.sum(has_n & (ref.any != 0))))


def assert_honest(batches):
    """`batches`: {class name: Ref}.  In every length class at least a quarter of the reads have a masked base and at least a
    quarter have none; over all, at least 1 % have a masked stretch of 100 bases or more, at least 1 % two separate
    stretches, and reads with an N and a masked base exist."""
    hs = {k: honesty(b) for k, b in batches.items()}
    print("fuzz conditions:", hs)
    for k, h in hs.items():
        assert 0.25 <= h["masked"] <= 0.75, (k, h)
    n = sum(b.n for b in batches.values())
    assert sum(hs[k]["long_run"] * batches[k].n for k in hs) >= 0.01 * n
    assert sum(hs[k]["two_runs"] * batches[k].n for k in hs) >= 0.01 * n
    assert sum(h["n_and_masked"] for h in hs.values()) > 0


def edge_batch(seed, max_len, n, with_n=False):
    """`n` reads of the fuzz's kinds whose longest is exactly `max_len`, the edge lengths mixed among random ones so that
    every wavefront of 64 reads holds short and long reads (reads with no triplet, no valid window, exactly one)."""
    rng = np.random.default_rng([seed, max_len, n, int(with_n)])
    edges = [x for x in EDGE_LENGTHS if x <= max_len]
    lens = np.where(rng.integers(0, 2, n) == 0, rng.choice(edges, n), rng.integers(1, max_len + 1, n))
    lens[rng.integers(0, n)] = max_len
    codes = fuzz_codes(rng, lens, False)
    if with_n:
        i = int(rng.integers(0, n))
        codes[int(np.concatenate([[0], np.cumsum(lens)])[i]) + int(rng.integers(0, lens[i]))] = 4
    return Ref(codes, lens)


@pytest.fixture(scope="module")
def pg():
    import pangea_plus_amd as pg
    pg.init(0)
    return pg


# ------------------------------------------------------------------------------------------------ CPU: the inputs
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_generator_meets_its_conditions(oracle_bin, seed):
    """The volume fuzz's inputs, judged by the reference alone (no device): the conditions of `assert_honest`.  On a smaller
    sample of each class than the device test's (the same generator and seeds; the device test asserts the same on its own)."""
    assert_honest({name: fuzz_batch(seed, name, max_len, max(2000, n // 8), with_n) for name, max_len, n, with_n in FUZZ_CLASSES})


def test_window_rule_vectorised_equals_the_plain_statement(oracle_bin):
    """Ref.words (what the device is compared with) against dust_rule.window_bits on the crafted reads and a mixed batch."""
    crafted = [R.canonical(s) for _n, s in R.crafted_reads()]
    ref = Ref.from_seqs(crafted + [edge_batch(1, 513, 300).seq(i) for i in range(300)])
    nw = (ref.lens + 63) // 64
    woff = np.concatenate([[0], np.cumsum(nw + 1)]).astype(np.uint32)   # (a spare word behind every read)
    mask_w, wf_w, wr_w, own, in_read = ref.words(woff, int(woff[-1]))
    assert int(own.sum()) == int(nw.sum())
    for i in range(ref.n):
        m = [bool(x) for x in ref.mask[ref.off[i]:ref.off[i + 1]]]
        wf, wr = R.window_bits(m)
        w0, k = int(woff[i]), int(nw[i])
        assert bits_text(mask_w, w0, k) == "".join("1" if x else "." for x in m).ljust(64 * k, "."), i
        assert bits_text(in_read, w0, k) == ("1" * len(m)).ljust(64 * k, "."), i
        assert bits_text(wf_w, w0, k) == "".join("1" if x else "." for x in wf), i
        assert bits_text(wr_w, w0, k) == "".join("1" if x else "." for x in wr), i
        assert not any(wf[max(0, len(m) - 27):]) and not any(wr[max(0, len(m) - 27):])
        assert not own[w0 + k]


# ------------------------------------------------------------------------------------------------ GPU: bits == rule
def device_bits(pg, ref):
    reads = pg.Reads.from_fasta_text(ref.fasta())
    assert len(reads) == ref.n
    return reads, reads.dust_bits()


@gpu
@pytest.mark.parametrize("max_len", [192, 193, 320, 321, 512, 513, 1400])
def test_every_scan_form_and_its_edges(pg, oracle_bin, max_len):
    """Batches whose longest read is `max_len` (k_dust_scan<6> up to 192, <10> up to 320, <16> up to 512, <0> beyond), of 1, 63,
    64, 65 and 3 000 reads, lengths mixed inside every wavefront."""
    for n in (1, 63, 64, 65, 3000):
        ref = edge_batch(7, max_len, n)
        assert int(ref.lens.max()) == max_len
        reads, got = device_bits(pg, ref)
        assert "".join("ACGTN"[b] for b in reads.get(n - 1)) == ref.seq(n - 1)
        assert_bits(ref, got, "longest %d, %d reads" % (max_len, n))


@gpu
def test_one_n_read_sends_a_short_batch_through_the_any_length_form(pg, oracle_bin):
    """At most 192 bases and a single read with an N: k_dust_scan<0> with ambiguity flags for every read."""
    for n in (1, 63, 64, 65, 3000):
        ref = edge_batch(8, 192, n, with_n=True)
        assert int((ref.codes == 4).sum()) == 1
        assert_bits(ref, device_bits(pg, ref)[1], "one N, %d reads" % n)


def _definition(seq):
    return R.dust_mask(seq)


@gpu
def test_crafted_reads(pg, oracle_bin):
    """tests/dust_rule.py: crafted_reads, as one batch (an N among them: the any-length form), as one batch without the
    reads that hold a letter that is no base (up to 1 500 bases: the any-length form without flags), the short ones of those
    alone (the register forms), and every read as a batch of its own.  The reference mask is checked against the Python
    definition first."""
    crafted = R.crafted_reads()
    seqs = [R.canonical(s) for _n, s in crafted]
    ref = Ref.from_seqs(seqs)
    with concurrent.futures.ProcessPoolExecutor(max_workers=16, mp_context=multiprocessing.get_context("spawn")) as ex:
        plain = list(ex.map(_definition, seqs, chunksize=4))
    for i, (name, _s) in enumerate(crafted):
        assert [bool(x) for x in ref.mask[ref.off[i]:ref.off[i + 1]]] == plain[i], name
    assert ref.any.sum() > 200 and (ref.any == 0).sum() > 20

    def batch(pick, what, letters=None):
        sub = Ref.from_seqs([seqs[i] for i in pick])
        text = sub.fasta() if letters is None else "".join(">r%d\n%s\n" % (k, letters[i]) for k, i in enumerate(pick)).encode()
        reads = pg.Reads.from_fasta_text(text)
        try:
            assert_bits(sub, reads.dust_bits(), what)
        except AssertionError as e:
            raise AssertionError("%s (%s)" % (e, [crafted[i][0] for i in pick][:3]))
    # the letters as written (IUPAC letters, lower case, U), then by kernel form
    batch(range(len(seqs)), "all crafted reads, letters as written", letters=[s for _n, s in crafted])
    clean = [i for i, s in enumerate(seqs) if "N" not in s]
    batch(clean, "crafted reads without N")
    for top in (192, 320, 512):
        batch([i for i in clean if len(seqs[i]) <= top], "crafted reads without N up to %d bases" % top)
    for i in range(len(seqs)):
        batch([i], "crafted read %s alone" % crafted[i][0], letters=[s for _n, s in crafted])


@gpu
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_volume_fuzz(pg, oracle_bin, seed):
    """144 000 reads per seed in five batches (FUZZ_CLASSES): every bit of every read against the rule."""
    batches = {name: fuzz_batch(seed, name, max_len, n, with_n) for name, max_len, n, with_n in FUZZ_CLASSES}
    assert_honest(batches)
    for name, ref in batches.items():
        assert_bits(ref, device_bits(pg, ref)[1], "fuzz seed %d class %s" % (seed, name))


def _small_db(pg, tmp_path, rng, n=6, L=900):
    fa = tmp_path / "db.fa"
    fa.write_text("".join(">gi|%d|x|s%d|\n%s\n" % (i + 1, i, "".join("ACGT"[x] for x in rng.integers(0, 4, L))) for i in range(n)))
    return pg.Db.from_fasta(str(fa))


@gpu
def test_same_bits_by_every_route(pg, oracle_bin, tmp_path):
    """One mixed batch: after import, after pgx_reads_redo_dust, and in the handle's workspace after a search with
    set_dust_each_search(True).  Then the stale-buffer case: through ONE handle with each-search on, a large heavily
    masked batch first and a small, differently laid-out batch second (the buffers are reused, `mask` is cleared per listed
    read only): the second batch's workspace bits equal the rule."""
    from pangea_plus_amd import _capi
    rng = np.random.default_rng(5)
    db = _small_db(pg, tmp_path, rng)
    ref = edge_batch(9, 700, 5000)
    reads, got = device_bits(pg, ref)
    assert_bits(ref, got, "after import")
    reads.redo_dust()
    assert_bits(ref, reads.dust_bits(), "after redo_dust")
    db.set_dust_each_search(True)
    _capi.blast_search(db, reads)
    assert _capi.stage_times().dust_ms > 0
    assert_bits(ref, db.dust_bits(reads), "workspace after a search")
    assert_bits(ref, reads.dust_bits(), "the batch's own bits after that search")
    # stale buffers: heavy first ...
    lens = rng.integers(150, 400, 20000)
    read_of = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(int(lens.sum())) - np.repeat(np.concatenate([[0], np.cumsum(lens)])[:-1], lens)
    pair = rng.integers(0, 4, (len(lens), 2)).astype(np.uint8)          # every read one dinucleotide repeat
    heavy = Ref(pair[read_of, pos % 2], lens)
    assert heavy.mask.mean() > 0.7
    h_reads = pg.Reads.from_fasta_text(heavy.fasta())
    _capi.blast_search(db, h_reads)
    assert_bits(heavy, db.dust_bits(h_reads), "workspace, heavily masked batch")
    # ... then small batches laid out otherwise
    for n, max_len in ((300, 513), (64, 192), (1, 1400)):
        small = edge_batch(10, max_len, n)
        s_reads = pg.Reads.from_fasta_text(small.fasta())
        _capi.blast_search(db, s_reads)
        assert_bits(small, db.dust_bits(s_reads), "workspace, %d reads after the heavy batch" % n)
    db.set_dust_each_search(False)


# ------------------------------------------------------------------------------------------------ tables that depend on one bit
def _one_window_reads(rng, want_per_cell=3):
    """[(read, n_windows)]: a masked repeat, 27 / 28 / 29 free bases, a masked repeat, 150 / 400 / 700 bases in all; kept only
    when the definition's mask of the finished read leaves exactly the wanted 0 / 1 / 2 windows of 28 unmasked bases."""
    units = ["A", "C", "AC", "GT", "AG", "ACG", "GGT", "CT", "TTC", "AAT"]
    out = []
    for L in (150, 400, 700):
        for k in (27, 28, 29):
            kept = 0
            for attempt in range(200):
                if kept == want_per_cell:
                    break
                n1 = int(rng.integers(30, L - k - 30))
                u1, u2 = (units[int(x)] for x in rng.choice(len(units), 2, replace=False))
                free = "".join("ACGT"[x] for x in rng.integers(0, 4, k))
                s = (u1 * L)[:n1] + free + (u2 * L)[:L - n1 - k]
                ref = Ref.from_seqs([s])
                wf, _wr = R.window_bits([bool(x) for x in ref.mask])
                if sum(wf) == k - 27:
                    out.append((s, k - 27))
                    kept += 1
            assert kept == want_per_cell, (L, k)
    return out


@gpu
def test_tables_that_depend_on_one_window_bit(pg, oracle_bin, tmp_path):
    """Reads that are exact copies of database stretches (both orientations) with exactly 0, 1 or 2 unmasked 28-base windows:
    the product's table equals the oracle's byte for byte, and by the ORACLE's table the 0-window reads have no row and
    the 1-window reads have one.  Reads of 150, 400 and 700 bases: the seed kernel's dense and any-length forms reading
    `dustwin_f` / `dustwin_r`."""
    rng = np.random.default_rng(77)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    made = _one_window_reads(rng)

    def rnd(n):
        return "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    db, rd = tmp_path / "w.fa", tmp_path / "w_reads.fa"
    db.write_text("".join(">gi|%d|x|w%d|\n%s\n" % (i + 1, i, rnd(120) + s + rnd(120)) for i, (s, _k) in enumerate(made)))
    names, text = {}, []
    for i, (s, k) in enumerate(made):
        for o, seq in (("f", s), ("r", "".join(comp[c] for c in reversed(s)))):
            names["q%d%s" % (i, o)] = k
            text.append(">q%d%s\n%s\n" % (i, o, seq))
    rd.write_text("".join(text))
    want = tmp_path / "w_oracle.tsv"
    assert run_cmd([oracle_bin, "blastn", "-query", str(rd), "-db", str(db), "-outfmt", "6", "-out", str(want), "-num_threads", "8"], timeout=900)[0] == 0
    rows = {}
    for l in want.read_text().splitlines():
        rows[l.split("\t")[0]] = rows.get(l.split("\t")[0], 0) + 1
    for q, k in names.items():
        if k == 0:
            assert q not in rows, q
        elif k == 1:
            assert rows.get(q) == 1, q
        else:
            assert rows.get(q, 0) >= 1, q
    assert sum(1 for k in names.values() if k == 0) >= 18 and sum(1 for k in names.values() if k == 1) >= 18
    pg.makeblastdb(str(db), str(tmp_path / "wdb"))
    out = tmp_path / "w.tsv"
    pg.blastn(str(rd), str(tmp_path / "wdb"), str(out))
    assert out.read_bytes() == want.read_bytes()
