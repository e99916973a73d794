"""Timing aid for the unclassified-read selector on the bench batch (synthetic 1 Gbp database, 10 M reads of 150 bases):
the row pass (mask-only call), scans + unpack + the import's second half (the call that also builds the subset batch, minus
the mask-only call), and beside them the route this replaces -- pgx_hits_format -> pgx_unclas_file ->
pgx_reads_from_fasta_text -- on a slice of the batch, scaled to the batch.
usage: python3 tools/probe_unclas.py [--reads N] [--slice N] [--roof BYTES_PER_S]   (--roof: bench.py --full's streaming figure)"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pangea_plus_amd as pg  # noqa: E402
from pangea_plus_amd import _capi  # noqa: E402


def timed(f, reps=3):
    best, out = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--slice", type=int, default=200_000)
    ap.add_argument("--roof", type=float, default=0.0)
    a = ap.parse_args()
    pg.init(0)
    cfg = pg.SynthCfg.default()
    db = pg.Db.from_synth(cfg)
    reads = pg.Reads.from_synth(cfg, 0, a.reads)
    hits = _capi.blast_search(db, reads)
    slots = len(hits)
    t_mask, (mask, _) = timed(lambda: pg.unclassified(db, reads, hits, want_reads=False))
    t_all, (_, sub) = timed(lambda: pg.unclassified(db, reads, hits), reps=2)
    print("reads %d, slots %d, selected %d (%.1f %%)" % (a.reads, slots, int(mask.sum()), 100.0 * mask.mean()))
    print("mask only (thresholds on the host + row pass + mask + scan + download): %.1f ms" % (1e3 * t_mask))
    gbs = slots * 40 / t_mask / 1e9
    print("  upper bound of the row pass: %.0f GB/s of slot-table traffic (32-byte record + offset and count)%s" % (
        gbs, "; %.0f %% of the streaming roof" % (100 * gbs * 1e9 / a.roof) if a.roof else ""))
    print("scans + unpack + import's second half: %.1f ms (subset of %d reads)" % (1e3 * (t_all - t_mask), len(sub)))
    n = min(a.slice, a.reads)
    with tempfile.TemporaryDirectory() as d:
        part_reads = pg.Reads.from_synth(cfg, 0, n)
        part = hits.slice(0, n)
        t0 = time.perf_counter()
        open(d + "/m.tsv", "wb").write(part.format(db, part_reads))
        part_reads.write_fasta(d + "/s.fas")
        t1 = time.perf_counter()
        pg.unclassified_selector(["-m", d + "/m.tsv", "-s", d + "/s.fas", "-o", d + "/out.fas"])
        t2 = time.perf_counter()
        pg.Reads.from_fasta_text(open(d + "/out.fas", "rb").read())
        t3 = time.perf_counter()
    k = a.reads / n
    print("text route on %d reads, scaled x %.0f: format + write %.1f s, file verb %.1f s, import %.1f s" % (
        n, k, k * (t1 - t0), k * (t2 - t1), k * (t3 - t2)))


if __name__ == "__main__":
    main()
