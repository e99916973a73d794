"""Reads per second of the barcode demultiplexer: the file verb (pg.barcode: files in, files out) and the resident form
(pg.barcode_reads, then a batch per barcode) on a generated 454-style FASTA -- by default 2 M reads of 250 bases at 60
letters a line, 96 barcodes of 8 letters; 90 % of the reads begin with a barcode, 5 % hold one inside the first line, 5 %
hold none.  With --perl SCRIPT the same file goes through `perl SCRIPT -s -b -d` (no GPU needed for that part: --no-gpu).

usage: python3 tools/probe_barcode.py [--reads N] [--barcodes B] [--dir DIR] [--perl Barcode/barcode.pl] [--no-gpu]
Prints one JSON line; verb_md5 and perl_md5 are digests of the two output directories (equal: byte-identical files).
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
READ, WIDTH = 250, 60


def write_inputs(d, n_reads, n_bars, seed=20261019):
    rng = np.random.RandomState(seed)
    bars = set()
    while len(bars) < n_bars:
        bars.add(bytes(ACGT[rng.randint(0, 4, 8)]))
    bars = sorted(bars)
    with open(os.path.join(d, "barcodes.txt"), "wb") as f:
        f.write(b"".join(b"s%02d\t%s\n" % (i, b) for i, b in enumerate(bars)))
    bar_arr = np.frombuffer(b"".join(bars), dtype=np.uint8).reshape(n_bars, 8)
    n_lines = (READ + WIDTH - 1) // WIDTH
    rec = 10 + READ + n_lines  # ">r0000000\n", the letters, a line end per line
    cols = np.concatenate([10 + k * (WIDTH + 1) + np.arange(min(WIDTH, READ - k * WIDTH)) for k in range(n_lines)])
    with open(os.path.join(d, "reads.fas"), "wb") as f:
        for first in range(0, n_reads, 200000):
            n = min(200000, n_reads - first)
            out = np.full((n, rec), ord("\n"), dtype=np.uint8)
            out[:, 0] = ord(">")
            out[:, 1] = ord("r")
            num = first + np.arange(n)
            for k in range(7):
                out[:, 8 - k] = ord("0") + (num // 10 ** k) % 10
            seq = ACGT[rng.randint(0, 4, (n, READ))]
            kind = rng.rand(n)
            which = bar_arr[rng.randint(0, n_bars, n)]
            off = np.where(kind < 0.90, 0, rng.randint(1, WIDTH - 8, n))
            planted = np.nonzero(kind < 0.95)[0]
            for k in range(8):
                seq[planted, off[planted] + k] = which[planted, k]
            out[:, cols] = seq
            f.write(out.tobytes())
        f.write(b">tail\nNNNN\n")  # (the script never ends on some last records: this one is safe)
    return os.path.getsize(os.path.join(d, "reads.fas"))


def digest(d):
    """one MD5 over the names and bytes of every file in `d`, in name order: equal digests, equal output directories"""
    h = hashlib.md5()
    for name in sorted(os.listdir(d)):
        h.update(name.encode() + b"\0")
        with open(os.path.join(d, name), "rb") as f:
            for piece in iter(lambda: f.read(1 << 24), b""):
                h.update(piece)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--barcodes", type=int, default=96)
    ap.add_argument("--dir", default=None, help="where the inputs and outputs go (default: a temporary directory)")
    ap.add_argument("--perl", default=None, help="path of the reference's Barcode/barcode.pl: time it on the same file")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="pgx_probe_barcode_")
    os.makedirs(d, exist_ok=True)
    res = {"reads": a.reads, "read_len": READ, "barcodes": a.barcodes, "bytes": write_inputs(d, a.reads, a.barcodes)}
    std = ["-s", "reads.fas", "-b", "barcodes.txt", "-d", "out"]

    def fresh_out():
        shutil.rmtree(os.path.join(d, "out"), ignore_errors=True)
        os.makedirs(os.path.join(d, "out"))

    if not a.no_gpu:
        import pangea_plus_amd as pg
        pg.init(0)
        verb = []
        for _ in range(2):
            fresh_out()
            t = time.perf_counter()
            log = pg.barcode(std, cwd=d)
            verb.append(time.perf_counter() - t)
        res["verb_s"] = [round(x, 3) for x in verb]
        res["verb_reads_per_s"] = round(a.reads / min(verb))
        res["verb_log"] = log.decode().split("\n")[3:7]
        res["verb_md5"] = digest(os.path.join(d, "out"))
        resident = []
        for _ in range(2):
            t = time.perf_counter()
            r = pg.barcode_reads(os.path.join(d, "reads.fas"), os.path.join(d, "barcodes.txt"))
            t_run = time.perf_counter() - t
            batches = [r.take_reads(i) for i in range(len(r))]
            resident.append((t_run, time.perf_counter() - t))
            n_batched = sum(len(b) for b in batches)
            for b in batches:
                b.close()
            r.close()
        res["resident_s"] = [round(x[0], 3) for x in resident]
        res["resident_with_batches_s"] = [round(x[1], 3) for x in resident]
        res["resident_reads_per_s"] = round(a.reads / min(x[0] for x in resident))
        res["resident_with_batches_reads_per_s"] = round(a.reads / min(x[1] for x in resident))
        res["reads_in_batches"] = n_batched
    if a.perl:
        fresh_out()
        t = time.perf_counter()
        p = subprocess.run(["perl", a.perl] + std, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        res["perl_s"] = round(time.perf_counter() - t, 3)
        res["perl_reads_per_s"] = round(a.reads / res["perl_s"])
        res["perl_log"] = p.stdout.decode().split("\n")[3:7]
        res["perl_md5"] = digest(os.path.join(d, "out"))
    if not a.dir:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
