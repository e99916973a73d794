"""Seed-mode golden vectors for `soap -l L -v V` (soap.man:59-72), single-end, produced by the reference's closed
`2bwt-builder` / `soap` ELFs (Classify/Runsoap/soap2.21release) against tests/golden/soap/ref.fa.

Runs on a machine that holds the reference tree only; no test imports it.  Outputs (tests/golden/soap_seed/, gzipped):
  reads.fa (the golden reads of tests/golden/soap) at -l 32 -v 5, -l 64, -l 32 -v 2, -l 32 -v 20 (each -r 2), -l 32 -v 5
  at -r 0 and -r 1, -l 32 at -M 0 / 1 / 2, -l 32 -v 5 -t, -g 3 / -s 40 (no -l: the rows of a plain run);
  sweep.fa: reads of 27-600 bases, both strands, mismatches planted at swept offsets inside and outside a 32-base seed
  (-l 32 -v 5 -r 2) and a 64-base seed (-l 64 -v 3 -r 2);
  long.fa: reads of 257-600 bases with 0-6 planted mismatches, at the defaults and at -l 256 -v 5 (-r 2).
Every run's -u file is kept.
usage: python3 tools/gen_goldens_soap_seed.py [reference root]
"""
import gzip
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "..", "tests", "golden")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

# name -> (reads file, options)
RUNS = {
    "l32v5": ("reads.fa", "-l 32 -v 5 -r 2"),
    "l64": ("reads.fa", "-l 64 -r 2"),
    "l32v2": ("reads.fa", "-l 32 -v 2 -r 2"),
    "l32v20": ("reads.fa", "-l 32 -v 20 -r 2"),
    "l32v5_r0": ("reads.fa", "-l 32 -v 5 -r 0"),
    "l32v5_r1": ("reads.fa", "-l 32 -v 5 -r 1"),
    "l32_M0": ("reads.fa", "-l 32 -M 0 -r 2"),
    "l32_M1": ("reads.fa", "-l 32 -M 1 -r 2"),
    "l32_M2": ("reads.fa", "-l 32 -M 2 -r 2"),
    "l32v5_t": ("reads.fa", "-l 32 -v 5 -r 2 -t"),
    "g3": ("reads.fa", "-g 3 -r 2"),
    "s40": ("reads.fa", "-s 40 -r 2"),
    "sweep_l32v5": ("sweep.fa", "-l 32 -v 5 -r 2"),
    "sweep_l64v3": ("sweep.fa", "-l 64 -v 3 -r 2"),
    "long_default": ("long.fa", "-r 2"),
    "long_l256v5": ("long.fa", "-l 256 -v 5 -r 2"),
}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def read_fasta(p):
    seqs, name, buf = [], None, []
    for line in open(p):
        line = line.rstrip("\n")
        if line.startswith(">"):
            if name is not None:
                seqs.append((name, "".join(buf)))
            name, buf = line[1:], []
        else:
            buf.append(line)
    seqs.append((name, "".join(buf)))
    return seqs


def synth(ref_fa):
    rng = random.Random(20261015)
    seqs = [(n.split()[0], "".join(c if c in "ACGT" else "G" for c in s.upper())) for n, s in read_fasta(ref_fa)]

    def cut(L):
        while True:
            n, s = rng.choice(seqs)
            if len(s) >= L + 2:
                o = rng.randrange(0, len(s) - L)
                return n, o, s[o:o + L]

    def planted(s, offs):
        x = list(s)
        for p in offs:
            x[p] = rng.choice([c for c in "ACGT" if c != x[p]])
        return "".join(x)

    sweep = []
    for L in (27, 31, 32, 33, 40, 48, 64, 65, 100, 150, 200, 256, 300, 400, 600):
        for rep in range(14):
            n, o, w = cut(L)
            strand = rep & 1
            seed = min(32, L)
            a = L - seed if strand else 0          # where a 32-base seed lies on the reference-oriented read
            k_in = rng.choice([0, 1, 1, 2, 2, 3])
            k_out = rng.choice([0, 1, 2, 3, 4, 5, 6, 8])
            ins = rng.sample(range(a, a + seed), min(k_in, seed))
            outside = [p for p in range(L) if not a <= p < a + seed]
            outs = rng.sample(outside, min(k_out, len(outside)))
            m = planted(w, ins + outs)
            sweep.append((f"sw{len(sweep)}_{n}_{o + 1}_{'-+'[strand == 0]}_L{L}_in{k_in}_out{k_out}", rc(m) if strand else m))
    for strand in (0, 1):          # one mismatch at every offset of a 32-base seed, two more outside it
        n, o, w = cut(150)
        for p in range(32):
            q = p + 118 if strand else p
            m = planted(w, [q, 60, 80])
            sweep.append((f"off{p}_{'+-'[strand]}_{n}_{o + 1}", rc(m) if strand else m))
    long_ = []
    for rep in range(60):
        L = rng.choice([257, 260, 300, 350, 400, 450, 500, 600])
        n, o, w = cut(L)
        strand = rep & 1
        k = rng.choice([0, 1, 2, 3, 4, 5, 6])
        head = rng.choice([0, 1, 2])                 # how many fall into the first 256 bases of the read
        a = L - 256 if strand else 0
        ins = rng.sample(range(a, a + 256), min(head, k))
        outs = rng.sample([p for p in range(L) if not a <= p < a + 256], min(k - len(ins), L - 256))
        m = planted(w, ins + outs)
        long_.append((f"lg{rep}_{n}_{o + 1}_{'+-'[strand]}_L{L}_k{k}", rc(m) if strand else m))
    return sweep, long_


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    soap_dir = os.path.join(root, "Classify", "Runsoap", "soap2.21release")
    builder, soap = os.path.join(soap_dir, "2bwt-builder"), os.path.join(soap_dir, "soap")
    if not (os.access(builder, os.X_OK) and os.access(soap, os.X_OK)):
        sys.exit("gen_goldens_soap_seed: the reference's soap / 2bwt-builder are not at %s" % soap_dir)
    src = os.path.join(GOLD, "soap")
    out = os.path.join(GOLD, "soap_seed")
    os.makedirs(out, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="pgx_soap_seed_") as work:
        shutil.copy(os.path.join(src, "ref.fa"), os.path.join(work, "ref.fa"))
        shutil.copy(os.path.join(src, "reads.fa"), os.path.join(work, "reads.fa"))
        sweep, long_ = synth(os.path.join(work, "ref.fa"))
        for name, reads in (("sweep.fa", sweep), ("long.fa", long_)):
            with open(os.path.join(work, name), "w") as f:
                for n, s in reads:
                    f.write(f">{n}\n{s}\n")
            shutil.copy(os.path.join(work, name), os.path.join(out, name))
        subprocess.run([builder, "ref.fa"], cwd=work, check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for tag, (reads, opts) in RUNS.items():
            subprocess.run([soap, "-a", reads, "-D", "ref.fa.index", "-o", f"out_{tag}.txt", "-u", f"unmapped_{tag}.txt", "-p", "1",
                            "-M", "4"] + opts.split(), cwd=work, check=True, timeout=600, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
            for n in (f"out_{tag}.txt", f"unmapped_{tag}.txt"):
                with open(os.path.join(work, n), "rb") as a, gzip.GzipFile(os.path.join(out, n + ".gz"), "wb", mtime=0) as b:
                    shutil.copyfileobj(a, b)
            print("%-14s %-26s %5d rows" % (tag, opts, sum(1 for _ in open(os.path.join(work, f"out_{tag}.txt")))))


if __name__ == "__main__":
    main()
