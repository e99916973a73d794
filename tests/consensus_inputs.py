"""Seeded inputs that drive every form of the device consensus (tests/consensus_rule.py labels them).

One database of families of near-identical subjects, one read set (windows of a family member on both strands), and
three taxonomies over the same subjects with an RDP file each:
  T1  seven one-word ranks, some lineages shorter; every RDP line holds <= 6 triplets (32-byte records, 7x6 grid);
  T2  T1's lineages; some RDP lines hold 7-8 triplets (15x8 grid), some 9-20 and a few about 100 repeated triplets
      (the general count, agreement counts of two and three digits);
  T3  names of 2-5 words (digits, dots, `sp.`), lineages of 8-15 pairs (64-byte records) and some of more than 15
      (the escape to the general count); some gi numbers have no taxon (`Unidentified(GI:n)`).
Each read has one row per family member (500 at most): the source subject on top at 100.00, the others at 9x.xx,
so that the text order `"100.00" lt "9x.xx"` decides between tied rows in nearly every read.
"""
import os
import random
import subprocess

from consensus_rule import RDP_RANKS, lineage_tokens
from tax_inputs import write_dumps

SIZES = [1, 2, 31, 32, 33, 34, 63, 64, 65, 66, 130, 600]
SUBJ_LEN, READ_LEN = 300, 150
READS_U, READS_M = 12, 36           # reads of a family of one lineage depth / of mixed depths
EXTRA_WORDS = ["sp.", "3", "7A", "K-12", "Candidatus", "alpha", "Beta", "str.", "group", "bacterium", "uncultured", "X1"]
COMP = str.maketrans("ACGT", "TGCA")


def _code(f):
    return chr(97 + f // 26) + chr(97 + f % 26)


def _families():
    """(family number, size, mixed) for every family: one of a single lineage depth and one of mixed depths per size."""
    out = []
    for s in SIZES:
        out.append((len(out), s, False))
        out.append((len(out), s, True))
    return out


def database(rng):
    """Subjects [(gi, family, member, sequence)]: every member carries substitutions in four slots 75 bases apart, so
    that every 150-base window of a member differs from every other member of its family."""
    subj = []
    for f, size, _ in _families():
        anc = [rng.choice("ACGT") for _ in range(SUBJ_LEN)]
        for j in range(size):
            s = list(anc)
            for k in range(4):
                for _ in range(1 + (j + k) % 2):
                    p = 37 + 75 * k + rng.randint(-30, 30)
                    s[p] = rng.choice([c for c in "ACGT" if c != anc[p]])
            subj.append((1000 + len(subj), f, j, "".join(s)))
    return subj


def taxa_of(f, mixed, j):
    """The taxon (by role) family member j belongs to: s1, s2 in genus G; s3 in genus H; s4 in genus K whose lineage
    has no family; u, an unranked leaf under G (its lineage ends at the genus); s5 in genus Q right below the
    superkingdom (6 tokens: a one-digit token count against the others' two)."""
    if not mixed:
        return ["s1", "s3", "s2"][j] if j < 3 else ["s1", "s2", "s3"][(j * 7 + f) % 3]
    return ["s1", "s4", "u", "s3", "s5"][j] if j < 5 else ["s1", "s2", "s3", "s4", "u", "s5"][(j * 5 + f) % 6]


def taxonomy(subj, multiword, rng):
    """nodes / names / gi list of one taxonomy over the database's subjects (ids per family: 100 * f + role)."""
    nodes = [(1, 1, "no rank", ""), (2, 1, "superkingdom", ""), (3, 1, "superkingdom", "")]
    names = {1: [("root", "", "scientific name")], 2: [("Bacteria", "", "scientific name")],
             3: [("Archaea", "", "scientific name")]}

    def nm(core, long_=False):
        if not multiword:
            return core
        w = [core] + [rng.choice(EXTRA_WORDS) for _ in range(4 if long_ else rng.randint(1, 2))]
        rng.shuffle(w)
        return " ".join(w)

    role_id = {}
    for f, size, mixed in _families():
        c = _code(f)
        b = 1000 + 100 * f
        ids = dict(ph=b + 1, cl=b + 2, od=b + 3, fa=b + 4, G=b + 5, H=b + 6, nr=b + 7, K=b + 8, s1=b + 11, s2=b + 12,
                   s3=b + 13, s4=b + 14, u=b + 15, fa2=b + 16, kg=b + 17, nq=b + 18, Q=b + 19, s5=b + 20)
        role_id[f] = ids
        long_ = multiword and mixed and f % 4 == 1
        spec = [(ids["ph"], 2 + f % 2, "phylum", nm("Phy" + c)), (ids["cl"], ids["ph"], "class", nm("Cls" + c)),
                (ids["od"], ids["cl"], "order", nm("Ord" + c)), (ids["fa"], ids["od"], "family", nm("Fam" + c)),
                (ids["G"], ids["fa"], "genus", nm("Gen" + c)), (ids["nr"], ids["od"], "no rank", "Nr" + c),
                (ids["K"], ids["nr"], "genus", nm("Kgen" + c)), (ids["s1"], ids["G"], "species", "Gen%s alpha" % c),
                (ids["s2"], ids["G"], "species", "Gen%s beta" % c), (ids["s4"], ids["K"], "species", "Kgen%s gamma" % c),
                (ids["u"], ids["G"], "no rank", "Gen%s sp. X1" % c), (ids["nq"], 2 + f % 2, "no rank", "Nq" + c),
                (ids["Q"], ids["nq"], "genus", nm("Qgen" + c)), (ids["s5"], ids["Q"], "species", "Qgen%s eta" % c)]
        if long_:
            # the widest lineages: H below a kingdom and a family of five-word names (more than 15 pairs)
            spec += [(ids["kg"], ids["od"], "kingdom", nm("King" + c, True)), (ids["fa2"], ids["kg"], "family", nm("Fam" + c, True)),
                     (ids["H"], ids["fa2"], "genus", nm("Hgen" + c, True))]
        else:
            spec += [(ids["H"], ids["fa"], "genus", nm("Hgen" + c))]
        spec += [(ids["s3"], ids["H"], "species", "Hgen%s delta" % c)]
        for t, p, r, n in spec:
            nodes.append((t, p, r, ""))
            names[t] = [(n, "", "scientific name")]
    gis = []
    for gi, f, j, _ in subj:
        mixed = _families()[f][2]
        if multiword and mixed and j % 7 == 3:
            gis.append((gi, 0))                 # no taxon: Unidentified(GI:n)
        else:
            gis.append((gi, role_id[f][taxa_of(f, mixed, j)]))
    return nodes, names, gis


def reads(subj, rng):
    """[(name, family, source member, sequence, mode)]: a window of the source on either strand.  mode: "same" (the RDP
    line names the source's lineage), "other" (a member of another genus), "none" (names that agree with nothing)."""
    by_fam = {}
    for gi, f, j, s in subj:
        by_fam.setdefault(f, []).append(s)
    out = []
    for f, size, mixed in _families():
        mem = by_fam[f]
        for k in range(READS_M if mixed else READS_U):
            while True:
                j = rng.randrange(size)
                st = rng.randint(0, SUBJ_LEN - READ_LEN)
                w = mem[j][st:st + READ_LEN]
                if all(m[st:st + READ_LEN] != w for i, m in enumerate(mem) if i != j):
                    break
            seq = w if rng.random() < 0.5 else w.translate(COMP)[::-1]
            mode = ["same", "other", "none"][k % 3] if mixed else ("none" if k % 6 == 5 else "same")
            out.append(("r%d" % len(out), f, j, seq, mode))
    return out


def _trip(name, rank, conf="1.0", quote=False):
    return ('"%s"' % name if quote else name) + "\t" + rank + "\t" + conf


def rdp_line(tax, lineage, mode, k, rng):
    """The five-tab RDP record of one read from a lineage text (consensus_rule.lineage_tokens' pairs)."""
    toks = [t.decode() for t in lineage_tokens(lineage.encode())]
    pairs = [(toks[a], toks[a + 1] if a + 1 < len(toks) else "") for a in range(0, len(toks), 2)]
    trips = []
    for r, n in pairs:
        if not n.isalpha():
            continue
        if r in "012345" and len(r) == 1:
            trips.append((n, RDP_RANKS[int(r)].decode()))
        elif tax == "T3" and r not in ("6",):
            trips.append((n, "subgenus"))       # a name token in a rank slot: undef against undef
    if mode == "none":
        trips = [("Zzz" + n[::-1], r) for n, r in trips]
    trips = trips[:5 if k % 4 == 3 else 6]
    cells = [_trip(n, r, "%.2f" % rng.uniform(0.5, 1.0), quote=(k + i) % 3 == 0) for i, (n, r) in enumerate(trips)]
    if tax == "T2" and mode != "none" and trips:
        genus = [c for c, (n, r) in zip(cells, trips) if r == "genus"] or cells[-1:]
        if k % 5 == 1:      # 7-8 triplets
            cells += [_trip("Zzzspecies", "species")] + ([_trip("Nothing", "norank")] if k % 2 else [])
        elif k % 5 == 2:    # 9-20 triplets: the genus repeated
            cells += genus * rng.randint(3, 14)
        elif k % 17 == 3:   # about a hundred
            cells += genus * rng.randint(93, 99)
    if k % 4 == 3:
        cells.append(_trip("12", "norank", "0.5", quote=True))      # a name that cleans to "" by an unranked rank
    return "\t".join(cells)


def subject_table(subj):
    return "".join("s%d\tgi|%d|f%d|m%d|\t100.00\t300\t0\t0\t1\t300\t1\t300\t1e-150\t 555\n" % (i, gi, f, j)
                   for i, (gi, f, j, _) in enumerate(subj))


def run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, **kw)
    assert p.returncode == 0, (cmd, p.stderr[-2000:])
    return p.stdout


def build(d, oracle_bin, seed=20261015):
    """Write the database, reads, taxonomies and RDP files under `d`, and run the oracle chain: one blastn, then
    taxcollector + consensus per taxonomy.  Returns {name: path} plus "lineages": {tax: [lineage of every subject]}."""
    d = str(d)
    rng = random.Random(seed)
    subj = database(rng)
    rd = reads(subj, rng)
    p = {"db": os.path.join(d, "db.fa"), "reads": os.path.join(d, "reads.fa"), "lineages": {}, "n_reads": len(rd),
         "n_subjects": len(subj)}
    with open(p["db"], "w") as f:
        f.write("".join(">gi|%d|f%d|m%d|\n%s\n" % (gi, fa, j, s) for gi, fa, j, s in subj))
    with open(p["reads"], "w") as f:
        f.write("".join(">%s\n%s\n" % (n, s) for n, _, _, s, _ in rd))
    with open(os.path.join(d, "subjects.tsv"), "w") as f:
        f.write(subject_table(subj))
    p["hits"] = os.path.join(d, "hits.tsv")
    run([oracle_bin, "blastn", "-query", p["reads"], "-db", p["db"], "-outfmt", "6", "-out", p["hits"], "-num_threads", "8"])
    by_fam = {}
    for i, (gi, f, j, _) in enumerate(subj):
        by_fam.setdefault(f, []).append(i)
    for tax in ("T1", "T2", "T3"):
        trng = random.Random(seed + int(tax[1]))
        td = os.path.join(d, tax)
        os.makedirs(td, exist_ok=True)
        src = "T1" if tax == "T2" else tax
        if tax != "T2":
            write_dumps(td, *taxonomy(subj, tax == "T3", trng))
        else:
            for n in ("nodes.dmp", "names.dmp", "gi_taxid_nucl.dmp"):
                with open(os.path.join(d, src, n), "rb") as a, open(os.path.join(td, n), "wb") as b:
                    b.write(a.read())
        run([oracle_bin, "tax_class", "-c"], cwd=td)
        run([oracle_bin, "taxcollector", "-f", os.path.join(d, "subjects.tsv"), "-o", os.path.join(td, "subjects_class.tsv"),
             "-d", td])
        with open(os.path.join(td, "subjects_class.tsv")) as f:
            lin = [l.split("\t")[1] for l in f.read().splitlines()]
        assert len(lin) == len(subj)
        p["lineages"][tax] = lin
        lines = ["zz_other_%d\t\t\t\t\tBacteria\tdomain\t1.0" % k for k in range(3)]    # reads not in the batch
        for k, (name, f, j, _, mode) in enumerate(rd):
            if k % 23 == 11:
                continue                                                            # a read without a line
            mem = by_fam[f]
            target = mem[j]
            if mode == "other":
                role = taxa_of(f, True, j)
                genus = {"s1": "G", "s2": "G", "u": "G", "s3": "H", "s4": "K", "s5": "Q"}
                others = [i for i in mem if genus.get(taxa_of(f, True, subj[i][2])) != genus.get(role)
                          and lin[i].startswith("[")]
                target = others[k % len(others)] if others else target
            lines.append(name + "\t\t\t\t\t" + rdp_line(tax, lin[target], mode, k, trng))
        p["rdp_" + tax] = os.path.join(td, "rdp.tsv")
        with open(p["rdp_" + tax], "w") as f:
            f.write("\n".join(lines) + "\n")
        p["class_" + tax] = os.path.join(td, "hits_class.tsv")
        p["cons_" + tax] = os.path.join(td, "consensus.txt")
        run([oracle_bin, "taxcollector", "-f", p["hits"], "-o", p["class_" + tax], "-d", td])
        run([oracle_bin, "consensus", "-b", p["class_" + tax], "-r", p["rdp_" + tax], "-o", p["cons_" + tax]])
        p["tax_" + tax] = td
    return p


def labelled(p, tax, v=None):
    """The restatement on taxonomy `tax` of a build(): (output, log, records with the device labels)."""
    import consensus_rule as cr
    with open(p["class_" + tax], "rb") as f:
        blast = f.read()
    with open(p["rdp_" + tax], "rb") as f:
        rdp = f.read()
    out, log, recs = cr.consensus(blast, rdp, v=v or cr.PERL)
    db_pairs = cr.max_pairs(len(lineage_tokens(x.encode())) for x in p["lineages"][tax])
    nr_max = min(8, max(r.ntrip for r in recs))     # every read with a line prints a record here
    return out, log, cr.label(recs, db_pairs, nr_max), db_pairs, nr_max
