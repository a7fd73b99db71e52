#!/usr/bin/env python3
"""The repeat-family fixture: a small genome of repeat families and read pairs SELECTED to sit on the thresholds of the chaining and
pairing kernels' wave-cooperative forms, with the SAM of the UNMODIFIED reference mapper (oracle/_ref/kart -t 1) for them.

TEST INFRASTRUCTURE; runs only where /root/reference exists (oracle/_ref is built from it).  Everything is seeded, and the gz members
carry no time stamp: a second run writes the same bytes.

  tests/golden/rep.fa.gz            contig "fam": families of 800 bp in 5, 6, 34 and 45 copies (0.1-0.4 % divergence from the consensus per copy: a
                                    read's seeds then reach most copies, n1 x n2 comes close to the square of the copy count), 80 copies (1-2.2 %)
                                    and 100 copies (3-4 %), between 200-300 random bases, the copies of all families shuffled, a third of them
                                    reverse-complemented; contig "uniq": 6 kb unique; the 2 kb "decoy"
  tests/golden/sam/rep_{1,2}.fq.gz  at most 2000 pairs (ONE 4000-read chunk: every pair is mapped under EstDistance = MaxInsertSize = 1500)
  tests/golden/sam/rep.sam.gz       kart -t 1
  tests/golden/sam/rep_m.sam.gz     kart -t 1 -m, and rep_m.never_assigned_flags.txt: the lines whose FLAG differs between two runs under
                                    different MALLOC_PERTURB_ fills

The pairs are drawn three ways -- at random over the genome, from inside single copies of a chosen family (both mates in the family, which
random sampling almost never gives), and the same with one mate carrying 5-20 % errors -- then seeded and chained by the CPU oracle, mapped
by the reference in slices of 2000 pairs (a pair's records depend on the pair and EstDistance alone), and selected by class; the classes are
asserted from the committed files by tests/test_rep_cpu.py.

    python oracle/make_golden_rep.py
"""
import gzip
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kart_amd import index_build, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402
import rep_fixture as F  # noqa: E402
from ref_flags import reference_sam_and_never_assigned_flags  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "sam")
KART = os.path.join(ROOT, "oracle", "_ref", "kart")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
FAM_LEN = 800
FAMILIES = [(5, 0.001, 0.004), (6, 0.001, 0.004), (34, 0.001, 0.004), (45, 0.001, 0.004), (80, 0.01, 0.022), (100, 0.03, 0.04)]      # (copies, divergence from .. to)
SPACER = (200, 300)
FLANK, UNIQ = 1000, 6000
READ_LEN = 150


def gz_write(path, data):
    """gzip without a time stamp or a name in the member: the same bytes every run"""
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, compresslevel=9, mtime=0) as fh:
        fh.write(data)
    open(path, "wb").write(buf.getvalue())


def make_genome(seed=20):
    """returns ({name: ASCII array}, [(family, start on "fam")] of every copy)"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: ACGT[rng.integers(0, 4, size=n)]
    consensus = [rnd(FAM_LEN) for _ in FAMILIES]
    copies = [f for f, (n, _, _) in enumerate(FAMILIES) for _ in range(n)]
    rng.shuffle(copies)
    parts, where, at = [rnd(FLANK)], [], FLANK
    for f in copies:
        c = consensus[f].copy()
        div = rng.uniform(FAMILIES[f][1], FAMILIES[f][2])
        hit = rng.random(FAM_LEN) < div
        c[hit] = ACGT[(np.searchsorted(ACGT, c[hit]) + rng.integers(1, 4, size=int(hit.sum()))) & 3]
        if rng.random() < 1 / 3:
            c = synth.revcomp(c)
        where.append((f, at))
        spacer = rnd(int(rng.integers(SPACER[0], SPACER[1] + 1)))
        parts += [c, spacer]
        at += FAM_LEN + len(spacer)
    parts.append(rnd(FLANK))
    return {"fam": np.concatenate(parts), "uniq": rnd(UNIQ), "decoy": rnd(2000)}, where


def add_errors(arr, rng, err):
    e = rng.random(arr.shape) < err
    arr[e] = ACGT[(np.searchsorted(ACGT, arr[e]) + rng.integers(1, 4, size=int(e.sum()))) & 3]
    return arr


def family_pairs(genome, where, fam, n, seed, noisy=False):
    """n pairs whose fragment lies inside one copy of family `fam` (up to 60 bases over its ends); noisy: one mate -- mate 1 in three pairs
    of four, so that the rescue windows are mate 1's (the other direction is the host's) -- carries 5-20 % substitutions instead of 1 %"""
    rng = np.random.default_rng(seed)
    g = genome["fam"]
    starts = [s for f, s in where if f == fam]
    names, r1, r2 = [], np.empty((n, READ_LEN), np.uint8), np.empty((n, READ_LEN), np.uint8)
    for i in range(n):
        s = starts[int(rng.integers(len(starts)))]
        frag = int(np.clip(round(rng.normal(500, 50)), READ_LEN, FAM_LEN))
        p0 = s + int(rng.integers(-60, FAM_LEN - frag + 61))
        left, right = g[p0:p0 + READ_LEN].copy(), synth.revcomp(g[p0 + frag - READ_LEN:p0 + frag])
        a, b = (right, left) if rng.random() < 0.5 else (left, right)
        e1 = e2 = 0.01
        if noisy:
            if rng.random() < 0.75:
                e1 = rng.uniform(0.05, 0.2)
            else:
                e2 = rng.uniform(0.05, 0.2)
        r1[i], r2[i] = add_errors(a, rng, e1), add_errors(b, rng, e2)
        names.append("%s%d_%d:Pos=%d" % ("n" if noisy else "f", fam, i, p0))
    return names, r1, r2


def write_pairs(tmp, tag, names, r1, r2):
    f1, f2 = os.path.join(tmp, tag + "_1.fq"), os.path.join(tmp, tag + "_2.fq")
    synth.write_fastq(f1, names, r1, mate=1)
    synth.write_fastq(f2, names, r2, mate=2)
    return f1, f2


def ref_run(prefix, f1, f2, extra, out):
    subprocess.run([KART, "-silent", "-t", "1", "-i", prefix, "-f", f1, "-f2", f2] + extra + ["-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out, "rb").read()


def main():
    assert os.path.exists(KART), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(OUT, exist_ok=True)
    genome, where = make_genome()
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "rep.fa")
        synth.write_fasta(fa, genome)
        gz_write(os.path.join(GOLD, "rep.fa.gz"), open(fa, "rb").read())
        prefix = os.path.join(tmp, "rep")
        index_build.build_index(fa, prefix, device="cpu")
        print("genome: %d bases, %d copies" % (sum(len(v) for v in genome.values()), len(where)))

        # ---- the pool ------------------------------------------------------------------------------------------------------------
        names, r1, r2 = synth.simulate_pairs(genome, 6000, seed=3, err=0.01, mut=0.002, indel_frac=0.3)
        pools = [(list(names), r1, r2)]
        for fam, (n_plain, n_noisy) in enumerate([(300, 200), (300, 200), (1500, 700), (2500, 900), (3000, 700), (1500, 300)]):
            pools.append(family_pairs(genome, where, fam, n_plain, seed=100 + fam))
            pools.append(family_pairs(genome, where, fam, n_noisy, seed=200 + fam, noisy=True))
        names = [n for p in pools for n in p[0]]
        r1, r2 = np.concatenate([p[1] for p in pools]), np.concatenate([p[2] for p in pools])
        n_pool, n_random = len(names), 6000
        held = F.held_reads([x.tobytes() for x in r1], [x.tobytes() for x in r2])
        orc = O.Oracle(prefix)
        so, _, cands = F.oracle_chain(orc, held)
        orc.close()
        n_seeds = np.diff(so)
        nc = np.array([len(c) for c in cands])
        prod = nc[0::2] * nc[1::2]
        pairing = np.array([F.chained_lists_pair(cands[2 * q], cands[2 * q + 1]) for q in range(n_pool)])
        print("pool: %d pairs; largest seed count %d, candidate count %d, product %d" % (n_pool, n_seeds.max(), nc.max(), prod.max()))

        # ---- the reference on the pool, 2000 pairs at a time: which pairs come out as proper pairs, how many records -m prints ----------------
        proper, multi = np.zeros(n_pool, bool), np.zeros(n_pool, int)
        for a in range(0, n_pool, 2000):
            b = min(n_pool, a + 2000)
            f1, f2 = write_pairs(tmp, "slice", names[a:b], r1[a:b], r2[a:b])
            recs = F.sam_records(ref_run(prefix, f1, f2, [], os.path.join(tmp, "s.sam")))
            lines, never = reference_sam_and_never_assigned_flags(KART, ["-i", prefix, "-f", f1, "-f2", f2, "-m"], tmp)
            recs_m = F.sam_records(b"\n".join(lines), never)
            for q in range(a, b):
                nm = names[q].encode()
                x, y = recs.get((nm, 0), []), recs.get((nm, 1), [])
                proper[q] = len(x) == 1 and len(y) == 1 and (int(x[0][1][1]) & 2) != 0 and (int(y[0][1][1]) & 2) != 0
                multi[q] = max(len(recs_m.get((nm, 0), [])), len(recs_m.get((nm, 1), [])))

        # ---- the selection -----------------------------------------------------------------------------------------------------------
        rng = np.random.default_rng(7)
        chosen = []

        def take(mask, k, what):
            idx = np.flatnonzero(mask)
            idx = idx[~np.isin(idx, chosen)]
            pick = rng.permutation(idx)[:k]
            chosen.extend(int(x) for x in pick)
            print("  %-58s %5d in the pool, %4d taken" % (what, int(mask.sum()), len(pick)))

        s1, s2 = n_seeds[0::2], n_seeds[1::2]
        heavy = prod > 32
        rescued = ~pairing & proper                       # the chained lists pair nothing, the reference's records are a proper pair
        mate1_side = np.array([max([c[0] for c in cands[2 * q + 1]], default=0) - max([c[0] for c in cands[2 * q]], default=0) > 50 for q in range(n_pool)])
        for k in (16, 17, 64, 65):
            take(((s1 == k) | (s2 == k)) & pairing, 6, "a read of exactly %d seeds" % k)
        take((prod >= 25) & (prod <= 32) & pairing, 10, "product 25..32")
        take((prod >= 33) & (prod <= 40) & pairing, 10, "product 33..40")
        take((prod >= 900) & (prod <= 1000) & pairing, 12, "product 900..1000")
        take((prod >= 1001) & (prod <= 4096) & pairing, 60, "product 1001..4096")
        take((prod > 4096), 10, "product above 4096")
        take((nc[1::2] > 64) & (prod <= 4096), 6, "mate 2 with more than 64 candidates")
        take((nc[0::2] > 64) & (prod <= 4096), 4, "mate 1 with more than 64 candidates")
        take(heavy & (prod <= 1000) & pairing, 200, "product 33..1000, paired by the chained lists")
        take(heavy & rescued & mate1_side, 40, "heavy, rescued, windows of mate 1")
        take(heavy & rescued & ~mate1_side, 12, "heavy, rescued, other strategies")
        take(heavy & (multi > 1), 40, "heavy, more than one record per read with -m")
        take(~heavy & rescued, 80, "light, rescued")
        take(~heavy & ~pairing & ~proper, 20, "light, not paired at all")
        take(np.arange(n_pool) < n_random, 300, "ordinary")
        chosen = rng.permutation(np.array(sorted(set(chosen))))
        assert len(chosen) <= 2000
        sel_names = [names[q] for q in chosen]
        f1, f2 = write_pairs(tmp, "rep", sel_names, r1[chosen], r2[chosen])
        sam = ref_run(prefix, f1, f2, [], os.path.join(tmp, "rep.sam"))
        assert sam == ref_run(prefix, f1, f2, [], os.path.join(tmp, "rep_again.sam"))
        lines, never = reference_sam_and_never_assigned_flags(KART, ["-i", prefix, "-f", f1, "-f2", f2, "-m"], tmp)
        gz_write(os.path.join(OUT, "rep_1.fq.gz"), open(f1, "rb").read())
        gz_write(os.path.join(OUT, "rep_2.fq.gz"), open(f2, "rb").read())
        gz_write(os.path.join(OUT, "rep.sam.gz"), sam)
        gz_write(os.path.join(OUT, "rep_m.sam.gz"), b"\n".join(lines))
        open(os.path.join(OUT, "rep_m.never_assigned_flags.txt"), "w").write("".join("%d\n" % i for i in sorted(never)))
        print("%d pairs; rep.sam %d lines, rep_m.sam %d lines, %d of them with a FLAG the reference never assigns" % (len(chosen), sam.count(b"\n"), len(lines) - 1, len(never)))
        for f in ("rep.fa.gz", "sam/rep_1.fq.gz", "sam/rep_2.fq.gz", "sam/rep.sam.gz", "sam/rep_m.sam.gz"):
            print("  %-22s %7d bytes" % (f, os.path.getsize(os.path.join(GOLD, f))))


if __name__ == "__main__":
    main()
