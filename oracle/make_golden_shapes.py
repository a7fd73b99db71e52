#!/usr/bin/env python3
"""The indel-shape fixture: reads with CONSTRUCTED edits, selected by the shape of the alignments the candidate report makes of them -- the
tile geometry of the finish pass (align_finish.hip works on tiles of 8 columns), the decision thresholds in front of it (align_plan.hip) and
the device envelope -- with the SAM of the UNMODIFIED reference mapper (oracle/_ref/kart -t 1) for them.

TEST INFRASTRUCTURE; runs only where oracle/_ref was built.  Everything is seeded and the gz members carry no time stamp: a second run writes the
same bytes.  The reads are cut from tests/golden/small.fa (index tests/golden/idx/small), contigs chrA and chrB, both strands, 150 and 300 bases.

  tests/golden/sam/shape_1.fq.gz        the reads (fewer than 2500: ONE chunk of the reference, EstDistance stays 1500)
  tests/golden/sam/shape_2.fq.gz        mate 2 of each: an error-free read 300 bases downstream on the other strand
  tests/golden/sam/shape_classes.txt    read name, class names (tests/shape_fixture.py defines the classes; data only)
  tests/golden/sam/shape_se.sam.gz      kart -t 1 -f shape_1
  tests/golden/sam/shape_pe.sam.gz      kart -t 1 -f shape_1 -f2 shape_2
  tests/golden/sam/shape_se_g20.sam.gz  kart -t 1 -f shape_1 -g 20

Every reference command runs twice, under two MALLOC_PERTURB_ fills, and must print the same bytes.

The sweep (about 150 000 reads, four in five of them variants of one edit pattern on the two strands of chrA and chrB): (a) a zone at the read's
start or end (1..60 / 1..110 bases) with a substitution at its inner edge and every 5, 8, 11 bases or nowhere else, alone or with an indel of
1..3 or an insertion + deletion of the same length (2..16) inside; (b) the same zone (2..50 bases) in the middle of the read; (c) the first or
last 2..14 bases all substituted; (d) two or three substitutions 1..3 bases apart; (e) a single indel of 1..9, 12 or 16 bases 3..59 bases from
either end, alone or next to a substitution; (f) edits every 14..29 bases over 150 and 300 bases, and 300-base reads with 7 or 8 evenly spaced
indels plus one inside the head and tail pairs (the envelope: seeds, gap pairs, CIGAR length).  Each read is seeded and chained by the CPU
oracle under -g 5 and -g 20, DROPPED unless it has exactly one candidate under both, and classified by tests/report_plain.py +
tests/shape_fixture.py under -g 5.  A read is KEPT WHEN ONE OF ITS CLASSES still holds fewer than 8 reads, and then counts for every class it has:
a class is sure of its first 8 members in sweep order and may end with many more (the common ones with over a hundred).  So that the common
members cannot stand in for the rare ones, what must be told apart is a class of its own: a head or tail geometry class counts every alignment
(the quality check walks it) and its "+ok" twin only those that PASS the check (the trimming and add_cigar walk them too); H.rLen50 / T.rLen100
hold only pairs that are aligned and pass (their CIGAR has M where a clip by length would print S), H.rLen51 / T.rLen101 only pairs whose
alignment would have passed as well; H.long / T.long only passing alignments, "+trim" those with a trimmed run.  A read outside the device
envelope is kept for its envelope class alone.  The generator prints the count per class and fails if a class of shape_fixture.wanted_classes()
stays below its least count, unless shape_fixture.UNREACHABLE names it; tests/test_shapes_cpu.py asserts that those hold no read, so that a
change which makes one reachable is noticed.

CLASSES OF wanted_classes() THAT DO NOT OCCUR (shape_fixture.UNREACHABLE), none found by any family of the sweep:
  H.L1-7 (and +ok),
  H.tiny-allmis           a head pair of fewer than 8 bases.  IdentifySeedPairs_FastMode starts its next search one base behind the LONGEST PREFIX
                          THAT OCCURS ANYWHERE in the text (pos += len + 1, src/AlignmentCandidates.cpp:62-74), found or not: the head pair is one
                          base longer than that prefix, and the text (2 x 97 kb) holds every 7-mer (asserted by tests/test_shapes_cpu.py).
                          Tail pairs of 1..7 columns do occur (the searches stop MinSeedLength before the end) and are held.
  M.L8                    a middle pair of exactly 8 columns.  For the same reason the read side of a middle pair is ONE base (the base the next
                          search skips) or at least 9, and the text side differs from it by at most MaxGaps = 5: 1..6 columns or 9 and more.
  M.rLen0                 a middle pair without read bases: two searches never touch in the read (the skipped base), and
                          CheckOverlappingSeeds only widens the gap.  A pure deletion between two seeds (CIGAR MDM) is a 1 x (1 + k) pair that
                          goes through nw_alignment; pure insertions (gLen == 0) occur and are held.
  H.p+p2                  a head with leading gaps on BOTH sides.  The head pair has equal sides (gGaps = rGaps, :458) and nw_alignment never opened
                          it with a gap run in the read followed by one in the text in 4 800 aligned heads that passed the quality check; tails
                          with both trailing runs (c and c2) occur and are held.  p + p2 == 8 and > 8 are held with one of the two runs.

    python oracle/make_golden_shapes.py
"""
import gzip
import io
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kart_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402
import shape_fixture as S  # noqa: E402
from ref_flags import reference_sam_and_never_assigned_flags  # noqa: E402

KART = os.path.join(ROOT, "oracle", "_ref", "kart")
ACGT = b"ACGT"
PER_CLASS = 8
MAX_READS = 2400


def gz_write(path, data):
    """gzip without a time stamp or a name in the member: the same bytes every run"""
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, compresslevel=9, mtime=0) as fh:
        fh.write(data)
    open(path, "wb").write(buf.getvalue())


def zone_edits(lo, hi, spacing, anchor_hi):
    """substitutions inside [lo, hi): at the zone's inner edge(s) and every `spacing` bases from there"""
    if anchor_hi:
        return [(p, "X", 1) for p in range(hi - 1, lo - 1, -spacing)]
    return [(p, "X", 1) for p in range(lo, hi, spacing)]


def sweep():
    """yields (family, read length, edits): edits are (position in the stretch the read is cut from -- negative: from its end --, 'X' / 'I' / 'D', bases)"""
    indels = [("I", k) for k in (1, 2, 3)] + [("D", k) for k in (1, 2, 3)]
    head_z = list(range(1, 21)) + [23, 24, 25, 31, 32, 33, 39, 40, 41, 45, 47, 48, 49, 50, 51, 52, 55, 60]
    tail_z = head_z + [63, 64, 65, 71, 72, 73, 80, 88, 89, 90, 95, 96, 97, 98, 99, 100, 101, 102, 105, 110]
    for role, zs in (("head", head_z), ("tail", tail_z)):
        for z in zs:
            for spacing in (5, 8, 11, 1000) * (2 if 9 <= z <= 16 else 1):
                if role == "head":
                    subs = zone_edits(0, z, spacing, True)
                    at = lambda o: o
                else:
                    subs = [(-1 - p, "X", 1) for p, _, _ in zone_edits(0, z, spacing, True)]
                    at = lambda o: -1 - o
                yield role, 150, subs
                offs = sorted({0, 1, 2, z // 3, z // 2, z - 3, z - 2, z - 1} & set(range(z)))
                for kind, k in indels:
                    for o in offs:
                        yield role, 150, subs + [(at(o), kind, k)]
                for k in (2, 4, 5, 6, 7, 8, 9, 10, 12, 16):   # an insertion and a deletion of the same length: the zone keeps its length
                    for o1, o2 in ((0, z - 1), (z - 1, 0), (1, z // 2), (z // 2, 1), (z // 2, z - 2)):
                        if 0 <= o1 < z and 0 <= o2 < z and o1 != o2 and k < z:
                            yield role, 150, subs + [(at(o1), "I", k), (at(o2), "D", k)]
    for z in range(2, 51):
        for a in ((60, 66, 77, 91) if z <= 14 else (60, 77)):
            for spacing in (5, 8, 11):
                subs = sorted(set(zone_edits(a, a + z, spacing, False)) | {(a + z - 1, "X", 1)})
                yield "middle", 150, subs
                for kind, k in indels:
                    for o in sorted({1, z // 2, z - 2} & set(range(1, z - 1))):
                        yield "middle", 150, subs + [(a + o, kind, k)]
                for k in (9, 10, 12, 16):
                    for o1, o2 in ((1, z - 2), (z - 2, 1), (z // 2, 2)):
                        if 0 < o1 < z - 1 and 0 < o2 < z - 1 and o1 != o2:
                            yield "middle", 150, subs + [(a + o1, "I", k), (a + o2, "D", k)]
    for k in range(2, 15):                                    # the first / last k bases all substituted, alone or with one more substitution further in
        for extra in (0, 3, 6, 9):
            for rep in range(3):
                yield "garbage", 150, [(p, "X", 1) for p in range(k)] + ([(k + extra, "X", 1)] if extra else [])
                yield "garbage", 150, [(-1 - p, "X", 1) for p in range(k)] + ([(-1 - k - extra, "X", 1)] if extra else [])
    for a in range(40, 110):                                  # two or three substitutions next to each other: the searches between them fail, the pair gets long
        for gaps in ((1,), (2,), (3,), (2, 2), (1, 3)):
            yield "close", 150, [(a, "X", 1)] + [(a + sum(gaps[:i + 1]), "X", 1) for i in range(len(gaps))]
    for d in range(3, 60):
        for kind, k in indels + [(kind, k) for k in (4, 5, 6, 7, 8, 9, 12, 16) for kind in "ID"]:
            for end in (1, -1):
                p = d if end > 0 else -1 - d
                yield "single", 150, [(p, kind, k)]
                yield "single", 150, [(p, kind, k), (p - end * 2, "X", 1)]
    rng = np.random.default_rng(41)
    for length in (150, 300):
        for step in range(14, 30):
            for rep in range(100 if length == 300 else 12):
                edits, p = [], int(rng.integers(5, step))
                while p < length - 8:
                    kind = "XXXID"[int(rng.integers(5))] if rep % 2 else "XID"[int(rng.integers(3))]
                    edits.append((p, kind, 1 if kind == "X" or rep % 3 else int(rng.integers(1, 4))))
                    p += step + int(rng.integers(-1, 2))
                yield "envelope", length, edits


def sweep_cigar():
    """300 bases, 7 or 8 indels evenly between the ends (a gap pair each), and an indel inside the head and tail pairs, which add CIGAR elements
    without adding gap pairs: CIGAR texts around the longest a record holds"""
    rng = np.random.default_rng(43)
    for rep in range(700):
        n = 7 + rep % 2
        edits = [(int(30 + (i + 0.5) * 240 / n + rng.integers(-4, 5)), "ID"[int(rng.integers(2))], 1 + int(rng.integers(4) == 0)) for i in range(n)]
        if rng.random() < 0.7:
            edits.append((int(rng.integers(4, 10)), "ID"[int(rng.integers(2))], 1))
        if rng.random() < 0.7:
            edits.append((-int(rng.integers(5, 11)), "ID"[int(rng.integers(2))], 1))
        yield "envelope", 300, edits


def build_read(g, x, length, reverse, edits, rng):
    """the read and the stretch [x, x + span) it was cut from, or None where an edit falls outside"""
    span = length + sum(k for _, kind, k in edits if kind == "D") - sum(k for _, kind, k in edits if kind == "I")
    s = g[x:x + span]
    if reverse:
        s = synth.revcomp(s)
    s = list(s.tobytes())
    seen = set()
    for p, kind, k in sorted(((p if p >= 0 else span + p, kind, k) for p, kind, k in edits), reverse=True):
        if p < 0 or p + (k if kind == "D" else 1) > len(s) or p in seen:
            return None, span
        seen.add(p)
        if kind == "X":
            s[p] = ACGT[(ACGT.index(s[p]) + 1 + int(rng.integers(3))) & 3]
        elif kind == "I":
            s[p:p] = [ACGT[int(i)] for i in rng.integers(0, 4, size=k)]
        else:
            del s[p:p + k]
    return (bytes(s) if len(s) == length else None), span


def mate_of(g, x, span, reverse, length):
    """mate 2 as the file holds it: as many error-free bases as the read has, whose near end lies MATE_OFFSET behind the read's start, on the other
    strand (the reference corrupts its heap on a 300-base read paired with a 150-base mate: both mates get one length)"""
    if not reverse:
        return synth.revcomp(g[x + S.MATE_OFFSET:x + S.MATE_OFFSET + length]).tobytes()
    e = x + span - S.MATE_OFFSET
    return g[e - length:e].tobytes()


def main():
    assert os.path.exists(KART), "build oracle/_ref first (make -C oracle ref)"
    lim = S.limits()
    wanted = S.wanted_classes(lim)
    _, seqs = S.genome()
    orc = O.Oracle(S.SMALL_PREFIX)
    gen = S.plain_genome(orc)
    rng = np.random.default_rng(2027)
    count = {c: 0 for c in wanted}
    chosen, tried, single = [], 0, 0
    for i, (family, length, edits) in enumerate(list(sweep()) + list(sweep_cigar())):
        for variant in range(4):                                      # strand x contig; the place moves with every read
            reverse, contig = bool(variant & 1), ("chrA", "chrB")[variant >> 1]
            if family == "envelope" and variant != i % 4:
                continue
            g = seqs[contig]
            x = int(rng.integers(600, len(g) - 1200))
            if not set(g[x - 200:x + 800].tobytes()) <= set(ACGT):
                continue
            read, span = build_read(g, x, length, reverse, edits, rng)
            if read is None:
                continue
            tried += 1
            reps = {name: S.model(orc, gen, read, mg) for name, mg in S.RUNS.items()}
            if any(r is None for r in reps.values()):
                continue
            single += 1
            rep = reps["se"]
            cls = S.fixture_classes(rep, lim, reverse, contig)
            need = {c for c in cls if count[c] < PER_CLASS}
            if not need:
                continue
            for c in cls:
                count[c] += 1
            name = "s%d:%s:%d:%s:%d" % (len(chosen), contig, x, "-" if reverse else "+", span)
            chosen.append((name, read, mate_of(g, x, span, reverse, length), sorted(cls)))
    print("sweep: %d reads built, %d with exactly one candidate under -g 5 and -g 20, %d kept" % (tried, single, len(chosen)))
    for c in sorted(wanted):
        print("  %-28s %3d%s" % (c, count[c], "" if count[c] >= wanted[c] else "   UNREACHABLE (documented)" if c in S.UNREACHABLE else "   <-- below %d" % wanted[c]))
    missing = [c for c in wanted if count[c] < wanted[c] and c not in S.UNREACHABLE]
    assert len(chosen) <= MAX_READS, len(chosen)
    if "--survey" in sys.argv:
        print("missing:", missing)
        return
    assert not missing, missing
    assert all(count[c] == 0 for c in S.UNREACHABLE), [c for c in S.UNREACHABLE if count[c]]

    with tempfile.TemporaryDirectory() as tmp:
        f1, f2 = os.path.join(tmp, "shape_1.fq"), os.path.join(tmp, "shape_2.fq")
        names = [c[0] for c in chosen]
        synth.write_fastq(f1, names, [np.frombuffer(c[1], np.uint8) for c in chosen], mate=1)
        synth.write_fastq(f2, names, [np.frombuffer(c[2], np.uint8) for c in chosen], mate=2)
        sams = {}
        for case, args in (("shape_se", ["-f", f1]), ("shape_pe", ["-f", f1, "-f2", f2]), ("shape_se_g20", ["-f", f1, "-g", "20"])):
            lines, never = reference_sam_and_never_assigned_flags(KART, ["-i", S.SMALL_PREFIX] + args, tmp)
            assert not never, (case, sorted(never)[:5])               # only deterministic output is kept
            sams[case] = b"\n".join(lines)
        # the model must reproduce the reference on every read kept, under both MaxGaps
        for run, mg in S.RUNS.items():
            lines = S.sam_lines(sams["shape_" + run])
            for name, read, _, _ in chosen:
                rep = S.model(orc, gen, read, mg)
                assert S.model_columns(rep, len(read)) == S.line_columns(lines[(name.encode(), 0)]), (run, name, S.model_columns(rep, len(read)), lines[(name.encode(), 0)][:9])
        gz_write(os.path.join(S.SAM, "shape_1.fq.gz"), open(f1, "rb").read())
        gz_write(os.path.join(S.SAM, "shape_2.fq.gz"), open(f2, "rb").read())
        for case, text in sams.items():
            gz_write(os.path.join(S.SAM, case + ".sam.gz"), text)
        open(S.CLASS_TABLE, "w").write("".join("%s %s\n" % (c[0], " ".join(c[3])) for c in chosen))
    for f in ("shape_1.fq.gz", "shape_2.fq.gz", "shape_se.sam.gz", "shape_pe.sam.gz", "shape_se_g20.sam.gz", "shape_classes.txt"):
        print("  %-22s %7d bytes" % (f, os.path.getsize(os.path.join(S.SAM, f))))
    orc.close()


if __name__ == "__main__":
    main()
