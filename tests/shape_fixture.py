"""The indel-shape fixture (tests/golden/sam/shape_*; written by oracle/make_golden_shapes.py) as the tests and its generator read it: the
reads, the class table, the classes themselves (from the shape descriptors of tests/report_plain.py), the limits of the device path read
from the kernels' sources, and the model's record per read.

A CLASS is a property of ONE read with ONE candidate, named "<role>.<what>" (role H / M / T: the head, a middle or the tail pair), "rule.*" /
"Q.*" for the decision thresholds, "E.*" for the device envelope.  A head or tail whose alignment FAILS the quality check is clipped whole: it exercises the check and nothing behind it.  So
every tile geometry class of a head or tail has a twin "...+ok" that counts only alignments which pass (the trimming and add_cigar walk those), and the
classes that stand for something behind the check (the trimming, the length limits, the long ends) hold passing alignments only.  The tail-trimming classes come a second and third time, for reads on the
reverse strand ("...|rev": POS comes from end_gPos, which the trimming moves) and for reads on chrB ("...|chrB")."""
import gzip
import os
import re

import numpy as np

import report_plain as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
SAM = os.path.join(GOLDEN, "sam")
SMALL_FA = os.path.join(GOLDEN, "small.fa")
SMALL_PREFIX = os.path.join(GOLDEN, "idx", "small")
CLASS_TABLE = os.path.join(SAM, "shape_classes.txt")
TILE = 8                       # kFinG of align_finish.hip: columns per tile (asserted against the source by limits())
MATE_OFFSET = 300              # mate 2: an error-free read this far downstream, on the other strand
RUNS = {"se": 5, "se_g20": 20}               # the single-end runs: name -> MaxGaps
LONG = {"H": 45, "T": 90}                    # columns from which a head / tail counts as long (they align at most 50 / 100 read bases)


def limits():
    """the device envelope, read from the sources: seeds and gap pairs of a candidate (align_kernels.hpp), CIGAR elements before merging, the
    longest CIGAR text a kg_aln_record takes -- report_by_group refuses an element when `at + nd + 1 > KG_ALN_CIGAR_MAX - 1`, so the text holds
    at most KG_ALN_CIGAR_MAX - 1 characters -- and the tile of the finish pass"""
    hpp = open(os.path.join(ROOT, "kart_amd", "csrc", "align_kernels.hpp")).read()
    fin = open(os.path.join(ROOT, "kart_amd", "csrc", "align_finish.hip")).read()
    api = open(os.path.join(ROOT, "include", "kart_amd.h")).read()
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    seeds, gaps = const(hpp, "kAlnMaxSeeds"), const(hpp, "kAlnMaxGaps")
    assert re.search(r"constexpr int kAlnMaxPairs = kAlnMaxSeeds \+ kAlnMaxGaps \+ 2;", hpp) and re.search(r"constexpr int kAlnMaxCigar = 2 \* kAlnMaxPairs \+ 8;", hpp)
    cigar_max = int(re.search(r"#define KG_ALN_CIGAR_MAX (\d+)", api).group(1))
    assert "if (at + nd + 1 > KG_ALN_CIGAR_MAX - 1) { fits = false; return; }" in fin
    assert const(fin, "kFinG") == TILE
    return {"seeds": seeds, "gaps": gaps, "elements": 2 * (seeds + gaps + 2) + 8, "cigar_text": cigar_max - 1}


def genome():
    """(report_plain.Genome's contig table, {name: ASCII array}) of tests/golden/small.fa"""
    from kart_amd.index_build import read_fasta
    seqs = read_fasta(SMALL_FA)
    return [(n, len(s)) for n, _, s in seqs], {n: s for n, _, s in seqs}


def plain_genome(orc):
    contigs, _ = genome()
    return P.Genome(contigs, orc.ref_sequence().tobytes())


def read_fastq_gz(path):
    lines = gzip.open(path).read().split(b"\n")
    n = len(lines) // 4
    return [lines[4 * i][1:].split(b"\t")[0] for i in range(n)], [lines[4 * i + 1] for i in range(n)]


def load_reads():
    """(names, mate 1 sequences, mate 2 sequences as the file holds them)"""
    names, s1 = read_fastq_gz(os.path.join(SAM, "shape_1.fq.gz"))
    names2, s2 = read_fastq_gz(os.path.join(SAM, "shape_2.fq.gz"))
    assert names == names2
    return names, s1, s2


def load_sam(name):
    return gzip.open(os.path.join(SAM, name + ".sam.gz")).read()


def load_class_table():
    out = {}
    for line in open(CLASS_TABLE):
        f = line.split()
        out[f[0].encode()] = set(f[1:])
    return out


def map_read(orc, read: bytes, max_gaps: int):
    """the read's candidates from the CPU oracle: IdentifySeedPairs_FastMode + GenerateAlignmentCandidateForIlluminaSeq"""
    from kart_amd import synth
    seeds = orc.seed_read(synth.encode(np.frombuffer(read, np.uint8)), 0)
    return orc.candidates(len(read), seeds, False, max_gaps)


def model(orc, gen, read: bytes, max_gaps: int):
    """report_plain's report of the read's ONLY candidate, or None when it has another number of candidates"""
    cands = map_read(orc, read, max_gaps)
    if len(cands) != 1:
        return None
    rep = P.report(read, cands[0][2], orc, gen, max_gaps, True)
    rep["chain_seeds"] = len(cands[0][2])
    return rep


def host_reason(rep, lim):
    """the reason index of kg_align_reasons() under which the device path hands the read back, in the order the kernels test (aln_plan_kernel: seeds,
    then gap pairs; the finish pass: CIGAR), or None for a read it decides"""
    if rep["chain_seeds"] > lim["seeds"]:
        return 6
    if rep["gap_pairs"] > lim["gaps"]:
        return 7
    if rep["elements"] > lim["elements"] or len(rep["cigar"]) > lim["cigar_text"]:
        return 10
    return None


GEOMETRY = ("L1-7", "L8", "L%8=0", "L%8=1", "L%8=7", "change@8k", "gapstart@8k", "gapend@8k-1", "gap9D", "gap9I")
TAIL_TRIM = ("T.c", "T.c2", "T.c+c2", "T.kept%8=0", "T.trim-crosses-tile", "T.L%8=0+trail")
UNREACHABLE = ("H.L1-7", "H.L1-7+ok", "H.tiny-allmis", "M.L8", "M.rLen0", "H.p+p2")       # classes of wanted_classes() no read of the generator's sweep has: its docstring says why


def classes_of(rep, lim, reverse: bool, contig: str):
    """the class names of one read from its report"""
    out = set()
    mapped = rep["score"] > 0
    for d in rep["shapes"]:
        r = d["role"][0].upper()
        rl, gl, dec = d["rLen"], d["gLen"], d["decided"]
        n = d.get("rule_mismatches")
        # ---- decisions without an alignment ----
        if rl == gl and n is not None:
            if rl >= 15 and n in (2, 3):
                out.add("%s.rule.%dmm" % (r, n))
            if rl in (4, 5, 9, 10, 14) and n in (1, 2):
                out.add("rule.rLen%d.%dmm" % (rl, n))
        # the clip by length, told from the whole-fragment S of a failed quality check: at the limit the pair is aligned and PASSES (its CIGAR holds M),
        # one base above it is clipped although its alignment would pass too
        limit = {"H": 50, "T": 100}.get(r)
        if limit is not None and ((rl == limit and dec == "aligned" and d["ok"]) or (rl == limit + 1 and dec == "S-length" and d["ok_if_aligned"])):
            out.add("%s.rLen%d" % (r, rl))
        if r == "M":
            if dec in ("I", "D"):
                out.add("M.gLen0" if dec == "I" else "M.rLen0")
            elif rl == gl:
                out.add("M.eq.rule" if dec == "M-rule" else "M.eq.aligned")
            if dec == "aligned":
                if (rl, gl) in ((30, 31), (31, 30), (31, 31)):
                    out.add("M.%dx%d" % (rl, gl))
                if rl >= 40 and gl >= 40:
                    out.add("M.above30")
        if dec != "aligned":
            continue
        # ---- tile geometry ----
        L, runs = d["L"], d["runs"]
        geo = set()
        if L < TILE:
            geo.add(r + ".L1-7")
        elif L == TILE:
            geo.add(r + ".L8")
        elif L % TILE in (0, 1, 7):
            geo.add("%s.L%%8=%d" % (r, L % TILE))
        for cls, start, length in runs:
            end = start + length
            if start > 0 and start % TILE == 0:
                geo.add(r + ".change@8k")
                if cls in "DI":
                    geo.add(r + ".gapstart@8k")
            if cls in "DI" and end % TILE == 0 and end < L:
                geo.add(r + ".gapend@8k-1")
            if cls in "DI" and length >= 9 and (start + TILE - 1) // TILE * TILE + TILE <= end and len(runs) > 1:
                geo.add("%s.gap9%s" % (r, cls))
        out |= geo
        if r == "M":
            continue
        # a head or tail that fails the quality check goes through quality_ok alone; one that passes ("+ok") also through the trimming and add_cigar
        if d["ok"]:
            out |= {g + "+ok" for g in geo}
            if L >= LONG[r]:
                out.add(r + ".long")
                if sum(d["trim"]) > 0:
                    out.add(r + ".long+trim")
        # ---- the quality check and the trimming ----
        ok, status, nn, mis = d["ok"], d["iStatus"], d["n"], d["mis"]
        if status in (3, 4):
            out.add("Q.iStatus%d" % status)
        if mis in (2, 3) and status < 4:
            out.add("Q.mis%d" % mis)
        if nn in (9, 10, 13, 14) and mis in (2, 3, 4) and status < 4:
            out.add("Q.n%d.mis%d" % (nn, mis))
        if not ok:
            out.add(r + ".fail")
            continue
        if L <= 2 and mis == nn == L:
            out.add(r + ".tiny-allmis")
        t1, t2 = d["trim"]
        trims = set()
        if r == "H":
            if t1 > 0 and t2 == 0:
                trims.add("H.p")
            if t2 > 0 and t1 == 0:
                trims.add("H.p2")
            if t1 > 0 and t2 > 0:
                trims.add("H.p+p2")
            if t1 + t2 == TILE:
                trims.add("H.p+p2=8")
            if t1 + t2 > TILE:
                trims.add("H.p+p2>8")
        else:
            if t1 > 0 and t2 == 0:
                trims.add("T.c")
            if t2 > 0 and t1 == 0:
                trims.add("T.c2")
            if t1 > 0 and t2 > 0:
                trims.add("T.c+c2")
            if t1 + t2 > 0:
                kept = L - t1 - t2
                if kept % TILE == 0:
                    trims.add("T.kept%8=0")
                if kept // TILE < (L - 1) // TILE:
                    trims.add("T.trim-crosses-tile")
                if L % TILE == 0:
                    trims.add("T.L%8=0+trail")
            if mapped:
                for t in list(trims):
                    if reverse:
                        trims.add(t + "|rev")
                    if contig == "chrB":
                        trims.add(t + "|chrB")
        out |= trims
    # ---- the envelope ----
    if rep["chain_seeds"] in (lim["seeds"], lim["seeds"] + 1):
        out.add("E.seeds%d" % rep["chain_seeds"])
    if rep["chain_seeds"] <= lim["seeds"]:
        if rep["gap_pairs"] in (lim["gaps"], lim["gaps"] + 1):
            out.add("E.gaps%d" % rep["gap_pairs"])
        if rep["gap_pairs"] <= lim["gaps"] and mapped and rep["elements"] <= lim["elements"]:
            if len(rep["cigar"]) == lim["cigar_text"]:
                out.add("E.cigar-longest")
            if len(rep["cigar"]) == lim["cigar_text"] + 1:
                out.add("E.cigar-over")
    return out


def wanted_classes(lim):
    """every class the fixture is to hold -> the least number of reads it must hold (4; 2 where strand or contig is itself the class).  The tile
    geometry classes of a head or a tail come twice: whatever the quality check says, and "+ok" for alignments that pass it"""
    w = {}
    for r in "HMT":
        for c in GEOMETRY:
            w["%s.%s" % (r, c)] = 4
            if r != "M":
                w["%s.%s+ok" % (r, c)] = 4
        for c in ("rule.2mm", "rule.3mm"):
            w["%s.%s" % (r, c)] = 4
    for c in ("H.long", "T.long", "H.long+trim", "T.long+trim", "H.p", "H.p2", "H.p+p2", "H.p+p2=8", "H.p+p2>8", "H.rLen50", "H.rLen51", "T.rLen100", "T.rLen101", "H.fail", "T.fail",
              "H.tiny-allmis", "T.tiny-allmis", "M.rLen0", "M.gLen0", "M.eq.rule", "M.eq.aligned", "M.30x31", "M.31x30", "M.31x31", "M.above30",
              "Q.iStatus3", "Q.iStatus4", "Q.mis2", "Q.mis3", "Q.n9.mis2", "Q.n9.mis3", "Q.n10.mis2", "Q.n10.mis3", "Q.n13.mis2", "Q.n13.mis3", "Q.n14.mis3", "Q.n14.mis4"):
        w[c] = 4
    for rl in (4, 5, 9, 10, 14):
        for n in (1, 2):
            w["rule.rLen%d.%dmm" % (rl, n)] = 4
    for c in TAIL_TRIM:
        w[c] = 4
        w[c + "|rev"] = 2
        w[c + "|chrB"] = 2
    for c in ("E.seeds%d" % lim["seeds"], "E.seeds%d" % (lim["seeds"] + 1), "E.gaps%d" % lim["gaps"], "E.gaps%d" % (lim["gaps"] + 1), "E.cigar-longest", "E.cigar-over"):
        w[c] = 4
    return w


def fixture_classes(rep, lim, reverse: bool, contig: str):
    """the classes a read stands for in the fixture: the wanted ones, and for a read outside the device envelope its envelope class alone (the
    device never sees its shapes)"""
    cls = classes_of(rep, lim, reverse, contig) & set(wanted_classes(lim))
    if host_reason(rep, lim) is not None:
        cls = {c for c in cls if c.startswith("E.")}
    return cls


def strand_and_contig(name: bytes):
    """read names carry their origin: <id>:<contig>:<0-based start>:<+ or ->:<length of the stretch of the contig the read was cut from>"""
    f = name.split(b":")
    return f[3] == b"-", f[1].decode()


def sam_lines(text: bytes):
    """{(name, mate 0 / 1): fields} of a SAM text that prints one line per read"""
    out = {}
    for line in text.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        key = (f[0], 1 if int(f[1]) & 0x80 else 0)
        assert key not in out, key
        out[key] = f
    return out


def model_columns(rep, rlen):
    """(reverse strand shown, RNAME, POS, CIGAR, AS, NM) as the reference prints a single-end read with this one candidate
    (src/Mapping.cpp:272-315: an AlnScore of 0 is the unmapped record)"""
    if rep["score"] <= 0:
        return (False, b"*", 0, b"*", 0, None)
    return (not rep["fwd"], rep["contig"].encode(), rep["pos"], rep["cigar"].encode(), rep["score"], rlen - rep["score"])


def line_columns(f):
    tags = dict(t.split(b":i:") for t in f[11:] if b":i:" in t)
    return (bool(int(f[1]) & 16), f[2], int(f[3]), f[5], int(tags[b"AS"]), int(tags[b"NM"]) if b"NM" in tags else None)
