"""GenMappingReport for ONE alignment candidate, stated plainly (imported by name, like nw_plain and md_plain).

What the reference does with a candidate between chaining and the SAM line (src/AlignmentCandidates.cpp:648-723, not -pacbio), a column at a
time, in Python: the fragment pairs of IdentifyNormalPairs(rlen, -1, ...), for each of them Process{Head,Normal,Tail}SequencePair
(src/tools.cpp:225-397) with CalFragPairMismatchBases' rule (:40-47), CheckLocalAlignmentQuality (:255-290), the leading / trailing gap
trimming (:323-336, :375-391) and AddNewCigarElements (:49-104), the `s == 0` collapse of the head and tail pair (:681-704), GapPenalty
(:612-622), GenCoordinateInfo (:515-562) and GenerateCIGAR (:492-513).  Two things are taken from the CPU oracle, which its own tests hold
to the reference: the pair list (Oracle.identify_normal_pairs) and the gapped strings of a fragment pair (Oracle.normal_pair_alignment,
GenerateNormalPairAlignment of src/tools.cpp:142-223).  Everything that reads those strings is here, and shares no code with the kernels
or with kart_amd/csrc/host.

Besides the report, every pair leaves a SHAPE DESCRIPTOR: what the finish pass of the alignment stage (align_finish.hip) and the planning
kernels in front of it (align_plan.hip) have to get right for this pair -- the number of columns, the counts of the quality check, the
trimmed runs, the column every run of a class starts at, or the decision that was taken without an alignment.  tests/shape_fixture.py
turns the descriptors into the classes of the indel-shape fixture."""
import bisect


def mismatch_bases(f1: bytes, f2: bytes) -> int:
    """CalFragPairMismatchBases, src/tools.cpp:40-47"""
    c = 0
    for i in range(len(f1)):
        if f1[i] != f2[i]:
            c += 1
    return c


def within_mismatch_rule(rlen: int, glen: int, f1: bytes, f2: bytes):
    """the test in front of every alignment (src/tools.cpp:240, :301, :352): equal lengths, at most 2 mismatches and at most (int)(rLen * 0.2).
    Returns (taken, mismatches or None)"""
    if rlen != glen:
        return False, None
    n = mismatch_bases(f1, f2)
    return (n <= 2 and n <= int(rlen * 0.2)), n


DASH = ord("-")


def column_classes(a1: bytes, a2: bytes):
    """the class of every column as AddNewCigarElements sees it (:56, :69, :82): 'D' where the read side shows '-', else 'I' where the text
    side does, else 'M'"""
    return ["D" if a1[i] == DASH else "I" if a2[i] == DASH else "M" for i in range(len(a1))]


def class_runs(a1: bytes, a2: bytes):
    """[(class, first column, length)] of the maximal runs of one class"""
    out = []
    for i, c in enumerate(column_classes(a1, a2)):
        if out and out[-1][0] == c:
            out[-1][2] += 1
        else:
            out.append([c, i, 1])
    return [tuple(x) for x in out]


def local_alignment_quality(a1: bytes, a2: bytes):
    """CheckLocalAlignmentQuality, src/tools.cpp:255-290 -> (passes, iStatus, n, mis)"""
    aln_type, n, mis, status = -1, 0, 0, 0
    for i in range(len(a1)):
        if a1[i] == DASH:
            if aln_type != 0:
                aln_type = 0
                status += 1
        elif a2[i] == DASH:
            if aln_type != 1:
                aln_type = 1
                status += 1
        else:
            n += 1
            if a1[i] != a2[i]:
                mis += 1
            if aln_type != 2:
                aln_type = 2
                status += 1
    return not (status >= 4 or (mis >= 3 and mis >= int(n * 0.3))), status, n, mis


def add_new_cigar_elements(a1: bytes, a2: bytes, cigar_vec) -> int:
    """AddNewCigarElements, src/tools.cpp:49-104: appends (length, op) per run, returns the number of identical characters among the M columns"""
    state, c, score = "*", 0, 0
    for i in range(len(a1)):
        if a1[i] == DASH:
            cls = "D"
        elif a2[i] == DASH:
            cls = "I"
        else:
            cls = "M"
            if a1[i] == a2[i]:
                score += 1
        if cls == state:
            c += 1
        else:
            if c > 0:
                cigar_vec.append((c, state))
            c, state = 1, cls
    if c > 0:
        cigar_vec.append((c, state))
    return score


def leading(s: bytes) -> int:
    p = 0
    while p < len(s) and s[p] == DASH:
        p += 1
    return p


def trailing(s: bytes) -> int:
    c = 0
    while c < len(s) and s[len(s) - 1 - c] == DASH:
        c += 1
    return c


class Genome:
    """ChromosomeVec / ChrLocMap (src/bwt_index.cpp:240-252) from the contig table [(name, length)] and RefSequence (both strands, characters)"""

    def __init__(self, contigs, text: bytes):
        self.names = [c[0] for c in contigs]
        self.lens = [int(c[1]) for c in contigs]
        self.size = sum(self.lens)
        self.text = text
        assert len(text) == 2 * self.size
        self.fwd, self.rev, ends, at = [], [], [], 0
        for i, n in enumerate(self.lens):
            self.fwd.append(at)
            at += n
            self.rev.append(2 * self.size - at)
            ends.append((self.fwd[i] + n - 1, i))
            ends.append((self.rev[i] + n - 1, i))
        ends.sort()
        self.end_keys = [e[0] for e in ends]
        self.end_chr = [e[1] for e in ends]

    def lower_bound(self, g):
        """ChrLocMap.lower_bound(g) -> (key, contig) or None at end()"""
        i = bisect.bisect_left(self.end_keys, g)
        return None if i == len(self.end_keys) else (self.end_keys[i], self.end_chr[i])


def coordinates_valid(gen: Genome, sp) -> bool:
    """CheckCoordinateValidity, src/AlignmentCandidates.cpp:582-610"""
    g1, g2 = 0, 2 * gen.size
    for p in sp:
        if p["gLen"] > 0:
            g1 = p["gPos"]
            break
    for p in reversed(sp):
        if p["gLen"] > 0:
            g2 = p["gPos"] + p["gLen"] - 1
            break
    if (g1 < gen.size) != (g2 < gen.size):
        return False
    i1, i2 = gen.lower_bound(g1), gen.lower_bound(g2)
    return i1 is not None and i2 is not None and i1[1] == i2[1]


def generate_cigar(cigar_vec) -> str:
    """GenerateCIGAR, src/AlignmentCandidates.cpp:492-513: neighbours of one op merge"""
    out, state, c = "", None, 0
    for n, op in cigar_vec:
        if op != state:
            if c > 0:
                out += "%d%s" % (c, state)
            c, state = n, op
        else:
            c += n
    if c > 0:
        out += "%d%s" % (c, state)
    return out


def gen_coordinate_info(gen: Genome, first: bool, g_pos: int, end_g_pos: int, cigar_vec):
    """GenCoordinateInfo, src/AlignmentCandidates.cpp:515-562 -> (contig index, 1-based position, forward?, CIGAR text)"""
    if g_pos < gen.size:
        fwd = first
        if len(gen.lens) == 1:
            chrom, pos = 0, g_pos + 1
        else:
            chrom = gen.lower_bound(g_pos)[1]
            pos = g_pos + 1 - gen.fwd[chrom]
    else:
        fwd = not first
        cigar_vec = cigar_vec[::-1]
        if len(gen.lens) == 1:
            chrom, pos = 0, 2 * gen.size - end_g_pos
        else:
            key, chrom = gen.lower_bound(g_pos)
            pos = key - end_g_pos + 1
    return chrom, pos, fwd, generate_cigar(cigar_vec)


def _end_pair(role, read, p, gen, orc, max_gaps, cigar_vec, shape):
    """ProcessHeadSequencePair (src/tools.cpp:292-342) / ProcessTailSequencePair (:344-397); moves the pair as the trimming does"""
    r_len, g_len = p["rLen"], p["gLen"]
    f1, f2 = read[p["rPos"]:p["rPos"] + r_len], gen.text[p["gPos"]:p["gPos"] + g_len]
    taken, n = within_mismatch_rule(r_len, g_len, f1, f2)
    shape.update(role=role, rLen=r_len, gLen=g_len, rule_mismatches=n)
    if taken:
        cigar_vec.append((r_len, "M"))
        shape["decided"] = "M-rule"
        return r_len - n
    if r_len > (50 if role == "head" else 100):                       # :307-311, :358-362
        cigar_vec.append((r_len, "S"))
        a1, a2 = orc.normal_pair_alignment(f1, f2, pacbio=False, max_gaps=max_gaps)   # (the reference does not align it: what the quality check WOULD
        shape.update(decided="S-length", ok_if_aligned=local_alignment_quality(a1, a2)[0])   #  say tells a clip by length from one that hides behind a failure)
        return 0
    a1, a2 = orc.normal_pair_alignment(f1, f2, pacbio=False, max_gaps=max_gaps)
    ok, status, n_cols, mis = local_alignment_quality(a1, a2)
    shape.update(decided="aligned", L=len(a1), iStatus=status, n=n_cols, mis=mis, ok=ok, runs=class_runs(a1, a2), trim=(0, 0))
    if not ok:
        cigar_vec.append((r_len, "S"))
        return 0
    if role == "head":
        t1 = leading(a1)                                              # :324-329: leading gaps in the read block shrink the genome block
        a1, a2 = a1[t1:], a2[t1:]
        p["gPos"] += t1
        p["gLen"] -= t1
        t2 = leading(a2)                                              # :331-336: leading gaps in the genome block are clipped
        a1, a2 = a1[t2:], a2[t2:]
        p["rPos"] += t2
        p["rLen"] -= t2
        if t2 > 0:
            cigar_vec.append((t2, "S"))
        score = add_new_cigar_elements(a1, a2, cigar_vec)
    else:
        t1 = trailing(a1)                                             # :377-383
        a1, a2 = a1[:len(a1) - t1], a2[:len(a2) - t1]
        p["gLen"] -= t1
        t2 = trailing(a2)                                             # :385-391
        a1, a2 = a1[:len(a1) - t2], a2[:len(a2) - t2]
        p["rLen"] -= t2
        score = add_new_cigar_elements(a1, a2, cigar_vec)
        if t2 > 0:                                                    # (:392 tests the second count alone)
            cigar_vec.append((t2, "S"))
    shape.update(trim=(t1, t2), score=score)
    return score


def _middle_pair(read, p, gen, orc, max_gaps, cigar_vec, shape):
    """ProcessNormalSequencePair, src/tools.cpp:225-253"""
    r_len, g_len = p["rLen"], p["gLen"]
    shape.update(role="middle", rLen=r_len, gLen=g_len, rule_mismatches=None)
    if r_len == 0 or g_len == 0:
        if r_len > 0:
            cigar_vec.append((r_len, "I"))
            shape["decided"] = "I"
        elif g_len > 0:
            cigar_vec.append((g_len, "D"))
            shape["decided"] = "D"
        return 0
    f1, f2 = read[p["rPos"]:p["rPos"] + r_len], gen.text[p["gPos"]:p["gPos"] + g_len]
    taken, n = within_mismatch_rule(r_len, g_len, f1, f2)
    shape["rule_mismatches"] = n
    if taken:
        cigar_vec.append((r_len, "M"))
        shape["decided"] = "M-rule"
        return r_len - n
    a1, a2 = orc.normal_pair_alignment(f1, f2, pacbio=False, max_gaps=max_gaps)
    score = add_new_cigar_elements(a1, a2, cigar_vec)
    shape.update(decided="aligned", L=len(a1), iStatus=None, n=None, mis=None, ok=None, runs=class_runs(a1, a2), trim=(0, 0), score=score)
    return score


def report(read: bytes, seeds, orc, gen: Genome, max_gaps: int = 5, first: bool = True):
    """GenMappingReport's body for one candidate (src/AlignmentCandidates.cpp:648-723).  `seeds`: the candidate's pair array as
    Oracle.candidates gives it.  Returns a dict: score (AlnScore, 0: nothing is reported), cigar, contig (name), pos (1-based), fwd, shapes (one
    descriptor per non-simple pair, in order), seeds / gap_pairs (simple pairs and the pairs inserted BETWEEN them after IdentifyNormalPairs'
    filters), elements (CIGAR elements before merging)"""
    v = orc.identify_normal_pairs(len(read), -1, seeds)                                       # :648
    sp = [{"rPos": int(x["rPos"]), "gPos": int(x["gPos"]), "rLen": int(x["rLen"]), "gLen": int(x["gLen"]), "simple": bool(x["bSimple"])} for x in v]
    num = len(sp)
    out = {"score": 0, "cigar": "", "contig": None, "pos": 0, "fwd": True, "shapes": [], "elements": 0,
           "seeds": sum(1 for p in sp if p["simple"]),
           "gap_pairs": sum(1 for j, p in enumerate(sp) if not p["simple"] and 0 < j < num - 1)}
    if not coordinates_valid(gen, sp):                                                         # :654
        return out
    cigar_vec, score = [], 0
    for j, p in enumerate(sp):
        if p["rLen"] == 0 and p["gLen"] == 0:                                                  # :659
            continue
        if p["simple"]:                                                                        # :660-665
            cigar_vec.append((p["rLen"], "M"))
            score += p["rLen"]
            continue
        shape = {}
        if j == 0:                                                                             # :669-687
            if p["rLen"] > 3000:
                cigar_vec.append((p["rLen"], "S"))
                shape.update(role="head", rLen=p["rLen"], gLen=p["gLen"], decided="S-3000")
                s = 0
            else:
                s = _end_pair("head", read, p, gen, orc, max_gaps, cigar_vec, shape)
                score += s
            if s == 0:
                p["gPos"], p["gLen"] = sp[1]["gPos"], 0
        elif j == num - 1:                                                                     # :688-706
            if p["rLen"] > 3000:
                cigar_vec.append((p["rLen"], "S"))
                shape.update(role="tail", rLen=p["rLen"], gLen=p["gLen"], decided="S-3000")
                s = 0
            else:
                s = _end_pair("tail", read, p, gen, orc, max_gaps, cigar_vec, shape)
                score += s
            if s == 0:
                p["gPos"], p["gLen"] = sp[j - 1]["gPos"] + sp[j - 1]["gLen"], 0
        else:
            score += _middle_pair(read, p, gen, orc, max_gaps, cigar_vec, shape)               # :709
        shape["collapsed"] = shape["role"] != "middle" and s == 0
        out["shapes"].append(shape)
    out["elements"] = len(cigar_vec)
    if len(cigar_vec) > 1:                                                                     # :714-722
        score -= sum(n for n, op in cigar_vec if op in "ID")                                   # GapPenalty, :612-622
        if score <= 0:
            return out
    if not cigar_vec:                                                                          # :723
        return out
    chrom, pos, fwd, cigar = gen_coordinate_info(gen, first, sp[0]["gPos"], sp[num - 1]["gPos"] + sp[num - 1]["gLen"] - 1, cigar_vec)
    if pos <= 0:
        return out
    out.update(score=score, cigar=cigar, contig=gen.names[chrom], pos=pos, fwd=fwd)
    return out
