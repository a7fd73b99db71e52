"""MD:Z in plain Python, written from the SAM specification (v1, section 1.5: [0-9]+(([A-Z]|\\^[A-Z]+)[0-9]+)*) and samtools calmd's matching rule.
Shares nothing with the product: the tests hold the host's and the device's strings to this one.

md_of(seq, cigar, ref_at)          the MD of a record whose printed SEQ is `seq` and whose CIGAR is `cigar`; ref_at(k) is the character the reference
                                   shows at the k-th reference base the record consumes (k = 0 at POS).  ref_at carries the hole rule: reference_at()
                                   below builds it from a contig's sequence, POS and the holes of .amb
ref_from_md(seq, cigar, md)        the reference bases the record consumes, rebuilt from SEQ, CIGAR and MD (a matching column takes the read's
                                   character, upper case; '=' cannot be rebuilt and comes back as '=')
Rules: an M (or =, X) column matches when the upper-cased read character is one of ACGT and equals the reference character, or when the read character
is '='; every other column is a mismatch and shows the reference character, upper case.  D shows '^' and the deleted reference characters; I and S
consume read only; N consumes reference only; H and P nothing.  A number -- 0 where nothing matched -- stands in front, behind and between any two of
these.  A reference position inside a hole shows the hole's own character (upper case), which is none of ACGT and so matches nothing but '=';
a position outside the contig shows N."""
import re

CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=X])")
MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")


def cigar_ops(cigar):
    ops = [(int(n), op) for n, op in CIGAR_RE.findall(cigar)]
    assert "".join("%d%s" % x for x in ops) == cigar, cigar
    return ops


def md_of(seq, cigar, ref_at):
    out, run, r, g = [], 0, 0, 0
    for n, op in cigar_ops(cigar):
        if op in "M=X":
            for _ in range(n):
                c, ref = seq[r], ref_at(g).upper()
                if c == "=" or (c.upper() in "ACGT" and c.upper() == ref):
                    run += 1
                else:
                    out.append(str(run) + ref)
                    run = 0
                r += 1
                g += 1
        elif op == "D":
            out.append(str(run) + "^" + "".join(ref_at(g + k).upper() for k in range(n)))
            run = 0
            g += n
        elif op == "N":
            g += n
        elif op in "IS":
            r += n
    out.append(str(run))
    return "".join(out)


def reference_at(contig_seq, pos, holes=()):
    """ref_at for a record at 1-based POS `pos` of a contig whose sequence (as the index holds it, or as the FASTA has it) is contig_seq;
    holes: (start, length, character) with start 0-based in the contig"""
    def at(k):
        i = pos - 1 + k
        if i < 0 or i >= len(contig_seq):
            return "N"
        for s, n, ch in holes:
            if s <= i < s + n:
                return ch.upper()
        return contig_seq[i].upper()
    return at


def ref_from_md(seq, cigar, md):
    assert MD_RE.fullmatch(md), md
    items = re.findall(r"[0-9]+|\^[A-Z]+|[A-Z]", md)
    # the MD as one instruction per reference base of M and D operations
    per_base = []
    for it in items:
        if it[0].isdigit():
            per_base += [None] * int(it)
        elif it[0] == "^":
            per_base += [("D", c) for c in it[1:]]
        else:
            per_base.append(("X", it))
    out, r, k = [], 0, 0
    for n, op in cigar_ops(cigar):
        if op in "M=X":
            for _ in range(n):
                what = per_base[k]
                assert what is None or what[0] == "X", (md, cigar)
                out.append(seq[r].upper() if what is None else what[1])
                r += 1
                k += 1
        elif op == "D":
            for _ in range(n):
                assert per_base[k] is not None and per_base[k][0] == "D", (md, cigar)
                out.append(per_base[k][1])
                k += 1
        elif op in "IS":
            r += n
    assert k == len(per_base), (md, cigar)
    return "".join(out)
