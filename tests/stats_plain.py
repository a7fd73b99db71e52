"""A plain recount of what -stats writes: SAM text in, the file's bytes out (and, for the API tests, a row in the layout of kg_stream_set_stats).
Nothing here comes from the product: the file's format and the row's layout are written out again from their description in include/kart_amd.h and
README.md, so that a slip on either side shows as a difference."""
import numpy as np

HEADER_TAGS = (b"@HD\t", b"@SQ\t", b"@RG\t", b"@PG\t", b"@CO\t")

# the row: uint32 words
RECORDS, FLAG0, PROPER, BOTH_MAPPED, SINGLETON, CIGAR0, MAPQ0, ISIZE0 = 0, 1, 13, 14, 15, 16, 26, 90
ISIZE_MAX = 2048
WORDS = ISIZE0 + ISIZE_MAX + 1
CIGAR_CLASSES = ("M", "I", "D", "S", "other")


def records(sam_text: bytes):
    """the fields of every record line (the header lines lead the text)"""
    lines = sam_text.split(b"\n")
    k = 0
    while k < len(lines) and lines[k].startswith(HEADER_TAGS):
        k += 1
    return [ln.split(b"\t") for ln in lines[k:] if ln]


def cigar_ops(cigar: bytes):
    """[(length, letter)] -- "*" has none"""
    ops, num = [], ""
    if cigar == b"*":
        return ops
    for ch in cigar.decode():
        if ch.isdigit():
            num += ch
        else:
            ops.append((int(num) if num else 0, ch))          # (a letter without a number counts as an operation of length 0)
            num = ""
    assert num == ""
    return ops


class Count:
    def __init__(self):
        self.records = self.proper = self.both = self.singleton = 0
        self.flag = [0] * 12
        self.mapq = {}
        self.isize = {}
        self.cigar = {k: [0, 0] for k in CIGAR_CLASSES}

    def add(self, f):
        flag, mapq, cigar, rnext, tlen = int(f[1]), int(f[4]), f[5], f[6], int(f[8])
        mapped = not flag & 4
        self.records += 1
        for b in range(12):
            if flag & (1 << b):
                self.flag[b] += 1
        if flag & 1 and flag & 2 and mapped:
            self.proper += 1
        if flag & 1 and not flag & 12:
            self.both += 1
        if flag & 1 and mapped and flag & 8:
            self.singleton += 1
        if mapped:
            q = min(mapq, 63)
            self.mapq[q] = self.mapq.get(q, 0) + 1
            for n, ch in cigar_ops(cigar):
                k = ch if ch in "MIDS" else "other"
                self.cigar[k][0] += n
                self.cigar[k][1] += 1
        if flag & 1 and rnext == b"=" and tlen > 0:
            d = min(tlen, ISIZE_MAX)
            self.isize[d] = self.isize.get(d, 0) + 1


def count(recs) -> Count:
    c = Count()
    for f in recs:
        c.add(f)
    return c


def text(sam_text: bytes) -> bytes:
    """the -stats file of a run that printed sam_text"""
    return text_of(count(records(sam_text)))


def text_of(c: Count) -> bytes:
    unmapped = c.flag[2]
    out = ["# kart-amd stats 1"]
    for key, v in (("records", c.records), ("mapped", c.records - unmapped), ("unmapped", unmapped), ("proper_pair", c.proper), ("both_mapped", c.both),
                   ("singleton", c.singleton)):
        out.append("SN\t%s\t%d" % (key, v))
    for b in range(12):
        out.append("FL\t0x%x\t%d" % (1 << b, c.flag[b]))
    for q in sorted(c.mapq):
        out.append("MQ\t%d\t%d" % (q, c.mapq[q]))
    for d in sorted(c.isize):
        out.append("IS\t%s\t%d" % (">=2048" if d == ISIZE_MAX else str(d), c.isize[d]))
    for k in CIGAR_CLASSES:
        out.append("CG\t%s\t%d\t%d" % (k, c.cigar[k][0], c.cigar[k][1]))
    return ("\n".join(out) + "\n").encode()


def row_of(c: Count) -> np.ndarray:
    r = np.zeros(WORDS, dtype=np.uint32)
    r[RECORDS], r[PROPER], r[BOTH_MAPPED], r[SINGLETON] = c.records, c.proper, c.both, c.singleton
    r[FLAG0:FLAG0 + 12] = c.flag
    for i, k in enumerate(CIGAR_CLASSES):
        r[CIGAR0 + 2 * i], r[CIGAR0 + 2 * i + 1] = c.cigar[k]
    for q, n in c.mapq.items():
        r[MAPQ0 + q] = n
    for d, n in c.isize.items():
        r[ISIZE0 + d] = n
    return r


def row(sam_text: bytes) -> np.ndarray:
    """the row kg_stream_set_stats makes of the records of sam_text (record lines only, or a whole file)"""
    return row_of(count(records(sam_text)))
