"""The plain specification of -un / -un2 (no project code): which bytes of the read files a run writes back, given its SAM text.

A record's span runs from the first byte of its header line through the line feed of its last line -- FASTQ: four lines; FASTA: the header and every
line up to the next line that starts with '>' or the end -- and nothing in it is changed; a file whose last line has no line feed gets one.  A
single-end read is written iff its record has FLAG & 4; a pair iff BOTH mates have (`samtools fastq -f 4` / `-f 12`)."""


def spans(text: bytes, fasta: bool):
    """(begin, end) of every record of `text`, in order"""
    ends, at = [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        at = len(text) if nl < 0 else nl + 1
        ends.append(at)
    begins = [0] + ends[:-1]
    if not fasta:
        return [(begins[i], ends[i + 3]) for i in range(0, len(ends) - 3, 4)]
    heads = [i for i in range(len(ends)) if i == 0 or text[begins[i]:begins[i] + 1] == b">"]
    return [(begins[h], ends[(heads[k + 1] if k + 1 < len(heads) else len(ends)) - 1]) for k, h in enumerate(heads)]


def records(text: bytes, fasta: bool):
    """the bytes -un writes for every record of `text`"""
    return [text[b:e] + (b"" if text[e - 1:e] == b"\n" else b"\n") for b, e in spans(text, fasta)]


def name_of(record: bytes) -> bytes:
    """QNAME as the mapper prints it: from the first byte behind the leading '@' / '>' characters up to the first blank, '/' or TAB of the header line"""
    line = record.split(b"\n", 1)[0] + b"\n"
    p1 = next((i for i in range(1, len(line)) if line[i:i + 1] not in (b">", b"@")), len(line) - 1)
    p2 = next((i for i in range(1, len(line)) if line[i:i + 1] in (b" ", b"/", b"\t")), len(line) - 1)
    return line[p1:p2] if p2 > p1 else b""


def unmapped_reads(names, sam_text: bytes, paired: bool):
    """for every read, in input order: does the SAM text hold a record of it with FLAG & 4.  The records of a read follow each other (-m: several); of a
    pair, mate 1's come first; a read whose next record carries another name (or, in a pair, the other mate's bit) has none"""
    lines = [ln.split(b"\t") for ln in sam_text.split(b"\n") if ln and not ln.startswith(b"@")]
    out, at = [], 0
    for i, name in enumerate(names):
        mate = (0x40 if i % 2 == 0 else 0x80) if paired else 0
        hit = False
        while at < len(lines) and lines[at][0] == name and (int(lines[at][1]) & 0xC0) == mate:
            hit = hit or bool(int(lines[at][1]) & 4)
            at += 1
        out.append(hit)
    assert at == len(lines), "record %d of the SAM text belongs to no read in input order" % at
    return out


def expected(texts, sam_text: bytes, paired: bool, two_files: bool, fasta: bool = False):
    """the (-un, -un2) bytes of one library: texts = [file] or [file 1, file 2]"""
    recs = [records(t, fasta) for t in texts]
    order = [r for pair in zip(*recs) for r in pair] if two_files else recs[0]
    un = unmapped_reads([name_of(r) for r in order], sam_text, paired)
    step = 2 if paired else 1
    out = [b"", b""]
    for u in range(0, len(order) - step + 1, step):
        if all(un[u:u + step]):
            for t in range(step):
                out[t if two_files else 0] += order[u + t]
    return out[0], out[1]
