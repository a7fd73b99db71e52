"""The reference's two FASTA readers in a few lines of Python -- the yardstick of tests/test_fasta_reads_cpu.py (the host pipeline) and
tests/test_fasta_stream_gpu.py (the device stream's fa_* kernels).  Written from the reference's reader (src/GetData.cpp), not from either of them.

GetNextEntry with FastQFormat == false (:51-107): the first line of an entry is its header, whatever it starts with; every further line up to the
next one whose first byte is '>' is appended to the sequence without its last byte (taken to be the newline, so a last line without one loses its
last base, the '\\r' of CR LF stays, a blank line adds nothing).  gzGetNextEntry (:145-182): exactly one sequence line per entry, read through
gzgets() with a 1000-byte buffer; an entry whose first line does not start with '@' or '>', or that names nothing, is empty.
GetNextChunk (:109-143): an empty read ends a chunk early, a chunk without reads ends the library."""


def comp(c):    # GetComplementaryBase, src/tools.cpp:3-17
    return {65: 84, 97: 84, 67: 71, 99: 71, 71: 67, 103: 67, 84: 65, 116: 65}.get(c, 78)


def held(seq: bytes, flip: bool) -> bytes:
    """the read as the reference holds it: mate 2 of a pair reverse-complemented (src/GetData.cpp:125-129)"""
    return bytes(comp(c) for c in reversed(seq)) if flip else seq


def lines_of(text: bytes):
    """getline(): every line with its newline; the last one as it is"""
    out = text.split(b"\n")
    last = out.pop()
    out = [l + b"\n" for l in out]
    return out + ([last] if last else [])


def name_of(h: bytes) -> bytes:   # IdentifyHeaderBegPos / IdentifyHeaderEndPos, src/GetData.cpp:29-49
    p1 = p2 = len(h) - 1
    for k in range(1, len(h)):
        if h[k] not in b">@":
            p1 = k
            break
    for k in range(1, len(h)):
        if h[k] in b" /\t":
            p2 = k
            break
    return h[p1:p2] if p2 > p1 else b""


def fasta_reads(text: bytes):
    """GetNextEntry over a whole plain file: [(name, sequence)]"""
    lines, out, i = lines_of(text), [], 0
    while i < len(lines):
        name, seq = name_of(lines[i]), b""
        i += 1
        while i < len(lines) and lines[i][:1] != b">":
            seq += lines[i][:-1].split(b"\0")[0]          # (a line is a C string)
            i += 1
        out.append((name, seq))
    return out


def gz_pieces(text: bytes, buf: int = 1000):
    """what successive gzgets() calls return: at most buf - 1 bytes, up to and including a newline"""
    out = []
    for l in lines_of(text):
        out += [l[k:k + buf - 1] for k in range(0, len(l), buf - 1)]
    return out


def fasta_reads_gz(text: bytes):
    """gzGetNextEntry over the whole inflated text: [(name, sequence)]"""
    pieces, out, i = gz_pieces(text), [], 0
    while i < len(pieces):
        h = pieces[i]
        i += 1
        name = name_of(h)
        if not name or h[:1] not in (b"@", b">"):
            out.append((b"", b""))
            continue
        s = pieces[i] if i < len(pieces) else h            # (the buffer keeps the last line that did arrive)
        i += 1
        out.append((name, s[:max(0, len(s) - 1)]))
    return out


def reads_mapped(reads, limit=4000):
    """GetNextChunk over the entries: an empty read ends its chunk early (and is dropped); the library ends with the first chunk that comes back empty"""
    out, i = [], 0
    while True:
        count = 0
        while i < len(reads) and count < limit:
            r = reads[i]
            i += 1
            if not r[1]:
                break
            out.append(r)
            count += 1
        if count == 0:
            return out


def wrap(seq: bytes, cols: int, eol: bytes = b"\n") -> bytes:
    return b"".join(seq[k:k + cols] + eol for k in range(0, len(seq), cols))


def fasta_text(recs, cols=None, eol=b"\n") -> bytes:
    """[(header without '>', sequence)] as FASTA: one sequence line per record, or wrapped at `cols` columns"""
    return b"".join(b">" + n + eol + (wrap(s, cols, eol) if cols else s + eol) for n, s in recs)
