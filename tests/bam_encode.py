"""One printed SAM record -> one BAM record, written from the SAM/BAM specification v1 (section 4.2, bins 5.3) and from what an encoder that
parses the printed line sees of it.  The yardstick of the -bo tests: tests/test_bam_records_cpu.py holds the host's encoder to it, tests/
test_bam_stream_gpu.py the device's kernels.  Nothing here is taken from either of them.

What parsing the LINE (and not the record it was printed from) implies:
  * the columns are cut at tabs: a tab among the qualities ends the QUAL column there, and what follows is an optional field that is no TAG:i:value;
  * SEQ "*" is no sequence (l_seq 0); QUAL "*", or a QUAL column whose length is not l_seq, is l_seq bytes of 0xFF;
  * the records are cut at line feeds: a quality line shorter than its read brings its line feed along as its last quality (the reference cuts the
    line to the read's length, not at the line feed), the printed line breaks there, and the piece behind it -- fewer than 11 columns -- is no record;
  * l_read_name is one byte (name length + 1, cut), FLAG / bin / n_cigar_op are 16 bits, the positions and TLEN 32 bits;
  * an unmapped record's bin is reg2bin(-1, 0) = 4680;
  * TAG:i:value goes into the smallest integer type that holds the value, unsigned when it is not negative.
"""
import struct

NT16 = "=ACMGRSVTWYHKDBN"
CODE = [15] * 256
for _i, _c in enumerate(NT16):
    CODE[ord(_c)] = _i
    CODE[ord(_c.lower())] = _i
CIGAR_OPS = "MIDNSHP=X"


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def int_tag(tag: bytes, v: int) -> bytes:
    if v < 0:
        ty, fmt = (b"c", "<b") if v >= -128 else (b"s", "<h") if v >= -32768 else (b"i", "<i")
    else:
        ty, fmt = (b"C", "<B") if v < 256 else (b"S", "<H") if v < 65536 else (b"I", "<I")
    return tag + ty + struct.pack(fmt, v)


def ref_ids_of_header(header: str) -> dict:
    """contig name -> reference id, in @SQ order"""
    ids = {}
    for line in header.splitlines():
        if line.startswith("@SQ"):
            name = [f[3:] for f in line.split("\t") if f.startswith("SN:")][0]
            ids[name.encode()] = len(ids)
    return ids


def bam_record(line: bytes, ref_ids: dict) -> bytes:
    """`line`: one SAM record without its newline; ref_ids: contig name (bytes) -> reference id"""
    f = line.rstrip(b"\n").split(b"\t")
    assert len(f) >= 11, line[:80]
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    rid = -1 if rname == b"*" else ref_ids[rname]
    nid = rid if rnext == b"=" else -1 if rnext == b"*" else ref_ids[rnext]
    pos0, pnext0 = int(pos) - 1, int(pnext) - 1
    words, ref_len, num = [], 0, 0
    if cigar != b"*":
        for ch in cigar.decode():
            if ch.isdigit():
                num = num * 10 + int(ch)
                continue
            op = CIGAR_OPS.index(ch)
            words.append(num << 4 | op)
            if ch in "MDN=X":
                ref_len += num
            num = 0
    l_seq = 0 if seq == b"*" else len(seq)
    packed = bytearray((l_seq + 1) // 2)
    for i in range(l_seq):
        packed[i >> 1] |= CODE[seq[i]] << (0 if i & 1 else 4)
    if qual == b"*" or len(qual) != l_seq:
        quals = b"\xff" * l_seq
    else:
        quals = bytes((q - 33) & 255 for q in qual)
    tags = b""
    for opt in f[11:]:
        if len(opt) >= 6 and opt[2:5] == b":i:":
            tags += int_tag(opt[:2], int(opt[5:]))
    body = struct.pack("<iiBBHHHIiii", rid, pos0, (len(qname) + 1) & 255, int(mapq) & 255,
                       reg2bin(pos0, pos0 + (ref_len if ref_len > 0 else 1)) & 0xFFFF, len(words) & 0xFFFF, int(flag) & 0xFFFF, l_seq, nid, pnext0, int(tlen))
    body += qname + b"\0" + b"".join(struct.pack("<I", w) for w in words) + bytes(packed) + quals + tags
    return struct.pack("<I", len(body)) + body


def bam_records_of_text(text: bytes, ref_ids: dict) -> bytes:
    """printed SAM text -> its BAM records: a piece between two line feeds that has fewer than the 11 mandatory columns is no record and is dropped"""
    return b"".join(bam_record(l, ref_ids) for l in text.split(b"\n") if l.count(b"\t") >= 10)
