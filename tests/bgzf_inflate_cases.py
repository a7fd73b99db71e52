"""BGZF members for the tests of the device's inflater (kernels/bgzf_inflate.inc): sound ones of every block shape zlib can be made to write, a
hand-assembled one with a 15-bit code, a mixed file, and that file with one member damaged in the ways a file can be damaged.  What Python's zlib
(plus gzip's CRC-32 / ISIZE check) says of a member is the yardstick: accepts()."""
import random
import struct
import zlib

PAYLOAD = 0xff00
OK, HEADER, STREAM, SIZE, CRC = 0, 1, 2, 3, 4


def wrap(body: bytes, crc: int, isize: int) -> bytes:
    """a BGZF member around a raw deflate stream"""
    bsize = 12 + 6 + len(body) + 8
    assert bsize <= 65536
    hdr = b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return hdr + body + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def member(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_at=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if flush_at is None:
        body = c.compress(data) + c.flush()
    else:
        body = c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()
    return wrap(body, zlib.crc32(data), len(data))


def split(data: bytes):
    """[(member, isize field)] along BSIZE"""
    out, at = [], 0
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(data[at:at + size])
        at += size
    assert at == len(data)
    return out


def isize_of(m: bytes) -> int:
    return struct.unpack_from("<I", m, len(m) - 4)[0]


def accepts(m: bytes):
    """what zlib and the trailer say of a member: (good, text)"""
    xlen = struct.unpack_from("<H", m, 10)[0]
    body = m[12 + xlen:len(m) - 8]
    crc, isize = struct.unpack_from("<II", m, len(m) - 8)
    d = zlib.decompressobj(-15)
    try:
        raw = d.decompress(body)
    except zlib.error:
        return False, b""
    good = d.eof and d.unused_data == b"" and len(raw) == isize and zlib.crc32(raw) == crc
    return good, raw


def fastq(n_bytes: int, seed: int) -> bytes:
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        seq = "".join(rng.choice("ACGT") for _ in range(rng.randint(90, 151)))
        qual = "".join(rng.choice("FFFFFFFF:,#") for _ in seq)
        rec = "@SYN.%d %d/1\n%s\n+\n%s\n" % (seed * 1000000 + i, i, seq, qual)
        out.append(rec); size += len(rec); i += 1
    return "".join(out).encode()[:n_bytes]


class Bits:
    """an LSB-first bit writer; Huffman codes go in from their most significant bit (RFC 1951 3.1.1)"""
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> i) & 1 for i in range(n)]

    def code(self, value, n):
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def canonical(lens):
    """{symbol: (code, length)} of RFC 1951 3.2.2"""
    count = [0] * 16
    for n in lens.values():
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s in sorted(lens):
        if lens[s]:
            out[s] = (nxt[lens[s]], lens[s]); nxt[lens[s]] += 1
    return out


def dynamic_header(w: Bits, lit_lens: dict, dist_lens: dict, nlit: int, ndist: int, final=1, cl_lens=None):
    """a dynamic block's header: every code length sent as it is, through a code-length code of sixteen 4-bit codes (cl_lens: another one)"""
    w.put(final, 1); w.put(2, 2)
    w.put(nlit - 257, 5); w.put(ndist - 1, 5); w.put(19 - 4, 4)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = cl_lens if cl_lens is not None else {s: 4 for s in range(16)}
    for s in order:
        w.put(cl.get(s, 0), 3)
    codes = canonical(cl) if cl_lens is None else {}
    if cl_lens is None:
        for s in range(nlit):
            w.code(*codes[lit_lens.get(s, 0)])
        for s in range(ndist):
            w.code(*codes[dist_lens.get(s, 0)])


def fifteen_bit_member():
    """code lengths 1, 2, ... 14, 15, 15 over sixteen literal/length symbols (fourteen letters, end-of-block, length 3); one distance code of one bit"""
    lit_lens = {65 + i: 1 + i for i in range(14)}
    lit_lens[256] = 15; lit_lens[257] = 15
    w = Bits()
    dynamic_header(w, lit_lens, {0: 1}, 258, 1)
    codes = canonical(lit_lens)
    text = bytes(range(65, 79)) * 3
    for b in text:
        w.code(*codes[b])
    w.code(*codes[257]); w.code(0, 1)          # three more of the last byte: length 3 at distance 1
    w.code(*codes[256])
    text += text[-1:] * 3
    return text, wrap(w.bytes(), zlib.crc32(text), len(text))


def sound_cases():
    """[(name, text, member)]"""
    fq = fastq(PAYLOAD, 1)
    rng = random.Random(7)
    out = []
    for level in (1, 6, 9):
        out.append(("fastq_level%d" % level, fq, member(fq, level)))
    out.append(("fastq_stored", fq, member(fq, 0)))
    rnd = rng.randbytes(PAYLOAD)
    out.append(("random", rnd, member(rnd)))
    out.append(("fastq_fixed", fq, member(fq, 6, zlib.Z_FIXED)))
    for tiny in (b"", b"A", b"ACGT\n"):
        out.append(("tiny%d" % len(tiny), tiny, member(tiny)))
    out.append(("fastq_many_blocks", fq, member(fq, 6, mem_level=1)))
    out.append(("fastq_huffman_only", fq, member(fq, 6, zlib.Z_HUFFMAN_ONLY)))
    out.append(("fastq_rle", fq, member(fq, 6, zlib.Z_RLE)))
    out.append(("fastq_flushed", fq, member(fq, 6, flush_at=30000)))
    run = b"z" * PAYLOAD
    out.append(("run", run, member(run)))
    fq64 = fastq(65536, 2)
    out.append(("fastq_65536", fq64, member(fq64)))
    text, m = fifteen_bit_member()
    out.append(("fifteen_bits", text, m))
    return out


def mixed_file(seed=11, n_bytes=300 * PAYLOAD // 2):
    """about 300 members of 1 .. 0xff00 bytes of FASTQ, an empty member in the middle, the EOF block at the end: ([text], [member])"""
    rng = random.Random(seed)
    data = fastq(200000, 3) * (n_bytes // 200000 + 1)
    texts, at = [], 0
    while at < n_bytes:
        n = rng.randint(1, PAYLOAD)
        texts.append(data[at:at + n]); at += n
    texts.insert(len(texts) // 2, b"")
    texts.append(b"")
    return texts, [member(t) for t in texts]


def damaged_cases(texts, members, victim, seed=5):
    """[(name, member)]: members[victim] damaged; its trailer still names the sound text, save where the trailer is what is damaged"""
    m, text = members[victim], texts[victim]
    body, crc, isize = m[18:-8], zlib.crc32(text), len(text)
    rng = random.Random(seed)
    out = []
    flip = bytearray(body)
    at = rng.randrange(len(body) // 4, len(body) - 16)
    flip[at] ^= 1 << rng.randrange(8)
    out.append(("data_bit", wrap(bytes(flip), crc, isize)))
    out.append(("crc_bit", wrap(body, crc ^ (1 << 13), isize)))
    out.append(("isize_plus", wrap(body, crc, isize + 1)))
    out.append(("isize_minus", wrap(body, crc, isize - 1)))
    out.append(("cut1", wrap(body[:-1], crc, isize)))
    out.append(("cut9", wrap(body[:-9], crc, isize)))
    out.append(("type3", wrap(b"\x07" + body[1:], crc, isize)))
    stored = text[:1000]
    out.append(("nlen", wrap(b"\x01" + struct.pack("<HH", len(stored), (len(stored) ^ 0xffff) ^ 0x10) + stored, zlib.crc32(stored), len(stored))))
    w = Bits()
    w.put(1, 1); w.put(1, 2); w.code(1, 7); w.code(0, 5); w.code(0, 7)          # fixed: length 3 at distance 1, end of block
    out.append(("before_start", wrap(w.bytes(), zlib.crc32(b"AAA"), 3)))
    w = Bits()
    dynamic_header(w, {}, {}, 257, 1, cl_lens={0: 1, 1: 1, 2: 1, 3: 1})
    out.append(("oversubscribed", wrap(w.bytes() + body[:100], crc, isize)))
    w = Bits()
    dynamic_header(w, {256: 1, 286: 1}, {0: 1}, 287, 1)
    w.code(1, 1); w.code(0, 1); w.code(0, 1)                                     # symbol 286, a distance, end of block
    out.append(("symbol286", wrap(w.bytes(), zlib.crc32(b""), 0)))
    # symbols that have a code and no meaning can only come out of a fixed block (a dynamic one may not name them, as above)
    w = Bits()
    w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(0xc0 + 6, 8); w.code(0, 5); w.code(0, 7)      # 'A', symbol 286, a distance, end of block
    out.append(("fixed_symbol286", wrap(w.bytes(), zlib.crc32(b"A"), 1)))
    w = Bits()
    w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(1, 7); w.code(30, 5); w.code(0, 7)             # 'A', length 3 at distance symbol 30
    out.append(("fixed_distance30", wrap(w.bytes(), zlib.crc32(b"AAAA"), 4)))
    w = Bits()
    dynamic_header(w, {65: 2, 256: 2}, {0: 1}, 257, 1)                                                     # two codes of two bits: incomplete
    w.code(0, 2); w.code(1, 2)
    out.append(("incomplete_literal", wrap(w.bytes(), zlib.crc32(b"A"), 1)))
    w = Bits()
    dynamic_header(w, {65: 1, 256: 2, 257: 2}, {0: 2, 1: 2}, 258, 2)                                       # the distance code is incomplete, and not used
    w.code(0, 1); w.code(2, 2)
    out.append(("incomplete_distance", wrap(w.bytes(), zlib.crc32(b"A"), 1)))
    out.append(("all_ones", wrap(b"\xff" * 200, crc, isize)))
    return out
