"""GPU: BGZF blocks compressed on the device (kart_amd/csrc/bgzf_kernels.hip, kernels/bgzf_block.inc) -- kg_bgzf_deflate on the inputs at which each
of its paths can go wrong, the stream's format "bgzf", and the product's -bo -bz device against -bo.  Every member is read by a strict reader written
from SAMv1 4.1 and RFC 1951 / 1952 (zlib's raw inflate does the decoding): the device's bytes are its own, the inflated stream must be the input's."""
import gzip
import heapq
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

from bam_encode import bam_records_of_text, ref_ids_of_header
from conftest import GOLDEN, ROOT, SMALL_PREFIX
from test_bam_stream_gpu import BGZF_EOF, edge_batch, fastq, pair_at

pytestmark = pytest.mark.gpu
KART_AMD = os.path.join(ROOT, "kart_amd", "bin", "kart-amd")
PAYLOAD = 0xff00
HEAD = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0]) + b"BC" + bytes([2, 0])      # bgzf_append_block's head[]


def read_members(data: bytes):
    """-> [(payload, member size)] of a series of BGZF blocks, every member checked: the 16 fixed bytes, BSIZE, a deflate stream that ends exactly
    where the trailer begins, CRC-32, ISIZE, at most 64 KiB in all"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 16] == HEAD, (at, data[at:at + 18].hex())
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert 18 + 8 < size <= 65536 and at + size <= len(data), (at, size)
        d = zlib.decompressobj(-15)
        raw = d.decompress(data[at + 18:at + size - 8])
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", (at, len(d.unused_data))
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        assert crc == zlib.crc32(raw) and isize == len(raw) <= PAYLOAD, (at, crc, zlib.crc32(raw), isize, len(raw))
        out.append((raw, size))
        at += size
    return out


def check_blocks(src: bytes, cuts, bgzf: bytes, block_src, block_off):
    """the blocks hold src cut at least at `cuts`, nothing else"""
    members = read_members(bgzf)
    assert len(members) == len(block_src) - 1 == len(block_off) - 1
    assert block_src[0] == 0 and block_src[-1] == len(src) and block_off[0] == 0 and block_off[-1] == len(bgzf)
    at = 0
    for i, (raw, size) in enumerate(members):
        assert (block_off[i], block_off[i + 1]) == (at, at + size)
        assert 0 < block_src[i + 1] - block_src[i] <= PAYLOAD                      # (an empty range makes no block)
        assert raw == src[block_src[i]:block_src[i + 1]], i
        at += size
    # no block straddles a cut: every cut is a block boundary; and no finer than needed: a range of n bytes makes ceil(n / 0xff00) blocks
    bounds = set(int(v) for v in block_src)
    assert all(int(c) in bounds for c in cuts)
    assert len(members) == sum((int(b) - int(a) + PAYLOAD - 1) // PAYLOAD for a, b in zip(cuts[:-1], cuts[1:]))
    return members


def zlib_members_bytes(payloads, strategy):
    total = 0
    for p in payloads:
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
        total += 18 + len(c.compress(p) + c.flush()) + 8
    return total


def huffman_depth(counts):
    """depth of a Huffman code over `counts` without a length limit"""
    heap = [(c, 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def fibonacci_block():
    fib = [1, 2]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    data = bytearray()
    for k, f in enumerate(fib):
        data += bytes([k + 1]) * f
    data = list(data)
    random.Random(20).shuffle(data)
    assert len(data) == 28655
    # (CPU check) the literals and the end-of-block symbol alone need 20 bits: the block cannot be coded without the 15-bit limit at work
    assert huffman_depth(fib + [1]) == 20
    return bytes(data)


@pytest.fixture(scope="module")
def bam_records():
    text = gzip.open(os.path.join(GOLDEN, "sam", "pe.sam.gz")).read()
    raw = bam_records_of_text(text, ref_ids_of_header(text.decode()))
    assert len(raw) == 2679356
    return raw


@pytest.fixture(scope="module")
def cases(bam_records):
    """[(name, bytes)]: the ranges of the one call, in order"""
    rng = random.Random(11)
    out = []
    lengths = (0, 1, 2, 3, 4, 257, 258, 259, 260, PAYLOAD - 1, PAYLOAD, PAYLOAD + 1, 2 * PAYLOAD + 7)
    for n in lengths:
        out.append(("random%d" % n, rng.randbytes(n)))
        out.append(("run%d" % n, bytes([rng.randrange(256)]) * n))           # distance 1, chains of length-258 matches, one distance code
    out.append(("range200", bytes(range(200))))                               # no match at all: an empty distance tree
    out.append(("stored65280", rng.randbytes(65280)))                         # the stored block, at the BSIZE limit
    out.append(("pattern40", rng.randbytes(40) * 300))
    same = rng.randbytes(300)
    out.append(("apart32768", same + rng.randbytes(32768 - 300) + same + rng.randbytes(64)))      # the furthest distance there is
    out.append(("apart32769", same + rng.randbytes(32769 - 300) + same + rng.randbytes(64)))      # ... and one beyond it
    out.append(("fibonacci", fibonacci_block()))
    for at in range(0, len(bam_records), PAYLOAD):
        out.append(("bam%d" % at, bam_records[at:at + PAYLOAD]))
    # ... and short ranges of records up to about 600 ranges: more blocks than the device has CUs, ranges that end anywhere
    while len(out) < 600:
        at, n = rng.randrange(len(bam_records) - 4000), rng.choice((5, 37, 300, 1000, 2999, 4000))
        out.append(("piece%d" % len(out), bam_records[at:at + n]))
    return out


@pytest.fixture(scope="module")
def deflated(built_lib, cases):
    """the one call: (src, cuts, bgzf, block_src, block_off)"""
    from kart_amd import api
    if api.device_count() <= 0:
        pytest.fail("no HIP device visible: -m gpu tests must run on the GPU box (there is no CPU fallback)")
    src = b"".join(b for _, b in cases)
    cuts = np.cumsum([0] + [len(b) for _, b in cases]).astype(np.int64)
    bgzf, block_src, block_off = api.bgzf_deflate(src, cuts)
    return src, cuts, bgzf, block_src, block_off


def blocks_of(deflated, cases, which, prefix=False):
    """the members (payload, size) of the range named `which` (prefix: of every range whose name starts with it)"""
    src, cuts, bgzf, block_src, block_off = deflated
    got = []
    for k, (name, _) in enumerate(cases):
        if not (name.startswith(which) if prefix else name == which):
            continue
        lo, hi = np.searchsorted(block_src, cuts[k]), np.searchsorted(block_src, cuts[k + 1])
        got += read_members(bgzf[block_off[lo]:block_off[hi]])
    return got


def test_every_member_reads_back(deflated, cases):
    src, cuts, bgzf, block_src, block_off = deflated
    members = check_blocks(src, cuts, bgzf, block_src, block_off)
    assert len(members) > 600
    assert max(size for _, size in members) <= 65536
    # the ranges of the list come back one by one
    for name in ("random0", "run0"):
        assert blocks_of(deflated, cases, name) == []
    for name, data in cases:
        if not name.startswith(("bam", "piece")):
            got = blocks_of(deflated, cases, name)
            assert b"".join(p for p, _ in got) == data and len(got) == (len(data) + PAYLOAD - 1) // PAYLOAD, name
    stored = blocks_of(deflated, cases, "stored65280")
    assert [size for _, size in stored] == [65280 + 5 + 26]          # stored: payload + 5, header and trailer -- inside BSIZE
    assert sum(size for _, size in blocks_of(deflated, cases, "pattern40")) < 600
    # (a run is 254 matches of length 258 at distance 1: two codes in use beside the literal and the end, a few bits each, behind ~110 bytes of tables)
    assert [size < 400 for _, size in blocks_of(deflated, cases, "run%d" % PAYLOAD)] == [True]
    # random bytes do not compress, so a block of them is stored (payload + 31 bytes) unless the repeated 300 bytes are found: the match at distance
    # 32768 is, the one at 32769 is out of reach
    near, far = blocks_of(deflated, cases, "apart32768"), blocks_of(deflated, cases, "apart32769")
    assert near[0][1] < len(near[0][0]) + 31 and far[0][1] == len(far[0][0]) + 31


def test_second_call_gives_the_same_bytes(deflated):
    from kart_amd import api
    src, cuts, bgzf, block_src, block_off = deflated
    again, src2, off2 = api.bgzf_deflate(src, cuts)
    assert again == bgzf and (src2 == block_src).all() and (off2 == block_off).all()


def test_matches_and_code_tables_are_at_work(deflated, cases, bam_records):
    """the records compress below what Huffman coding alone reaches (no matches: fails), the Fibonacci block below the fixed tables (no real
    code tables: fails); both bounds hold with margin for zlib's own level 1 (674 543 / 12 356 bytes against 1 207 107 / 14 958)"""
    payloads = [bam_records[at:at + PAYLOAD] for at in range(0, len(bam_records), PAYLOAD)]
    got = sum(size for _, size in blocks_of(deflated, cases, "bam", prefix=True))
    bound = zlib_members_bytes(payloads, zlib.Z_HUFFMAN_ONLY)
    print("BAM records: device %d bytes, zlib Z_HUFFMAN_ONLY %d" % (got, bound))
    assert got < bound
    fib = [b for n, b in cases if n == "fibonacci"]
    got = sum(size for _, size in blocks_of(deflated, cases, "fibonacci"))
    bound = zlib_members_bytes(fib, zlib.Z_FIXED)
    print("Fibonacci block: device %d bytes, zlib Z_FIXED %d" % (got, bound))
    assert got < bound


def test_bad_cuts_and_short_buffers_are_errors(built_lib):
    from kart_amd import api
    data = bytes(range(256)) * 1000
    for cuts in ([1, len(data)], [0, len(data) - 1], [0, 700, 600, len(data)], [0, len(data), len(data) + 1]):
        with pytest.raises(api.KartAmdError, match="status 3"):
            api.bgzf_deflate(data, cuts)
    with pytest.raises(api.KartAmdError, match=r"status 4.*take \d+ bytes"):
        api.bgzf_deflate(data, [0, len(data)], dst_capacity=1000)
    with pytest.raises(api.KartAmdError, match="status 4.*make 5 blocks"):
        api.bgzf_deflate(data, [0, 100, len(data)], max_blocks=4)
    bgzf, block_src, _ = api.bgzf_deflate(data, [0, 0, 100, 100, len(data)])
    assert list(block_src) == [0, 100, 100 + PAYLOAD, 100 + 2 * PAYLOAD, 100 + 3 * PAYLOAD, len(data)]
    assert b"".join(p for p, _ in read_members(bgzf)) == data
    assert api.bgzf_deflate(b"", [0])[0] == b""


# ---- the stream ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome():
    from kart_amd.index_build import read_fasta
    return {n: s for n, _, s in read_fasta(os.path.join(GOLDEN, "small.fa"))}


def test_stream_format_bgzf(gpu_index_full, genome):
    from kart_amd import api, synth
    recs = edge_batch(genome)
    g = genome["chrA"]
    long1, long2 = bytes(g[6000:10100]), bytes(synth.revcomp(g[10300:10450]))          # a read above 4000 bases is handed back (align_plan.hip)
    at = 2 * 37
    recs = recs[:at] + [(b"long4100", long1, b"I" * len(long1)), (b"long4100", long2, b"5" * len(long2))] + recs[at:]
    text, n = fastq(recs), len(recs)
    stream = api.Stream(gpu_index_full, max_reads=16000, max_window=8 << 20, lanes=1)
    try:
        def run(fmt):
            stream.set_format(fmt)
            p = stream.parse(text, None, paired=True, chunk_reads=8, want_reads=(n + 7) // 8 * 8)
            assert (p.n_reads, p.stop, p.done) == (n, 0, 1)
            return stream.map()
        sam, host_sam = run("sam")
        assert stream.last_blocks is None
        bam, host_bam = run("bam")
        assert stream.last_blocks is None
        got, host = run("bgzf")
        blocks = stream.last_blocks
        assert run("bam") == (bam, host_bam) and stream.last_blocks is None
        assert run("sam") == (sam, host_sam) and stream.last_blocks is None
    finally:
        stream.close()
    assert got == bam and host == host_bam == host_sam
    assert len(host) >= 1 and at in host, host
    raw = b"".join(got)
    off = np.cumsum([0] + [len(r) for r in got])
    bgzf, block_src, block_off = blocks
    cuts = sorted(set([int(off[r]) for r in range(0, n, 8)] + [int(off[r]) for r in host] + [0, len(raw)]))
    members = read_members(bgzf)
    assert len(members) == len(block_src) - 1 and block_src[0] == 0 and block_src[-1] == len(raw) and block_off[-1] == len(bgzf)
    for i, (payload, size) in enumerate(members):
        assert payload == raw[block_src[i]:block_src[i + 1]] and size == block_off[i + 1] - block_off[i]
    assert set(cuts) <= set(int(v) for v in block_src)
    assert len(members) == sum((b - a + PAYLOAD - 1) // PAYLOAD for a, b in zip(cuts[:-1], cuts[1:]))


# ---- the product -----------------------------------------------------------------------------------------------------------------
def _golden(name, tmp_path):
    dst = str(tmp_path / name)
    with gzip.open(os.path.join(GOLDEN, "sam", name + ".gz")) as fi, open(dst, "wb") as fo:
        fo.write(fi.read())
    return dst


def _cli_start(args, out, env=None):
    return subprocess.Popen([KART_AMD, "-silent", "-i", SMALL_PREFIX, "-t", "8"] + args + ["-bo", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                            env=dict(os.environ, KART_AMD_VERBOSE="1", KART_AMD_UNSET_FLAG="0", **(env or {}))), out


def _cli_end(started):
    """-> (report, file) of a run begun with _cli_start"""
    proc, out = started
    try:
        report = proc.communicate(timeout=120)[0].decode()
    except subprocess.TimeoutExpired:
        proc.kill()
        raise
    assert proc.returncode == 0, report[-600:]
    return report, open(out, "rb").read()


def _cli(args, out, env=None):
    return _cli_end(_cli_start(args, out, env))


def _deflate_line(report):
    line = [l for l in report.splitlines() if l.startswith("device deflate:")]
    assert len(line) == 1, report[-600:]
    w = line[0].split()
    return int(w[2]), int(w[4])


@pytest.mark.parametrize("case", ["plain", "m", "gz", "fa"])
def test_product_bz_device(case, built_lib, tmp_path):
    """-bo x -bz device and -bo y, each from a fresh process: both files are sound BGZF, inflate to the same bytes, and y is still the file of the
    host's own reader, printer and encoder (KART_AMD_NO_STREAM=1) byte for byte"""
    f1, f2 = _golden("pe_1.fq", tmp_path), _golden("pe_2.fq", tmp_path)
    if case == "gz":
        for f in (f1, f2):
            with open(f, "rb") as fi, gzip.open(f + ".gz", "wb", compresslevel=6) as fo:
                fo.write(fi.read())
        f1, f2 = f1 + ".gz", f2 + ".gz"
    if case == "fa":
        for f in (f1, f2):
            lines = open(f, "rb").read().split(b"\n")
            with open(f[:-3] + ".fa", "wb") as fo:
                for i in range(0, len(lines) - 3, 4):
                    fo.write(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n")
        f1, f2 = f1[:-3] + ".fa", f2[:-3] + ".fa"
    args = ["-f", f1, "-f2", f2] + (["-m"] if case == "m" else [])
    # (three fresh processes, side by side: most of a run this small is the start of the process)
    started = [_cli_start(args + ["-bz", "device"], str(tmp_path / "x.bam")), _cli_start(args, str(tmp_path / "y.bam")),
               _cli_start(args, str(tmp_path / "h.bam"), {"KART_AMD_NO_STREAM": "1"})]
    (rep_x, x), (rep_y, y), (rep_h, h) = [_cli_end(p) for p in started]
    assert "device stream:" in rep_x and "device stream:" in rep_y and "device stream:" not in rep_h
    read_members(x)
    read_members(y)
    assert gzip.open(str(tmp_path / "x.bam")).read() == gzip.open(str(tmp_path / "y.bam")).read()
    assert x[-28:] == BGZF_EOF and y[-28:] == BGZF_EOF and len(x) > 100000
    dev, total = _deflate_line(rep_x)
    assert 0 < dev <= total <= len(x), (dev, total, len(x))
    assert _deflate_line(rep_y)[0] == 0
    assert y == h                                        # the default path has not moved


def test_session_resets_the_format_per_run(built_lib, tmp_path):
    from kart_amd import api
    f1, f2 = _golden("pe_1.fq", tmp_path), _golden("pe_2.fq", tmp_path)
    _, host_file = _cli(["-f", f1, "-f2", f2], str(tmp_path / "cli.bam"))
    a, b, c = str(tmp_path / "a.bam"), str(tmp_path / "b.sam"), str(tmp_path / "c.bam")
    sess = api.HostSession(SMALL_PREFIX, 0, 8)
    try:
        st_a = sess.map(["-f", f1, "-f2", f2, "-bo", a, "-bz", "device"])
        st_b = sess.map(["-f", f1, "-f2", f2, "-o", b])
        st_c = sess.map(["-f", f1, "-f2", f2, "-bo", c])
    finally:
        sess.close()
    assert st_a.bgzf_device_bytes > 0 and st_a.bgzf_device_bytes + st_a.bgzf_host_bytes <= os.path.getsize(a)
    assert st_b.bgzf_device_bytes == 0 and st_b.bgzf_host_bytes == 0
    assert st_c.bgzf_device_bytes == 0 and st_c.bgzf_host_bytes > 0
    read_members(open(a, "rb").read())
    assert open(b, "rb").read() == gzip.open(os.path.join(GOLDEN, "sam", "pe.sam.gz")).read()
    assert open(c, "rb").read() == host_file
    assert gzip.open(a).read() == gzip.open(c).read()
