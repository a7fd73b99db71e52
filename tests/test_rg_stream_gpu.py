"""GPU: the read group made on the device (kg_stream_set_read_group; the kRg instantiations of sam_size / sam_format / bam_size / bam_format in
kart_amd/csrc/sam_kernels.hip and bam_kernels.hip).  The field is a constant of the batch, so the check needs no model: every line of a run with it is the line of the run
without it plus "\\tRG:Z:<ID>", on unmapped records, 1- and 2-base reads, chained records of multi_hit reads and records that take the record-by-record path
alike; a BAM record is what the host's encoder makes of that line.  ID lengths sit on either side of the widths the copies use (16-byte pieces, 64 lanes)."""
import gzip

import pytest

from bam_encode import bam_record
from test_bam_stream_gpu import fastq, genome, ref_ids  # noqa: F401  (fixtures and builders of the BAM stream test)
from test_md_stream_gpu import MD_LDS, edge_batch, fields_of, md_field, multi_hit_batch

pytestmark = pytest.mark.gpu
ALL = [(f, m) for f in ("sam", "bam") for m in (False, True)]
NO_MD = [("sam", False), ("bam", False)]


def rg_id(n):
    """n bytes that walk through every accepted character ('!'..'~'), colons and '@' among them"""
    return bytes(33 + (7 * i + n) % 94 for i in range(n))


@pytest.fixture(scope="module")
def stream(gpu_index_full):
    from kart_amd import api
    s = api.Stream(gpu_index_full, max_reads=16000, max_window=8 << 20, lanes=1)
    yield s
    s.close()


def bam_with_zs(text, ref_ids):
    """the BAM records of SAM lines whose last one or two optional fields are TAG:Z:value (tests/bam_encode.py encodes the integer fields)"""
    out = b""
    for ln in text.split(b"\n"):
        if ln.count(b"\t") < 10:
            continue
        f = ln.split(b"\t")
        z = b""
        while f[-1][2:5] == b":Z:":
            z = f[-1][:2] + b"Z" + f[-1][5:] + b"\0" + z
            f.pop()
        rec = bam_record(b"\t".join(f), ref_ids)
        size = int.from_bytes(rec[:4], "little") + len(z)
        out += size.to_bytes(4, "little") + rec[4:] + z
    return out


class Runner:
    """one batch through one stream: map(fmt, md, rg) -> (texts per read, reads handed back); the runs without a read group are kept, and every later
    one is held against the first"""

    def __init__(self, stream, text, n_reads, multi_hit=False, fasta=False, paired=True):
        self.s, self.text, self.n, self.multi_hit, self.fasta, self.paired = stream, text, n_reads, multi_hit, fasta, paired
        self.off = {}

    def map(self, fmt, md, rg):
        s = self.s
        s.set_input("fasta" if self.fasta else "fastq")
        s.set_format(fmt)
        s.set_tags(md=md)
        s.set_read_group(rg)
        p = s.parse(self.text, None, paired=self.paired, chunk_reads=8, want_reads=(self.n + 7) // 8 * 8)
        assert (p.n_reads, p.stop, p.done) == (self.n, 0, 1)
        return s.map(multi_hit=self.multi_hit)          # (a format error of the device -- ctl[1] != 0 -- fails the call)

    def off_on_off(self, fmt, md, rg):
        """-> (texts without, texts with, reads handed back); the run without the read group behind the run with it is the run before it"""
        try:
            first = self.off.setdefault((fmt, md), self.map(fmt, md, None))
            on = self.map(fmt, md, rg)
            again = self.map(fmt, md, None)
        finally:
            self.s.set_read_group(None)
            self.s.set_tags(md=False)
            self.s.set_format("sam")
            self.s.set_input("fastq")
        assert again == first, "the output without the read group changed after a run with it"
        assert on[1] == first[1], "another set of reads was handed back"
        return first[0], on[0], first[1]


def check(runner, rg, combos, ref_ids, max_host=None):
    """-> the SAM texts with the read group, by MD setting"""
    sam_on = {}
    hosts = set()
    for fmt, md in combos:
        off, on, host = runner.off_on_off(fmt, md, rg)
        hosts.add(tuple(host))
        assert len(off) == len(on) == runner.n and len(host) <= (runner.n // 2 if max_host is None else max_host)
        if fmt == "sam":
            sam_on[md] = on
            for i, (a, b) in enumerate(zip(off, on)):
                want = b"".join(ln + b"\tRG:Z:" + rg + b"\n" for ln in a.split(b"\n")[:-1])
                assert b == want, (i, a[:200], b[:200])
        else:
            # (the SAM run of the same MD setting came first: combos list it so)
            for i, (s, b) in enumerate(zip(sam_on[md], on)):
                assert b == bam_with_zs(s, ref_ids), (i, s[:300])
            for s, b in zip(runner.off["sam", md][0], off):
                assert b == bam_with_zs(s, ref_ids)
    assert len(hosts) == 1
    return sam_on


@pytest.fixture(scope="module")
def edge(stream, genome):
    recs = edge_batch(genome)
    return Runner(stream, fastq(recs), len(recs))


@pytest.mark.parametrize("n", [1, 17, 255])
def test_read_group_on_the_edge_batch_full_matrix(n, edge, ref_ids):
    sam_on = check(edge, rg_id(n), ALL, ref_ids)
    lines = fields_of(sam_on[True])
    # what the batch must hold (conditions on the input, read off the device's own lines)
    assert all(f[-1] == "RG:Z:" + rg_id(n).decode() for f in lines)
    assert any(f[2] == "*" for f in lines), "no unmapped record"
    assert any(f[2] != "*" for f in lines), "no mapped record"
    for k in (1, 2):
        assert any(len(f[9]) == k for f in lines), "no record of %d bases" % k
    assert any(f[2] != "*" and len(md_field(f[:-1]) or "") > MD_LDS for f in lines), "no device-made MD beyond the in-LDS limit"
    assert all(f[-2].startswith("MD:Z:") for f in lines if f[2] != "*") and all(f[-2] == "XS:i:0" for f in lines if f[2] == "*")


@pytest.mark.parametrize("n", [15, 16, 63, 64, 65])
def test_read_group_lengths_around_the_copy_widths(n, edge, ref_ids):
    check(edge, rg_id(n), NO_MD, ref_ids)


@pytest.mark.parametrize("n", [1, 17, 255])
def test_read_group_with_multi_hit(n, stream, genome, ref_ids):
    """-m: every record of a chain carries the field (the record-by-record path of both format kernels)"""
    recs = multi_hit_batch(genome)
    sam_on = check(Runner(stream, fastq(recs), len(recs), multi_hit=True), rg_id(n), ALL, ref_ids)
    for md in (False, True):
        chains = [t for t in sam_on[md] if t.count(b"\n") >= 2]
        assert chains, "no read with two or more records"
        assert all(ln.endswith(b"\tRG:Z:" + rg_id(n)) for t in chains for ln in t.split(b"\n") if ln)


def test_read_group_with_fasta_input(stream, genome, ref_ids):
    recs = edge_batch(genome)
    text = b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _ in recs)
    check(Runner(stream, text, len(recs), fasta=True), rg_id(17), ALL, ref_ids)


# ---- a small stream, a large tag: the tags outweigh the lines ----------------------------------------------------------------------------------------
SMALL_READS, SMALL_WINDOW = 256, 20 << 10


@pytest.fixture(scope="module")
def small_stream(gpu_index_full):
    from kart_amd import api
    s = api.Stream(gpu_index_full, max_reads=SMALL_READS, max_window=SMALL_WINDOW, lanes=1)
    yield s
    s.close()


def test_small_stream_large_tag(small_stream, genome, ref_ids):
    """256 reads of 30 bases and a 255-byte ID: 261 bytes of field on a line of some 110.  The stream's buffers as opened hold 2 * 20 KB + 64 (BAM: 144)
    bytes per read + 4 KB = 60 KB (BAM: 80 KB); the lines need 95 KB and the records 90 KB.  kg_stream_set_read_group allocates nothing: kg_stream_map,
    which knows the batch's size before its text is made, must have grown them"""
    g = genome["chrB"]
    recs = []
    for k in range(SMALL_READS // 2):
        name = b"s%03d" % k
        recs.append((name, bytes(g[3000 + 97 * k:3030 + 97 * k]), b"I" * 30))
        recs.append((name, bytes(g[3200 + 97 * k:3230 + 97 * k])[::-1], b"5" * 30))          # (reversed, not complemented: most of these stay unmapped)
    text = fastq(recs)
    assert len(text) <= SMALL_WINDOW
    rg = rg_id(255)
    sam_on = check(Runner(small_stream, text, len(recs)), rg, NO_MD, ref_ids, max_host=len(recs))
    assert sum(len(t) for t in sam_on[False]) > 2 * SMALL_WINDOW + 64 * SMALL_READS + 4096
    assert sum(len(bam_with_zs(t, ref_ids)) for t in sam_on[False]) > 2 * SMALL_WINDOW + 144 * SMALL_READS + 4096


CHAIN_READS, CHAIN_WINDOW = 40, 12 << 10


def chain_batch(genome):
    """36 single-end reads that each lie in all three copies of the repeat of the golden pe_m case (chrA 20261 / 20970 / 44046), either strand, one
    planted mismatch: with multi_hit every one of them carries a chain of three records"""
    from kart_amd import synth
    from test_md_stream_gpu import other_base
    g = genome["chrA"]
    recs = []
    for k in range(6):
        for base in (20260, 20969, 44045):
            for rev in (False, True):
                m = g[base:base + 150].copy()
                m[90] = other_base(m[90])
                m = synth.revcomp(m) if rev else m
                recs.append((b"chain%d_%d_%d" % (k, base, rev), bytes(m), b"!" * 75 + b"~" * 75))
    return recs


def test_small_stream_chains_grow_the_buffers_in_map(gpu_index_full, genome, ref_ids):
    """a stream of 40 reads and a batch of three-record chains: the chains multiply the field, so the batch needs more than the stream's buffers hold --
    2 * 12 KB + 4 KB + (64 + 32) * 40 = 32 KB for SAM lines with MD; kg_stream_set_read_group reserves nothing -- and kg_stream_map grows them; as BGZF
    blocks the larger size reaches the block tables too.  (The bounds asserted below add a field per read to that: the batch would outgrow even buffers
    that held one field for every read)"""
    from kart_amd import api
    recs = chain_batch(genome)
    text = fastq(recs)
    assert len(text) <= CHAIN_WINDOW and len(recs) <= CHAIN_READS
    rg = rg_id(255)
    small_stream = api.Stream(gpu_index_full, max_reads=CHAIN_READS, max_window=CHAIN_WINDOW, lanes=1)
    try:
        runner = Runner(small_stream, text, len(recs), multi_hit=True, paired=False)
        sam_on = check(runner, rg, ALL, ref_ids)
        # (conditions on the input: chains, and more bytes than the setters made room for, in either format)
        assert sum(t.count(b"\n") for t in sam_on[True]) >= 2 * len(recs)
        assert sum(len(t) for t in sam_on[True]) > 2 * CHAIN_WINDOW + 4096 + (64 + 32 + 6 + 255) * CHAIN_READS
        assert sum(len(bam_with_zs(t, ref_ids)) for t in sam_on[True]) > 2 * CHAIN_WINDOW + 4096 + (144 + 32 + 4 + 255) * CHAIN_READS
        bam, host = runner.map("bam", True, rg)
        got, host_z = runner.map("bgzf", True, rg)
        blocks = small_stream.last_blocks
    finally:
        small_stream.close()
    assert (got, host_z) == (bam, host) and blocks is not None
    assert gzip.decompress(blocks[0]) == b"".join(got)
    assert b"".join(got).count(b"RGZ" + rg + b"\0") == sum(t.count(b"\n") for t in sam_on[True])


# ---- the setter ------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_ids_are_rejected_and_the_earlier_one_stays(stream, edge):
    from kart_amd import api
    try:
        stream.set_read_group("kept")
        for bad in (b"", "", b"x" * 256, b"a\tb", "a b", b"a\nb", b"caf\xe9", b"\x7f", "caf\u00e9", "lane\u4e2d"):
            with pytest.raises(api.KartAmdError):
                stream.set_read_group(bad)
        # (Runner.map would set its own: the calls by hand)
        stream.set_format("sam")
        p = stream.parse(edge.text, None, paired=True, chunk_reads=8, want_reads=(edge.n + 7) // 8 * 8)
        assert p.n_reads == edge.n
        texts, host = stream.map()
        lines = [ln for t in texts for ln in t.split(b"\n") if ln]
        assert lines and all(ln.endswith(b"\tRG:Z:kept") for ln in lines)
        stream.set_read_group(None)
        p = stream.parse(edge.text, None, paired=True, chunk_reads=8, want_reads=(edge.n + 7) // 8 * 8)
        texts, host2 = stream.map()
        assert host2 == host and not any(b"RG:Z" in t for t in texts)
        # 255 bytes, str or bytes
        stream.set_read_group("y" * 255)
        stream.set_read_group(b"~" * 255)
    finally:
        stream.set_read_group(None)
        stream.set_format("sam")
