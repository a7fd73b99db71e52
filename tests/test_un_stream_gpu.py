"""GPU: the unmapped reads of a batch handed back by the device (kg_stream_set_unmapped; un_size_kernel / un_copy_kernel in kart_amd/csrc/un_kernels.hip).
The expectation needs no model of the mapper: the bytes of a unit are its records as they lie in the input (tests/un_plain.py), and which units are
selected is read off the SAM text of the SAME map() call -- a read is unmapped iff its record there has FLAG & 4, a pair is selected iff both mates are.
Unmapped reads are random sequence that shares no 13-mer with either strand of the genome (a seed is at least 13 bases: such a read has none); mapped
ones are exact pieces of the genome fixture."""
import numpy as np
import pytest

import un_plain
from test_bam_stream_gpu import fastq, genome, ref_ids  # noqa: F401  (fixtures and builders of the BAM stream test)
from test_md_stream_gpu import multi_hit_batch

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 150, 300)
PATTERNS = {
    "none": lambda u, n: False,
    "all": lambda u, n: True,
    "first": lambda u, n: u == 0,
    "last": lambda u, n: u == n - 1,
    "alternating": lambda u, n: u % 2 == 0,
    "one_per_64": lambda u, n: u % 64 == 37 % n,
}


@pytest.fixture(scope="module")
def stream(gpu_index_full):
    from kart_amd import api
    s = api.Stream(gpu_index_full, max_reads=16000, max_window=8 << 20, lanes=1)
    yield s
    s.close()


class Seedless:
    """random reads without a 13-mer of the genome, either strand: no seed, so no candidate, so the unmapped record"""

    def __init__(self, genome):
        from kart_amd import synth
        self.kmers = set()
        for g in genome.values():
            for strand in (g, synth.revcomp(g)):
                b = strand.tobytes().upper()
                self.kmers.update(b[i:i + 13] for i in range(len(b) - 12))
        self.rng = np.random.default_rng(20261020)

    def read(self, n):
        while True:
            r = np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, n)].tobytes()
            if not any(r[i:i + 13] in self.kmers for i in range(n - 12)):
                return r


@pytest.fixture(scope="module")
def seedless(genome):
    return Seedless(genome)


def name_of(u, k):
    """k bytes, 1..40; neighbours differ in their first byte"""
    s = b"%c%d" % (97 + u % 26, u)
    return (s + b"n" * k)[:k]


def build(genome, seedless, n_units, pattern, pairs):
    """-> (records [(name, seq, qual)] -- two per unit for pairs --, the units meant to stay unmapped)"""
    from kart_amd import synth
    g = genome["chrB"]
    recs, meant = [], []
    for u in range(n_units):
        name = name_of(u, 1 + (u * 7 + u // 40) % 40)
        un = PATTERNS[pattern](u, n_units)
        meant.append(un)
        for mate in range(2 if pairs else 1):
            if un:
                seq = seedless.read(LENGTHS[(u * 3 + u // 10 + mate) % len(LENGTHS)])
            else:
                length, p = 100 + (u * 13 + mate) % 51, 2000 + 211 * (u % 400)
                seq = bytes(g[p:p + length]) if mate == 0 else bytes(synth.revcomp(g[p + 400 - length:p + 400]))
            recs.append((name, seq, bytes(33 + (i * 5 + u) % 41 for i in range(len(seq)))))
    return recs, meant


def fastq_decorated(recs):
    """FASTQ with what a reader must leave alone: a comment behind the name, the name repeated on the '+' line, lower case"""
    out = b""
    for i, (n, s, q) in enumerate(recs):
        out += b"@" + n + (b" comment:%d/x" % i if i % 3 == 0 else b"") + b"\n" + (s.lower() if i % 5 == 4 else s) + b"\n+" + (n if i % 4 == 1 else b"") + b"\n" + q + b"\n"
    return out


def fasta(recs, width=None):
    out = b""
    for n, s, _ in recs:
        out += b">" + n + b"\n" + (s + b"\n" if not width else b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width)))
    return out


def run(stream, texts, n_reads, paired, fasta_in=False, gz_lines=0, multi_hit=False, fmt="sam", md=False, rg=None, unmapped=True):
    """one batch -> (SAM text per read, reads handed back, last_unmapped())"""
    try:
        stream.set_input("fasta" if fasta_in else "fastq")
        stream.set_format(fmt)
        stream.set_tags(md=md)
        stream.set_read_group(rg)
        stream.set_unmapped(unmapped)
        p = stream.parse(texts[0], texts[1] if len(texts) > 1 else None, paired=paired, chunk_reads=8, want_reads=(n_reads + 7) // 8 * 8, gz_lines=gz_lines)
        assert (p.n_reads, p.stop, p.done) == (n_reads, 0, 1)
        sam, host = stream.map(multi_hit=multi_hit)          # (bytes written other than announced, a span outside its window: the call fails)
        return sam, host, stream.last_unmapped()
    finally:
        stream.set_unmapped(False)
        stream.set_read_group(None)
        stream.set_tags(md=False)
        stream.set_format("sam")
        stream.set_input("fastq")


def check(texts, sam, host, un, paired, fasta_in=False, max_host=None):
    """the device's bytes against tests/un_plain.py and the FLAGs of `sam`; -> the selected units"""
    two = len(texts) == 2
    n_reads = len(sam)
    step = 2 if paired else 1
    n_units = n_reads // step
    assert len(host) <= (n_reads // 2 if max_host is None else max_host)
    assert len(un) == len(texts)
    recs = [un_plain.records(t, fasta_in) for t in texts]
    unmapped = [any(int(ln.split(b"\t")[1]) & 4 for ln in t.split(b"\n") if ln) for t in sam]
    selected = []
    for f, (data, off) in enumerate(un):
        assert len(off) == n_units + 1 and off[0] == 0 and off[-1] == len(data)
        for u in range(n_units):
            reads = range(u * step, (u + 1) * step)
            got = data[off[u]:off[u + 1]]
            if any(r in host for r in reads):
                assert got == b"", "unit %d was handed back and has bytes" % u
                continue
            sel = all(unmapped[r] for r in reads)
            mine = [recs[f][u]] if two else [recs[0][r] for r in reads]
            assert got == (b"".join(mine) if sel else b""), (f, u, sel, got[:120])
            if f == 0 and sel:
                selected.append(u)
    return selected


def as_texts(recs, kind):
    """the batch's text(s) in one of the input kinds -> (texts, paired, fasta, gz_lines)"""
    if kind == "se":
        return [fastq_decorated(recs)], False, False, 0
    if kind == "two_files":
        return [fastq_decorated(recs[0::2]), fastq(recs[1::2])], True, False, 0
    if kind == "interleaved":
        return [fastq_decorated(recs)], True, False, 0
    if kind == "fq_no_final_lf":
        return [fastq_decorated(recs)[:-1]], False, False, 0
    if kind == "gz_lines":
        return [fastq_decorated(recs)], True, False, 1
    if kind == "fa1":
        return [fasta(recs)], False, True, 0
    if kind == "fa60":
        return [fasta(recs, 60)], True, True, 0
    if kind == "fa60_no_final_lf":
        return [fasta(recs, 60)[:-1]], False, True, 0
    raise KeyError(kind)


PAIRED_KINDS = ("two_files", "interleaved", "gz_lines", "fa60")


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n_units", [1, 63, 64, 65, 129])
def test_single_end_shapes_and_selection_patterns(n_units, pattern, stream, genome, seedless):
    recs, meant = build(genome, seedless, n_units, pattern, pairs=False)
    texts, paired, fa, gz = as_texts(recs, "se")
    sam, host, un = run(stream, texts, len(recs), paired)
    selected = check(texts, sam, host, un, paired)
    assert selected == [u for u in range(n_units) if meant[u]]          # (a condition on the input: seedless reads stay unmapped, genome reads map)


@pytest.mark.parametrize("kind", ["two_files", "interleaved", "fq_no_final_lf", "gz_lines", "fa1", "fa60", "fa60_no_final_lf"])
@pytest.mark.parametrize("n_units,pattern", [(65, "alternating"), (129, "all"), (64, "last"), (129, "one_per_64")])
def test_input_kinds(kind, n_units, pattern, stream, genome, seedless):
    pairs = kind in PAIRED_KINDS
    recs, meant = build(genome, seedless, n_units, pattern, pairs)
    texts, paired, fa, gz = as_texts(recs, kind)
    assert not kind.endswith("no_final_lf") or not texts[0].endswith(b"\n")
    sam, host, un = run(stream, texts, len(recs), paired, fasta_in=fa, gz_lines=gz)
    selected = check(texts, sam, host, un, paired, fasta_in=fa)
    assert selected == [u for u in range(n_units) if meant[u]]
    if kind.endswith("no_final_lf") and meant[-1]:
        assert un[0][0].endswith(b"\n") and len(un[0][0]) == int(un[0][1][-1])          # (the line feed the file does not have is counted and written)


def test_span_starts_and_lengths_cover_every_residue_mod_16(stream, genome, seedless):
    """what the 16-byte chunks of un_copy_kernel can meet: every alignment of a span's first byte in the window and of its length (and so of where it goes)"""
    starts, lengths, dests = set(), set(), set()
    for kind in ("se", "interleaved"):
        recs, meant = build(genome, seedless, 129, "all", kind == "interleaved")
        texts, paired, fa, gz = as_texts(recs, kind)
        sam, host, un = run(stream, texts, len(recs), paired)
        selected = check(texts, sam, host, un, paired)
        assert len(selected) == 129
        step = 2 if paired else 1
        spans = un_plain.spans(texts[0], False)
        for u in selected:
            b, e = spans[u * step][0], spans[u * step + step - 1][1]
            starts.add(b % 16); lengths.add((e - b) % 16); dests.add(int(un[0][1][u]) % 16)
    assert starts == lengths == dests == set(range(16))


def test_multi_hit_reads_with_any_mapped_record_are_mapped(stream, genome, seedless):
    chains = multi_hit_batch(genome)
    extra, meant = build(genome, seedless, 40, "alternating", pairs=True)
    recs = chains[:18] + extra + chains[18:]
    texts = [fastq(recs)]
    sam, host, un = run(stream, texts, len(recs), True, multi_hit=True)
    selected = check(texts, sam, host, un, True)
    assert any(t.count(b"\n") >= 2 for t in sam), "no read with two or more records"
    assert len(selected) == sum(meant)


def test_other_formats_and_tags_give_the_same_bytes_and_the_setting_leaves_no_trace(stream, genome, seedless):
    recs, meant = build(genome, seedless, 129, "alternating", pairs=True)
    texts = [fastq(recs)]
    off = run(stream, texts, len(recs), True, unmapped=False)
    assert off[2] == []
    sam, host, un = run(stream, texts, len(recs), True)
    assert (sam, host) == off[:2], "the SAM text changed under the setting"
    assert check(texts, sam, host, un, True) == [u for u in range(129) if meant[u]]
    for kw in ({"fmt": "bam"}, {"md": True}, {"rg": b"lane1"}, {"fmt": "bam", "md": True, "rg": b"g"}):
        other = run(stream, texts, len(recs), True, **kw)
        assert other[1] == host
        assert [(d, o.tolist()) for d, o in other[2]] == [(d, o.tolist()) for d, o in un], kw
    again = run(stream, texts, len(recs), True, unmapped=False)
    assert again == off, "the output without the setting changed after runs with it"


def test_a_batch_that_needs_more_room_grows_the_buffers_inside_the_call(gpu_index_full, genome, seedless):
    """kg_stream_set_unmapped allocates nothing.  A batch without a selected unit needs no buffer; the next one's few bytes get the first (64 KiB); the
    third, every unit selected and near the window's size, outgrows it: kg_stream_map must have grown the device and the page-locked buffer"""
    from kart_amd import api
    window, max_reads = 256 << 10, 512
    s = api.Stream(gpu_index_full, max_reads=max_reads, max_window=window, lanes=1)
    try:
        for n_units, pattern, length in ((64, "none", None), (64, "first", None), (360, "all", 300)):
            recs, meant = build(genome, seedless, n_units, pattern, pairs=False)
            if length:
                recs = [(n, seedless.read(length), b"F" * length) for n, _, _ in recs]
            texts = [fastq(recs)]
            assert len(texts[0]) <= window
            sam, host, un = run(s, texts, len(recs), False)
            assert check(texts, sam, host, un, False) == [u for u in range(n_units) if meant[u]]
        assert len(un[0][0]) == len(texts[0]) > (64 << 10) + (64 << 10) // 8 and len(texts[0]) > 0.8 * window
    finally:
        s.close()
