"""GPU: MD:Z made on the device (kg_stream_set_tags; kernels/md_tag.inc in sam_size / sam_format / bam_size / bam_format of kart_amd/csrc/sam_kernels.hip and bam_kernels.hip)
against tests/md_plain.py -- the plain-Python MD of the printed SEQ, the CIGAR, POS and tests/golden/small.fa -- on a batch built for the kernel's edges:
read lengths around the 32-base text words, starts at every phase of a word, contig ends, both strands and mates, mismatches in the first and last column
and side by side, indels, clipped ends, characters that are no bases, and an MD longer than the 58 characters a lane keeps in the LDS (kMdLds in
text_device.hpp: a longer one sends the read down the record-by-record path)."""
import re

import numpy as np
import pytest

from bam_encode import bam_record
from conftest import GOLDEN
from md_plain import MD_RE, cigar_ops, md_of, reference_at
from test_bam_stream_gpu import fastq, genome, pair_at, ref_ids  # noqa: F401  (fixtures and builders of the BAM stream test)

pytestmark = pytest.mark.gpu
MD_LDS = 58          # kMdLds
ONE_CHAR = b"NR=ynr"  # reads "one_<k>" carry ONE_CHAR[k] once in either mate


@pytest.fixture(scope="module")
def stream(gpu_index_full):
    from kart_amd import api
    s = api.Stream(gpu_index_full, max_reads=16000, max_window=8 << 20, lanes=1)
    yield s
    s.close()


def other_base(c):
    return {65: 67, 67: 71, 71: 84, 84: 65}[int(c)]


def edge_batch(genome):
    """200 reads, interleaved pairs: the cases the module's docstring names (the test below asserts on the batch's own SAM lines that they are there)"""
    from kart_amd import synth
    rng = np.random.default_rng(1312)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = []

    def add(name, m1, m2):
        m1, m2 = bytes(m1), bytes(m2)
        recs.append((name, m1, b"I" * len(m1)))
        recs.append((name, m2, b"5" * len(m2)))

    # read lengths around one, two and many text words; either orientation
    for k, length in enumerate((1, 2, 31, 32, 33, 63, 64, 65, 150, 151, 300)):
        m1, m2 = pair_at(genome, "chrB", 1000 + 611 * k, length, rng, swap=bool(k & 1))
        m1 = m1.copy()
        if length >= 31:
            m1[length // 2] = other_base(m1[length // 2])
        add(b"len%d" % length, m1, m2)
    # the record's first base at every phase of a 32-base text word (the contig starts are no multiples of 32: whatever they are, three
    # consecutive starts around a multiple of 32 of the GENOME coordinate cover phases 31, 0 and 1)
    starts, at = {}, 0
    for n, g in genome.items():
        starts[n] = at
        at += len(g)
    for k, contig in enumerate(("chrA", "chrC")):
        base = 4000 + (-(starts[contig] + 4000)) % 32           # contig offset whose genome coordinate is a multiple of 32
        for d in (-1, 0, 1):
            m1, m2 = pair_at(genome, contig, base + d, 150, rng, swap=bool(k))
            m1, m2 = m1.copy(), m2.copy()
            m1[40] = other_base(m1[40])
            m2[100] = other_base(m2[100])
            add(b"phase_%s_%d" % (contig.encode(), d + 1), m1, m2)
    # POS 1 of a contig; a record that ends on the last base of the first and of the last contig
    for contig in ("decoy", "chrB"):
        m1, m2 = pair_at(genome, contig, 0, 150, rng)
        add(b"pos1_" + contig.encode(), m1, m2)
    for contig in (list(genome)[0], list(genome)[-1]):
        n = len(genome[contig])
        m1, m2 = pair_at(genome, contig, n - 400, 150, rng, swap=contig != "decoy")
        add(b"last_" + contig.encode(), m1, m2)
    # a mismatch in the first and in the last column; two and three side by side
    for k in range(4):
        m1, m2 = pair_at(genome, "chrA", 9000 + 1201 * k, 150, rng, swap=bool(k & 1))
        m1, m2 = m1.copy(), m2.copy()
        for i in ((0,), (149,), (70, 71), (30, 31, 32))[k]:
            m1[i] = other_base(m1[i])
            m2[149 - i] = other_base(m2[149 - i])
        add(b"mis%d" % k, m1, m2)
    # an inserted base, a deleted base, a deleted base with a mismatch right behind it; ends that do not match (S on either side)
    for k in range(12):
        m1, m2 = pair_at(genome, "chrA", 30000 + 1777 * k, 150, rng, swap=bool(k & 1))
        m1, m2 = m1.copy(), m2.copy()
        if k % 3 == 0:
            m1 = np.concatenate([m1[:60], acgt[rng.integers(0, 4, 1)], m1[60:]])
        elif k % 3 == 1:
            m1 = np.concatenate([m1[:80], m1[81:]])
        else:
            m1 = np.concatenate([m1[:80], m1[82:]])
            m1[80] = other_base(m1[80])
            m1[81] = other_base(m1[81])
        junk = acgt[rng.integers(0, 4, 14)]
        if k % 4 == 0:
            m2[:14] = junk
        elif k % 4 == 1:
            m2[-14:] = junk
        elif k % 4 == 2:
            m1[:14] = junk
        else:
            m1[-14:] = junk
        add(b"indel%d" % k, m1, m2)
    # lower case; N, IUPAC codes and '=' as held and through the reverse complement
    # (300 bases, a marked character every 25: seeds between them, so that the characters land in aligned columns.  The alignment stage hands
    #  reads of that many pieces back to the host, as it does the "dense" ones below: in a stream run their MD is the host's)
    for k in range(6):
        m1, m2 = pair_at(genome, "chrC", 500 + 1201 * k, 150 if k < 2 else 300, rng, frag=400 if k < 2 else 700, swap=bool(k & 1))
        m1, m2 = bytearray(bytes(m1)), bytearray(bytes(m2))
        if k < 2:
            m1, m2 = bytearray(bytes(m1).lower()), bytearray(bytes(m2).lower())
        else:
            for j, ch in enumerate(b"NRYKM=nrykm"):
                m1[15 + 25 * j] = ch
                m2[17 + 25 * j] = ch
        add(b"iupac%d" % k, m1, m2)
    # ... and one such character per read
    for k, ch in enumerate(ONE_CHAR):
        for swap in (False, True):          # (mate 1 forward shows the character as held; every other record shows what comp_char made of it)
            m1, m2 = pair_at(genome, "chrB", 6000 + 1009 * (2 * k + swap), 150, rng, swap=swap)
            m1, m2 = bytearray(bytes(m1)), bytearray(bytes(m2))
            m1[75] = ch
            m2[70] = ch
            add(b"one_%d" % k, m1, m2)
    # 300 bases whose middle 60 have every second base changed: an MD of more than MD_LDS characters
    for k in range(3):
        m1, m2 = pair_at(genome, "chrA", 52000 + 3001 * k, 300, rng, frag=700, swap=k == 1)
        m1, m2 = m1.copy(), m2.copy()
        for i in range(120, 180, 2):
            m1[i] = other_base(m1[i])
            m2[i] = other_base(m2[i])
        add(b"dense%d" % k, m1, m2)
    # random reads stay unmapped; next to a mapped mate they leave a record without a mate
    for k in range(2):
        add(b"random%d" % k, acgt[rng.integers(0, 4, 150)], acgt[rng.integers(0, 4, 150)])
    for k in range(4):
        m1, m2 = pair_at(genome, "chrB", 20000 + 997 * k, 150, rng)
        rnd = acgt[rng.integers(0, 4, 150)]
        add(b"lone%d" % k, *((m1, rnd) if k & 1 else (rnd, m2)))
    # ... and ordinary pairs with errors up to 100 pairs: the batch crosses the 64-read groups at 63 / 64 / 65 and 127 / 128 / 129
    names, r1, r2 = synth.simulate_pairs(genome, 100 - len(recs) // 2, seed=9, err=0.02, mut=0.003, indel_frac=0.3)
    for n, a, b in zip(names, r1, r2):
        add(n.encode(), a, b)
    assert len(recs) == 200
    order = rng.permutation(100)
    return [recs[2 * i + j] for i in order for j in (0, 1)]


def fields_of(texts):
    return [ln.split("\t") for t in texts for ln in t.decode("latin-1").split("\n") if ln.count("\t") >= 10]


def md_field(f):
    return f[-1][5:] if f[-1].startswith("MD:Z:") else None


def batch_conditions(lines, genome_len):
    """what the edge batch must contain, read off its own SAM lines (f = the fields of a mapped record, MD last)"""
    mapped = [f for f in lines if f[2] != "*"]
    md = [md_field(f) for f in mapped]
    assert all(m is not None for m in md)

    def has(what, cond):
        assert any(cond(f, m) for f, m in zip(mapped, md)), "no mapped record " + what
    for flag_bits, what in ((0x40, "of mate 1"), (0x80, "of mate 2")):
        has(what + " on the forward strand", lambda f, m: int(f[1]) & flag_bits and not int(f[1]) & 16)
        has(what + " on the reverse strand", lambda f, m: int(f[1]) & flag_bits and int(f[1]) & 16)
    for n in (1, 2):          # (shorter than any seed: such a read cannot map; its record goes through the kernels all the same)
        assert any(len(f[9]) == n for f in lines), "no record of %d bases" % n
    for n in (31, 32, 33, 63, 64, 65, 150, 151, 300):
        has("of %d bases" % n, lambda f, m: len(f[9]) == n)
    has("at POS 1", lambda f, m: f[3] == "1")
    for contig in (list(genome_len)[0], list(genome_len)[-1]):
        has("ending on the last base of " + contig,
            lambda f, m: f[2] == contig and int(f[3]) - 1 + sum(n for n, op in cigar_ops(f[5]) if op in "MD") == genome_len[contig])
    has("with a mismatch in the first aligned column", lambda f, m: re.match(r"0[A-Z]", m))
    has("with a mismatch in the last aligned column", lambda f, m: re.search(r"[A-Z]0$", m))
    has("with two adjacent mismatches", lambda f, m: re.search(r"[1-9][0-9]*[A-Z]0[A-Z][1-9]", m))
    has("with three adjacent mismatches", lambda f, m: re.search(r"[A-Z]0[A-Z]0[A-Z]", m))
    has("with an insertion", lambda f, m: "I" in f[5])
    has("with a deletion", lambda f, m: "D" in f[5] and "^" in m)
    has("with a deletion directly followed by a mismatch", lambda f, m: re.search(r"\^[A-Z]+0[A-Z]", m))
    has("clipped on the left", lambda f, m: re.match(r"\d+S", f[5]))
    has("clipped on the right", lambda f, m: f[5].endswith("S"))
    has("in lower case", lambda f, m: f[9].islower())
    for k, ch in enumerate(ONE_CHAR.decode()):
        has("with %r in an aligned column, as held" % ch, lambda f, m: f[0] == "one_%d" % k and ch in f[9] and "S" not in f[5])
        if ch not in "Nn":
            has("with %r in an aligned column, through the reverse complement" % ch, lambda f, m: f[0] == "one_%d" % k and ch not in f[9] and "N" in f[9] and "S" not in f[5])
    has("with an MD longer than the in-LDS limit", lambda f, m: len(m) > MD_LDS)
    has("with an MD of exactly a number", lambda f, m: m.isdigit())
    has("without a mate", lambda f, m: f[6] == "*")
    assert any(f[2] == "*" for f in lines), "no unmapped record"


def contig_phases(lines, genome):
    starts, at = {}, 0
    for n, s in genome.items():
        starts[n] = at
        at += len(s)
    return {(starts[f[2]] + int(f[3]) - 1) % 32 for f in lines if f[2] != "*"}


def check_md(on, off, genome_str):
    """on / off: the texts per read with and without the tag.  Every line minus its MD is the line without; MD is the plain model's"""
    assert len(on) == len(off)
    n = 0
    for a, b in zip(on, off):
        la, lb = a.decode("latin-1").split("\n"), b.decode("latin-1").split("\n")
        assert len(la) == len(lb)
        for x, y in zip(la, lb):
            if x.count("\t") < 10:
                assert x == y
                continue
            f = x.split("\t")
            if f[2] == "*":
                assert x == y
                continue
            assert f[-1].startswith("MD:Z:") and "\t".join(f[:-1]) == y, (x, y)
            md = f[-1][5:]
            assert MD_RE.fullmatch(md), x
            assert md == md_of(f[9], f[5], reference_at(genome_str[f[2]], int(f[3]))), x
            n += 1
    return n


def bam_with_z(text, ref_ids):
    """the BAM records of SAM lines whose last optional field may be TAG:Z:value (tests/bam_encode.py encodes the integer fields)"""
    out = b""
    for ln in text.split(b"\n"):
        if ln.count(b"\t") < 10:
            continue
        f = ln.split(b"\t")
        z = b""
        if f[-1][2:5] == b":Z:":
            z = f[-1][:2] + b"Z" + f[-1][5:] + b"\0"
            ln = b"\t".join(f[:-1])
        rec = bam_record(ln, ref_ids)
        size = int.from_bytes(rec[:4], "little") + len(z)
        out += size.to_bytes(4, "little") + rec[4:] + z
    return out


def run_batch(stream, text, n_reads, multi_hit=False, fasta=False):
    """the same text through the stream as SAM and BAM, with and without the tag: {(fmt, md): texts per read}"""
    out = {}
    try:
        stream.set_input("fasta" if fasta else "fastq")
        for fmt in ("sam", "bam"):
            for md in (False, True, False):           # (off again behind on: the parent's output once more)
                stream.set_format(fmt)
                stream.set_tags(md=md)
                p = stream.parse(text, None, paired=True, chunk_reads=8, want_reads=(n_reads + 7) // 8 * 8)
                assert (p.n_reads, p.stop, p.done) == (n_reads, 0, 1)
                texts, host = stream.map(multi_hit=multi_hit)      # (a format error of the device -- ctl[1] != 0 -- fails the call)
                assert len(host) < n_reads // 2
                if (fmt, md) in out:
                    assert out[fmt, md] == (texts, host), "the output without the tag changed after a run with it"
                out[fmt, md] = (texts, host)
    finally:
        stream.set_tags(md=False)
        stream.set_format("sam")
        stream.set_input("fastq")
    return out


def check_all(out, genome_str, ref_ids):
    (sam_off, h0), (sam_on, h1), (bam_off, h2), (bam_on, h3) = out["sam", False], out["sam", True], out["bam", False], out["bam", True]
    assert h0 == h1 == h2 == h3
    n = check_md(sam_on, sam_off, genome_str)
    for i, (s, b) in enumerate(zip(sam_on, bam_on)):
        assert b == bam_with_z(s, ref_ids), (i, s[:300])
    for s, b in zip(sam_off, bam_off):
        assert b == bam_with_z(s, ref_ids)
    return n


def test_device_md_on_the_edge_batch(stream, genome, ref_ids):
    recs = edge_batch(genome)
    genome_str = {n: s.tobytes().decode() for n, s in genome.items()}
    out = run_batch(stream, fastq(recs), len(recs))
    assert check_all(out, genome_str, ref_ids) > 150
    lines = fields_of(out["sam", True][0])
    print("handed back to the host:", sorted({recs[i][0] for i in out["sam", True][1]}))
    batch_conditions(lines, {n: len(s) for n, s in genome.items()})
    assert {0, 1, 31} <= contig_phases(lines, genome)


def multi_hit_batch(genome):
    from kart_amd import synth
    recs = []
    g = genome["chrA"]
    for base in (20260, 20969, 44045):
        for d in (0, 40, 80):
            for swap in (False, True):
                m2 = synth.revcomp(g[base + d:base + d + 150])
                m1 = g[base + d - 380:base + d - 230].copy()
                m1[60], m2[90] = other_base(m1[60]), other_base(m2[90])          # (every record of a chain shows it: no MD is a plain number)
                a, b = (m2, m1) if swap else (m1, m2)
                n = b"rep%d_%d_%d" % (base, d, swap)
                recs.append((n, bytes(a), b"I" * 150))
                recs.append((n, bytes(b), b"!" * 75 + b"~" * 75))
    return recs


def test_device_md_with_multi_hit(stream, genome, ref_ids):
    """-m: reads from the repeat of the golden pe_m case (chrA 20261 / 20970 / 44046) carry a chain of records, each with its own MD"""
    recs = multi_hit_batch(genome)
    genome_str = {n: s.tobytes().decode() for n, s in genome.items()}
    out = run_batch(stream, fastq(recs), len(recs), multi_hit=True)
    assert check_all(out, genome_str, ref_ids) >= len(recs)
    chains = [t for t in out["sam", True][0] if t.count(b"\n") >= 2]
    assert chains, "no read with two or more records"
    assert all(re.fullmatch(rb"MD:Z:\d+[ACGT]\d+", ln.split(b"\t")[-1]) for t in chains for ln in t.split(b"\n") if ln), "a chained record without the planted mismatch"


def test_device_md_with_fasta_input(stream, genome, ref_ids):
    recs = edge_batch(genome)
    text = b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _ in recs)
    genome_str = {n: s.tobytes().decode() for n, s in genome.items()}
    out = run_batch(stream, text, len(recs), fasta=True)
    assert check_all(out, genome_str, ref_ids) > 150
    assert any(len(md_field(f) or "") > MD_LDS for f in fields_of(out["sam", True][0]))


def test_set_tags_rejects_an_unknown_bit(stream):
    from kart_amd import api
    with pytest.raises(api.KartAmdError):
        api._check(stream.lib.kg_stream_set_tags(stream.h, 2), "kg_stream_set_tags")
