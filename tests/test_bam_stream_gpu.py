"""GPU: BAM records made on the device (kg_stream_set_format, bam_size_kernel / bam_format_kernel in kart_amd/csrc/bam_kernels.hip) against
tests/bam_encode.py -- an encoder of the printed SAM line written from the SAM/BAM specification, which tests/test_bam_records_cpu.py holds the
host's own encoder to -- and the product's -bo run through the device stream against the same run with the host's reader, printer and encoder."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from bam_encode import bam_records_of_text
from conftest import GOLDEN, ROOT, SMALL_PREFIX
from test_bam_output import decode_bam, sam_records

pytestmark = pytest.mark.gpu
KART_AMD = os.path.join(ROOT, "kart_amd", "bin", "kart-amd")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def genome():
    from kart_amd.index_build import read_fasta
    return {n: s for n, _, s in read_fasta(os.path.join(GOLDEN, "small.fa"))}


@pytest.fixture(scope="module")
def ref_ids(genome):
    return {n.encode(): i for i, n in enumerate(genome)}          # (the index keeps the FASTA's order; the product test below does not rely on it)


@pytest.fixture(scope="module")
def stream(gpu_index_full):
    from kart_amd import api
    s = api.Stream(gpu_index_full, max_reads=16000, max_window=8 << 20, lanes=1)
    yield s
    s.close()


def fastq(recs) -> bytes:
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs)


def both_formats(stream, text, n_reads, multi_hit):
    """the same text parsed and mapped twice: -> (SAM text per read, BAM bytes per read, reads handed back in either run)"""
    out = []
    try:
        for fmt in ("sam", "bam"):
            stream.set_format(fmt)
            p = stream.parse(text, None, paired=True, chunk_reads=8, want_reads=(n_reads + 7) // 8 * 8)
            assert (p.n_reads, p.stop, p.done) == (n_reads, 0, 1)
            out.append(stream.map(multi_hit=multi_hit))
    finally:
        stream.set_format("sam")
    (sam, host_s), (bam, host_b) = out
    return sam, bam, host_s, host_b


def compare(sam, bam, host_s, host_b, ref_ids):
    assert host_s == host_b
    assert len(sam) == len(bam)
    for i in host_s:
        assert sam[i] == b"" and bam[i] == b""
    for i, (s, b) in enumerate(zip(sam, bam)):
        want = bam_records_of_text(s, ref_ids)
        assert b == want, (i, s[:200], b.hex(), want.hex())


def pair_at(genome, contig, p, length, rng, frag=400, swap=False):
    """(mate 1, mate 2) of a fragment at contig[p, p + frag): mate 2 is the reverse complement of the far end; swap: the other strand"""
    from kart_amd import synth
    g = genome[contig]
    left, right = g[p:p + length].copy(), synth.revcomp(g[p + frag - length:p + frag])
    return (right, left) if swap else (left, right)


def edge_batch(genome):
    """interleaved pairs: every path of the BAM kernels at least once (the assertions of the test below name them)"""
    from kart_amd import synth
    rng = np.random.default_rng(2025)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = []

    def add(name, m1, m2, q1=None, q2=None, name2=None):
        m1, m2 = bytes(m1), bytes(m2)
        recs.append((name, m1, b"I" * len(m1) if q1 is None else q1))
        recs.append((name if name2 is None else name2, m2, b"5" * len(m2) if q2 is None else q2))

    # every length at which the chunked copy changes: below / at / above 16 bytes of packed bases (32 bases), of qualities (16), odd tails
    for k, length in enumerate((1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, 300)):
        m1, m2 = pair_at(genome, "chrB", 1000 + 611 * k, length, rng, swap=bool(k & 1))
        add(b"len%d" % length, m1, m2)
    # exact 300-base copies of the reference: AS = 300 needs the 16-bit tag type
    for k in range(3):
        m1, m2 = pair_at(genome, "chrA", 3000 + 7001 * k, 300, rng, frag=700, swap=k == 1)
        add(b"exact300_%d" % k, m1, m2)
    # an inserted and a deleted base, ends that do not match: CIGARs of several operations
    for k in range(10):
        m1, m2 = pair_at(genome, "chrA", 30000 + 1777 * k, 150, rng, swap=bool(k & 1))
        m1 = np.concatenate([m1[:60], acgt[rng.integers(0, 4, 1)], m1[60:100], m1[101:]])
        m2 = m2.copy()
        junk = acgt[rng.integers(0, 4, 14)]
        if k % 3 == 0:
            m2[:14] = junk
        elif k % 3 == 1:
            m2[-14:] = junk
        add(b"indel%d" % k, m1, m2)
    # lower case, IUPAC codes and '=' in reads (shown as held: their own 4-bit codes; through the reverse complement: N)
    for k in range(6):
        m1, m2 = pair_at(genome, "chrC", 500 + 1301 * k, 150, rng, swap=bool(k & 1))
        m1, m2 = bytearray(bytes(m1)), bytearray(bytes(m2))
        if k < 2:
            m1, m2 = bytearray(bytes(m1).lower()), bytearray(bytes(m2).lower())
        else:
            for j, ch in enumerate(b"NRYKM=nrykm"):
                m1[9 + 12 * j] = ch
                m2[11 + 12 * j] = ch
        add(b"iupac%d" % k, m1, m2)
    # quality strings: shorter than the read, empty, bytes below '!' (no borrow between the bytes of a word), a tab
    low = bytes([1, 2, 31, 32, 32, 1, 33, 34, 0x7E, 0xFF, 0x80, 11, 12, 13, 14, 15] * 10)
    for k, (qa, qb) in enumerate(((b"I" * 100, None), (None, b"I" * 149), (b"", b"F"), (low[:150], low[5:155]), (low[:150], None), (b"I" * 70 + b"\t" + b"I" * 79, None),
                                  (None, b"5" * 20 + b"\t" + b"5" * 129))):
        m1, m2 = pair_at(genome, "chrB", 12000 + 907 * k, 150, rng, swap=bool(k & 1))
        add(b"qual%d" % k, m1, m2, qa, qb)
    # names of 1, 250 and (l_read_name is one byte) 260 characters
    for k, name in enumerate((b"x", b"n" * 250, b"w" * 260)):
        m1, m2 = pair_at(genome, "chrA", 50000 + 803 * k, 150, rng)
        add(name, m1, m2)
    # random reads stay unmapped; next to a mapped mate they leave a record without a mate
    for k in range(3):
        add(b"random%d" % k, acgt[rng.integers(0, 4, 150)], acgt[rng.integers(0, 4, 150)])
    for k in range(4):
        m1, m2 = pair_at(genome, "chrB", 20000 + 997 * k, 150, rng)
        rnd = acgt[rng.integers(0, 4, 150)]
        add(b"lone%d" % k, *((m1, rnd) if k & 1 else (rnd, m2)))
    # ... and ordinary pairs of either orientation up to 100 pairs: the batch crosses the 64-read groups at 63 / 64 / 65 and 127 / 128 / 129
    names, r1, r2 = synth.simulate_pairs(genome, 100 - len(recs) // 2, seed=7)
    for n, a, b in zip(names, r1, r2):
        add(n.encode(), a, b)
    assert len(recs) == 200
    # the special reads spread over the batch, pairs kept together
    order = rng.permutation(100)
    return [recs[2 * i + j] for i in order for j in (0, 1)]


def test_device_bam_records_equal_the_encoded_sam_lines(stream, genome, ref_ids):
    recs = edge_batch(genome)
    sam, bam, host_s, host_b = both_formats(stream, fastq(recs), len(recs), multi_hit=False)
    compare(sam, bam, host_s, host_b, ref_ids)
    # the batch covers what it was built for
    lines = [l.split(b"\t") for s in sam for l in s.split(b"\n") if l.count(b"\t") >= 10]
    mapped = [f for f in lines if f[2] != b"*"]
    assert any(not int(f[1]) & 16 for f in mapped), "no record mapped forward"
    assert any(int(f[1]) & 16 for f in mapped), "no record mapped to the reverse strand"
    assert any(f[2] == b"*" for f in lines), "no unmapped record"
    assert any(f[6] == b"*" for f in mapped), "no mapped record without a mate"
    assert any(sum(c in b"MIDNSHP=X" for c in f[5]) >= 2 for f in mapped), "no CIGAR of several operations"
    assert any(int(o[5:]) >= 256 for f in mapped for o in f[11:] if o.startswith(b"AS:i:")), "no AS beyond one byte"
    assert len(host_s) < 100


def test_device_bam_records_with_multi_hit(stream, genome, ref_ids):
    """-m: reads from the repeat of the golden pe_m case (chrA 20261 / 20970 / 44046) carry a chain of records"""
    from kart_amd import synth
    recs = []
    g = genome["chrA"]
    for base in (20260, 20969, 44045):
        for d in (0, 40, 80):
            for swap in (False, True):
                m2 = synth.revcomp(g[base + d:base + d + 150])
                m1 = g[base + d - 380:base + d - 230]
                a, b = (m2, m1) if swap else (m1, m2)
                n = b"rep%d_%d_%d" % (base, d, swap)
                recs.append((n, bytes(a), b"I" * 150))
                recs.append((n, bytes(b), b"!" * 75 + b"~" * 75))
    sam, bam, host_s, host_b = both_formats(stream, fastq(recs), len(recs), multi_hit=True)
    compare(sam, bam, host_s, host_b, ref_ids)
    assert any(s.count(b"\n") >= 2 for s in sam), "no read with two or more records"


def _golden(name, tmp_path):
    dst = str(tmp_path / name)
    with gzip.open(os.path.join(GOLDEN, "sam", name + ".gz")) as fi, open(dst, "wb") as fo:
        fo.write(fi.read())
    return dst


@pytest.mark.parametrize("case", ["session", "plain", "m", "gz"])
def test_product_bam_runs_through_the_stream(case, built_lib, tmp_path):
    """session: a HostSession's -bo run goes through the device stream and decodes to the golden SAM's records; plain / m / gz: the stream's
    file == the file of the host's reader, printer and encoder (KART_AMD_NO_STREAM=1), byte for byte, each from a fresh process"""
    from kart_amd import api
    f1, f2 = _golden("pe_1.fq", tmp_path), _golden("pe_2.fq", tmp_path)
    if case == "session":
        out = str(tmp_path / "a.bam")
        sess = api.HostSession(SMALL_PREFIX, 0, 8)
        try:
            st = sess.map(["-f", f1, "-f2", f2, "-bo", out])
        finally:
            sess.close()
        assert st.stream_reads == st.total_reads > 0
        head, want = sam_records(_golden("pe.sam", tmp_path))
        text, refs, got = decode_bam(out)
        assert text == head and got == want
        assert open(out, "rb").read()[-28:] == BGZF_EOF
        return
    if case == "gz":
        for f in (f1, f2):
            with open(f, "rb") as fi, gzip.open(f + ".gz", "wb", compresslevel=6) as fo:
                fo.write(fi.read())
        f1, f2 = f1 + ".gz", f2 + ".gz"
    args = ["-f", f1, "-f2", f2] + (["-m"] if case == "m" else [])
    files = []
    for how, env in (("stream", {}), ("host", {"KART_AMD_NO_STREAM": "1"})):
        o = str(tmp_path / ("%s_%s.bam" % (case, how)))
        r = subprocess.run([KART_AMD, "-silent", "-i", SMALL_PREFIX, "-t", "8"] + args + ["-bo", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           env=dict(os.environ, KART_AMD_VERBOSE="1", KART_AMD_UNSET_FLAG="0", **env), timeout=120)
        assert r.returncode == 0, r.stdout.decode()[-600:]
        assert ("device stream:" in r.stdout.decode()) == (how == "stream"), r.stdout.decode()[-600:]
        files.append(open(o, "rb").read())
    assert files[0] == files[1]
    assert files[0][-28:] == BGZF_EOF and len(files[0]) > 100000
