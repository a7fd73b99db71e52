"""GPU: FASTA read libraries through the device stream (kg_stream_set_input; fa_line / fa_head / fa_record / fa_materialise kernels in
kart_amd/csrc/read_kernels.hip) against the reference's readers restated in tests/fasta_reads.py, the output against the FASTQ form of the same
reads with the quality column starred and against tests/bam_encode.py, and the product binary against the reference's golden SAM and against its
own host path (KART_AMD_NO_STREAM=1 / KART_AMD_NO_GZ_STREAM=1)."""
import gzip
import os
import subprocess

import pytest

from bam_encode import bam_records_of_text
from conftest import GOLDEN, ROOT, SMALL_PREFIX
from fasta_reads import fasta_reads, fasta_reads_gz, fasta_text, held, reads_mapped, wrap

pytestmark = pytest.mark.gpu
KART_AMD = os.path.join(ROOT, "kart_amd", "bin", "kart-amd")
STOP_IRREGULAR, STOP_TAIL = 1, 2
COLS = (1, 15, 16, 17, 31, 32, 33, 60, 127, 128, 129)


@pytest.fixture(scope="module")
def stream(gpu_index_full):
    from kart_amd import api
    s = api.Stream(gpu_index_full, max_reads=16000, max_window=8 << 20, lanes=2)
    s.set_input("fasta")
    yield s
    s.close()


def _golden_text(name):
    return gzip.open(os.path.join(GOLDEN, "sam", name + ".gz")).read()


def some_reads(n, seed=5):
    """[(header, sequence)]: lengths 1 .. 300 (every 16-byte tail and 128-byte step of the gather among them), lower case and IUPAC codes"""
    import numpy as np
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNRYKMn", np.uint8)
    lengths = [1, 2, 15, 16, 17, 31, 32, 33, 59, 60, 61, 127, 128, 129, 143, 144, 145, 255, 256, 257, 299, 300]
    return [(b"r%d extra words/1" % i, alphabet[rng.integers(0, len(alphabet), lengths[i % len(lengths)] if i < len(lengths) else int(rng.integers(1, 301)))].tobytes())
            for i in range(n)]


def parsed_reads(stream, text1, text2=None, paired=False, want=None, **kw):
    n = len(fasta_reads(text1)) * (2 if text2 is not None else 1)
    p = stream.parse(text1, text2, paired=paired, chunk_reads=8, want_reads=want or (n + 7) // 8 * 8, **kw)
    return p, (stream.fetch_reads(p) if p.n_reads else [])


@pytest.mark.parametrize("cols", (None,) + COLS)
def test_parser_equals_the_reader(stream, cols):
    recs = some_reads(40)
    text = fasta_text(recs, cols)
    want = fasta_reads(text)
    assert [s for _, s in want] == [s for _, s in recs]
    # single reads
    p, got = parsed_reads(stream, text)
    assert (p.n_reads, p.n_chunks, p.stop, p.done, p.used[0]) == (40, 5, 0, 1, len(text))
    assert got == [s for _, s in want]
    # interleaved pairs: mate 2 is held reverse-complemented (lower case and IUPAC codes go through GetComplementaryBase)
    p, got = parsed_reads(stream, text, paired=True)
    assert (p.n_reads, p.done) == (40, 1)
    assert got == [held(s, bool(i & 1)) for i, (_, s) in enumerate(want)]
    # two files, the second wrapped differently
    text2 = fasta_text(recs[::-1], 60 if cols is None else None)
    want2 = fasta_reads(text2)
    p, got = parsed_reads(stream, text, text2, paired=True)
    assert (p.n_reads, p.done, p.used[0], p.used[1]) == (80, 1, len(text), len(text2))
    assert got == [held((want, want2)[i & 1][i >> 1][1], bool(i & 1)) for i in range(80)]


def test_parser_line_rules(stream):
    recs = some_reads(24, seed=6)
    # CR LF line ends: the '\r' of every sequence line stays in the sequence
    text = fasta_text(recs, 60, b"\r\n")
    p, got = parsed_reads(stream, text, paired=True)
    assert p.n_reads == 24 and got == [held(s, bool(i & 1)) for i, (_, s) in enumerate(fasta_reads(text))]
    assert got[0].count(b"\r") == (len(recs[0][1]) + 59) // 60
    # a blank line inside a sequence adds nothing
    text = b"".join(b">" + n + b"\n" + s[:7] + b"\n\n" + s[7:] + b"\n" for n, s in recs)
    p, got = parsed_reads(stream, text)
    assert p.n_reads == 24 and got == [s for _, s in recs] == [s for _, s in fasta_reads(text)]
    # no final newline: the last base is lost (one-line and wrapped records)
    for cols in (None, 16):
        text = fasta_text(recs, cols)[:-1]
        p, got = parsed_reads(stream, text)
        assert (p.n_reads, p.done, p.used[0]) == (24, 1, len(text))
        assert got == [s for _, s in fasta_reads(text)] and got[-1] == recs[-1][1][:-1]
    # a first line that does not start with '>' is a header all the same
    text = b"@" + fasta_text(recs, 33)[1:]
    p, got = parsed_reads(stream, text)
    assert p.n_reads == 24 and got == [s for _, s in fasta_reads(text)]


def test_window_cut_behind_a_sequence_line(stream):
    """the sequence of the window's last record may go on in the next window: the record counts only if the file ends there"""
    recs = [(n, s * 2) for n, s in some_reads(17, seed=7)]
    text = fasta_text(recs, 60)
    hdr16 = text.index(b">r16 ")
    for cut in (len(text), hdr16 + len(b">r16 extra words/1\n") + min(61, len(recs[16][1]) + 1)):   # behind the record's last / first sequence line
        window = text[:cut]
        assert window.endswith(b"\n")
        p, got = parsed_reads(stream, window, want=24, eof=(False, False), begin=(333, 0))
        assert (p.n_reads, p.stop, p.done, p.used[0]) == (16, 0, 0, 333 + hdr16)
        assert got == [s for _, s in recs[:16]]
    p, got = parsed_reads(stream, text, want=24, eof=(True, True), begin=(333, 0))
    assert (p.n_reads, p.stop, p.done, p.used[0]) == (17, 0, 1, 333 + len(text))
    assert got == [s for _, s in recs]


def test_parser_stops(stream):
    recs = some_reads(40, seed=8)
    # a header directly behind a header: an empty read ends a chunk early in the reference
    bad = fasta_text(recs[:19], 60) + b">empty\n" + fasta_text(recs[20:], 60)
    p, _ = parsed_reads(stream, bad)
    assert (p.n_reads, p.stop, p.done, p.used[0]) == (16, STOP_IRREGULAR, 0, bad.index(b">r16 "))
    # a NUL byte: lines are C strings in the reference
    p, _ = parsed_reads(stream, fasta_text(recs, 60).replace(b"r7 ", b"r7\0"))
    assert (p.n_reads, p.stop) == (0, STOP_IRREGULAR)
    # a lone mate at the end of an interleaved file
    p, _ = parsed_reads(stream, fasta_text(recs[:39], 60), paired=True)
    assert (p.n_reads, p.stop, p.done) == (32, STOP_TAIL, 0)
    # mate files of different record counts
    p, _ = parsed_reads(stream, fasta_text(recs[:20]), fasta_text(recs[:17], 60), paired=True)
    assert (p.n_reads, p.stop, p.done) == (32, STOP_TAIL, 0)
    # the text of a gz file: gzgets() takes one sequence line per entry, and at most 999 bytes per call
    ok = fasta_text(recs)
    p, got = parsed_reads(stream, ok, gz_lines=1)
    assert (p.n_reads, p.done) == (40, 1) and got == [s for _, s in fasta_reads_gz(ok)]
    two = fasta_text(recs[:19]) + b">two\nACGTACGT\nACGT\n" + fasta_text(recs[20:])
    p, _ = parsed_reads(stream, two, gz_lines=1)
    assert (p.n_reads, p.stop) == (16, STOP_IRREGULAR)
    for line, reads in ((b"A" * 998 + b"\n", 40), (b"A" * 999 + b"\n", 16)):            # 999 bytes fit a call, 1000 do not
        long = fasta_text(recs[:19]) + b">long\n" + line + fasta_text(recs[20:])
        p, _ = parsed_reads(stream, long, gz_lines=1)
        assert (p.n_reads, p.stop) == (reads, 0 if reads == 40 else STOP_IRREGULAR)
    p, _ = parsed_reads(stream, fasta_text(recs[:19]) + b">\nACGT\n" + fasta_text(recs[20:]), gz_lines=1)     # a header that names nothing
    assert (p.n_reads, p.stop) == (16, STOP_IRREGULAR)


def test_more_records_or_lines_than_the_tables_hold(stream):
    """a window whose records or lines outnumber the parser's tables is the caller's reader's: nothing is taken, and nothing is read outside the tables.
    The stream's windows are 8 MB: 528 384 lines, 264 193 records"""
    for text in (b">a\n" * 300000,                 # 300 000 records of one line each: the record table
                 b">a\nA\n" * 300000,             # 600 000 lines: the line table
                 b"\n" * 600000):                 # ... of one record
        p = stream.parse(text, None, paired=False, chunk_reads=8, want_reads=16000)
        assert (p.n_reads, p.stop, p.done) == (0, STOP_IRREGULAR, 0)
    # 250 000 two-line records fit both tables
    text = b">a\nA\n" * 250000
    p = stream.parse(text, None, paired=False, chunk_reads=8, want_reads=16000, eof=(False, False))
    assert (p.n_reads, p.stop, p.used[0]) == (16000, 0, 5 * 16000)


def test_set_input_rejects_an_unknown_value(stream):
    from kart_amd import api
    for bad in ("bam", 7, -1):
        with pytest.raises(api.KartAmdError):
            stream.set_input(bad)
    # ... and the input stays what it was
    p, got = parsed_reads(stream, b">x\nAC\nGT\n")
    assert p.n_reads == 1 and got == [b"ACGT"]


def as_fastq(fasta: bytes, q=b"I") -> bytes:
    return b"".join(b"@" + n0 + b"\n" + s + b"\n+\n" + q * len(s) + b"\n" for n0, s in raw_records(fasta))


def raw_records(fasta: bytes):
    """[(header line without its first byte and newline, sequence)] of a well-formed FASTA text"""
    out = []
    for block in fasta.split(b"\n>"):
        lines = block.lstrip(b">").split(b"\n")
        out.append((lines[0], b"".join(lines[1:])))
    return out


def starred(text: bytes) -> bytes:
    out = []
    for line in text.split(b"\n")[:-1]:
        f = line.split(b"\t")
        f[10] = b"*"
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


@pytest.fixture(scope="module")
def ref_ids():
    from kart_amd.index_build import read_fasta
    return {n.encode(): i for i, (n, _, _) in enumerate(read_fasta(os.path.join(GOLDEN, "small.fa")))}


@pytest.fixture(scope="module")
def both_forms(stream):
    """the golden single-end FASTA set, and the first 1999 golden pairs with both files wrapped at 60 columns (a one-base read in front of either: 4000
    reads): mapped as FASTA (SAM and BAM) and as the FASTQ form of the same reads with a constant quality, on the same stream"""
    se = b">one_base\nA\n" + _golden_text("se.fa")
    pe1 = b">one_base/1\nC\n" + b"".join(b">" + n + b"\n" + wrap(s, 60) for n, s in raw_records(_golden_text("pe_fasta_1.fa"))[:1999])
    pe2 = b">one_base/2\nG\n" + b"".join(b">" + n + b"\n" + wrap(s, 60) for n, s in raw_records(_golden_text("pe_fasta_2.fa"))[:1999])
    out = {}
    try:
        for name, texts, paired in (("se", (se, None), False), ("pe", (pe1, pe2), True)):
            n = sum(t.count(b">") for t in texts if t)
            want = (n + 3999) // 4000 * 4000
            for kind, fmt in (("fasta", "sam"), ("fasta", "bam"), ("fastq", "sam")):
                stream.set_input(kind)
                stream.set_format(fmt)
                tt = [t if kind == "fasta" or t is None else as_fastq(t) for t in texts]
                p = stream.parse(tt[0], tt[1], paired=paired, want_reads=want, lane=1)
                assert (p.n_reads, p.done) == (n, 1)
                out[name, kind, fmt] = stream.map(lane=1)
    finally:
        stream.set_input("fasta")
        stream.set_format("sam")
    return out


@pytest.mark.parametrize("name", ["se", "pe"])
def test_output_equals_fastq_with_the_quality_column_starred(both_forms, ref_ids, name):
    fa, host_fa = both_forms[name, "fasta", "sam"]
    fq, host_fq = both_forms[name, "fastq", "sam"]
    bam, host_bam = both_forms[name, "fasta", "bam"]
    assert host_fa == host_fq == host_bam                     # alignment ignores qualities
    assert len(host_fq) * 4000 <= 200 * len(fq)               # the share of test_stream_gpu.py's golden case: 200 of 4000
    handed = set(host_fa)
    for i, (a, q, b) in enumerate(zip(fa, fq, bam)):
        if i in handed:
            assert a == b"" and b == b""
            continue
        assert a == starred(q) and a.count(b"\n") == 1, i
        assert b == bam_records_of_text(a, ref_ids), i
    # the one-base reads (their "*" column is as long as l_seq) were decided on the device
    assert 0 not in handed and fa[0].split(b"\t")[9:11] == [b"A" if name == "se" else b"C", b"*"]


def test_decided_lines_equal_the_reference_sam(both_forms):
    text, host = both_forms["se", "fasta", "sam"]
    want = [l + b"\n" for l in _golden_text("se_fasta.sam").split(b"\n") if l and not l.startswith(b"@")]
    assert len(text) == len(want) + 1
    handed = set(host)
    assert [t for i, t in enumerate(text[1:], 1) if i not in handed] == [w for i, w in enumerate(want, 1) if i not in handed]


def _run(args, out, env=None, fmt="-o"):
    r = subprocess.run([KART_AMD, "-silent", "-i", SMALL_PREFIX, "-t", "8"] + args + [fmt, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, KART_AMD_VERBOSE="1", KART_AMD_UNSET_FLAG="0", **(env or {})), timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-600:]
    return r.stdout.decode(), open(out, "rb").read()


def _put(tmp_path, name, data, gz=False):
    dst = str(tmp_path / name)
    (gzip.open(dst, "wb", compresslevel=6) if gz else open(dst, "wb")).write(data)
    return dst


def test_product_single_end_fasta_runs_through_the_stream(built_lib, tmp_path):
    fa = _put(tmp_path, "se.fa", _golden_text("se.fa"))
    log, got = _run(["-f", fa], str(tmp_path / "a.sam"))
    assert "device stream:" in log, log[-400:]
    assert got == _golden_text("se_fasta.sam")
    log2, got2 = _run(["-f", fa], str(tmp_path / "b.sam"), {"KART_AMD_NO_STREAM": "1"})
    assert "device stream:" not in log2 and got2 == got


@pytest.mark.parametrize("case", ["two_files", "interleaved", "m", "bam"])
def test_product_paired_fasta_equals_the_host_path(case, built_lib, tmp_path):
    t1, t2 = _golden_text("pe_fasta_1.fa"), _golden_text("pe_fasta_2.fa")
    if case == "interleaved":
        r1, r2 = raw_records(t1), raw_records(t2)
        text = b"".join(b">" + n + b"\n" + (s + b"\n" if k == 0 else wrap(s, 60)) for a, b in zip(r1, r2) for k, (n, s) in enumerate((a, b)))
        args = ["-f", _put(tmp_path, "il.fa", text), "-p"]
    else:
        args = ["-f", _put(tmp_path, "1.fa", t1), "-f2", _put(tmp_path, "2.fa", t2)] + (["-m"] if case == "m" else [])
    fmt = "-bo" if case == "bam" else "-o"
    log, got = _run(args, str(tmp_path / "a.out"), fmt=fmt)
    assert "device stream:" in log, log[-400:]
    log2, got2 = _run(args, str(tmp_path / "b.out"), {"KART_AMD_NO_STREAM": "1"}, fmt=fmt)
    assert "device stream:" not in log2
    assert got == got2 and len(got) > 100000
    if case == "two_files":
        assert got == _golden_text("pe_fasta.sam")


def test_product_gz_fasta(built_lib, tmp_path):
    text = _golden_text("se.fa")
    assert all(len(b.split(b"\n")) == 2 for b in text.split(b"\n>")[:-1])          # one sequence line per record
    _, plain = _run(["-f", _put(tmp_path, "se.fa", text)], str(tmp_path / "p.sam"))
    log, got = _run(["-f", _put(tmp_path, "se.fa.gz", text, gz=True)], str(tmp_path / "g.sam"))
    assert "device stream:" in log and got == plain
    # 60 columns: gzgets() takes the record's second sequence line for the next entry's header; the stream leaves such text to the gz reader
    wrapped = b"".join(b">" + n + b"\n" + wrap(s, 60) for n, s in raw_records(text)[:500])
    assert reads_mapped(fasta_reads_gz(wrapped)) != reads_mapped(fasta_reads(wrapped))
    wz = _put(tmp_path, "w.fa.gz", wrapped, gz=True)
    _, a = _run(["-f", wz], str(tmp_path / "w1.sam"))
    _, b = _run(["-f", wz], str(tmp_path / "w2.sam"), {"KART_AMD_NO_GZ_STREAM": "1"})
    assert a == b
    names = [l.split(b"\t")[0] for l in a.split(b"\n") if l and not l.startswith(b"@")]
    assert names == [n for n, _ in reads_mapped(fasta_reads_gz(wrapped))]


def test_product_chunk_ends_at_an_empty_record(built_lib, tmp_path):
    """a library whose 13th record is empty: the chunk ends there on both paths (GetNextChunk, src/GetData.cpp:116,124), the empty read is dropped and
    the next chunk starts behind it; the device parser stops in front of such a record and the host's reader continues"""
    recs = raw_records(_golden_text("se.fa"))[:40]
    recs[12] = (b"empty", b"")
    text = b"".join(b">" + n + b"\n" + (wrap(s, 60) if s else b"") for n, s in recs)
    fa = _put(tmp_path, "e.fa", text)
    _, a = _run(["-f", fa], str(tmp_path / "a.sam"))
    _, b = _run(["-f", fa], str(tmp_path / "b.sam"), {"KART_AMD_NO_STREAM": "1"})
    assert a == b
    names = [l.split(b"\t")[0] for l in a.split(b"\n") if l and not l.startswith(b"@")]
    assert names == [n for n, _ in reads_mapped(fasta_reads(text))] and len(names) == 39
    # ... and in front of a chunk: the library ends there
    text = b">empty\n" + text
    fa = _put(tmp_path, "e2.fa", text)
    _, a = _run(["-f", fa], str(tmp_path / "a2.sam"))
    _, b = _run(["-f", fa], str(tmp_path / "b2.sam"), {"KART_AMD_NO_STREAM": "1"})
    assert a == b and not [l for l in a.split(b"\n") if l and not l.startswith(b"@")]


def test_product_fastq_library_behind_a_fasta_library(built_lib, tmp_path):
    """the input format is set for every library: the stream belongs to the session"""
    fa = _put(tmp_path, "a.fa", _golden_text("se.fa"))
    fq = _put(tmp_path, "b.fq", _golden_text("se.fq"))
    log, got = _run(["-f", fa, fq], str(tmp_path / "a.sam"))
    assert log.count("device stream:") == 2, log[-600:]
    _, want = _run(["-f", fa, fq], str(tmp_path / "b.sam"), {"KART_AMD_NO_STREAM": "1"})
    assert got == want
    body = lambda t: [l for l in t.split(b"\n") if l and not l.startswith(b"@")]
    assert body(got) == body(_golden_text("se_fasta.sam")) + body(_golden_text("se.sam"))
