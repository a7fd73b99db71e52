"""GPU: the list of 16-byte chunks that sam_format_kernel, bam_format_kernel and un_copy_kernel share (chunk_list / for_each_chunk in
kart_amd/csrc/text_device.hpp) at its boundaries.  One batch of single-end reads, cut from the genome fixture at EVERY length from 32 to 97 -- every
residue mod 16 of the SAM chunks, every residue mod 32 of BAM's packed bases, odd and even l_seq -- each length once as cut and once reverse-complemented,
with six reads that stay unmapped among them: 138 reads, so the batch crosses the 64-read groups at 63 / 64 / 65 and 127 / 128 / 129 and ends in a group
of 10 whose last lane is an unmapped read.  Position i of a read carries the quality '!' + (i * 7 + length) % 90: a chunk moved to the wrong offset or
the wrong line shows."""
import numpy as np
import pytest

from bam_encode import bam_records_of_text
from test_bam_stream_gpu import fastq, genome, ref_ids  # noqa: F401  (fixtures and builders of the BAM stream test)
from test_un_stream_gpu import seedless  # noqa: F401

pytestmark = pytest.mark.gpu

LENGTHS = range(32, 98)
UNMAPPED_AT = (0, 63, 64, 65, 127, 137)
UNMAPPED_LEN = (40, 16, 17, 33, 150, 64)


def quals(length):
    return bytes(33 + (i * 7 + length) % 90 for i in range(length))


@pytest.fixture(scope="module")
def stream(gpu_index_full):
    from kart_amd import api
    s = api.Stream(gpu_index_full, max_reads=16000, max_window=8 << 20, lanes=1)
    yield s
    s.close()


@pytest.fixture(scope="module")
def batch(genome, seedless):
    from kart_amd import synth
    g = genome["chrB"]
    recs = []
    for k, length in enumerate(LENGTHS):
        p = 2000 + 211 * k
        piece = g[p:p + length]
        recs.append((b"w%d_as_cut" % length, bytes(piece), quals(length)))
        recs.append((b"w%d_rc" % length, bytes(synth.revcomp(piece)), quals(length)))
    assert len(recs) == 132
    for at, length in zip(UNMAPPED_AT, UNMAPPED_LEN):
        recs.insert(at, (b"random_at_%d" % at, seedless.read(length), quals(length)))
    assert len(recs) == 138 and all(recs[at][0].startswith(b"random") for at in UNMAPPED_AT)
    return recs


def run(stream, recs, fmt="sam", unmapped=False):
    """one parse + map of the batch -> (bytes per read, reads handed back, last_unmapped()); map() raises on any device format error (ctl[1])"""
    try:
        stream.set_format(fmt)
        stream.set_unmapped(unmapped)
        p = stream.parse(fastq(recs), None, paired=False, chunk_reads=8, want_reads=(len(recs) + 7) // 8 * 8)
        assert (p.n_reads, p.stop, p.done) == (len(recs), 0, 1)
        out, host = stream.map()
        return out, host, stream.last_unmapped()
    finally:
        stream.set_unmapped(False)
        stream.set_format("sam")


@pytest.fixture(scope="module")
def first(stream, batch):
    return run(stream, batch)


def test_sam_lines_carry_every_reads_bases_and_qualities(first, batch):
    from kart_amd import synth
    sam, host, un = first
    assert un == [] and len(sam) == len(batch)
    strands = {length: set() for length in LENGTHS}
    mapped = 0
    for i, (name, seq, qual) in enumerate(batch):
        if i in host:
            assert sam[i] == b""
            continue
        assert sam[i].endswith(b"\n") and sam[i].count(b"\n") == 1, (i, sam[i])
        f = sam[i][:-1].split(b"\t")
        assert f[0] == name
        if int(f[1]) & 16:
            assert (f[9], f[10]) == (bytes(synth.revcomp(np.frombuffer(seq, np.uint8))), qual[::-1]), (i, sam[i])
        else:
            assert (f[9], f[10]) == (seq, qual), (i, sam[i])
        if f[2] != b"*" and not name.startswith(b"random"):
            strands[len(seq)].add(int(f[1]) & 16)
            mapped += 1
    # (a condition on the input, not a measurement: the cut reads are decided on the device and map, the two of a length to either strand)
    assert mapped >= 120
    assert all(s == {0, 16} for s in strands.values()), {n: s for n, s in strands.items() if s != {0, 16}}


def test_bam_records_equal_the_encoded_sam_lines(stream, first, batch, ref_ids):
    sam, host, _ = first
    bam, host_b, _ = run(stream, batch, fmt="bam")
    assert host_b == host and len(bam) == len(sam)
    for i, (s, b) in enumerate(zip(sam, bam)):
        want = bam_records_of_text(s, ref_ids)
        assert b == want, (i, s[:200], b.hex(), want.hex())


def test_unmapped_text_is_the_six_random_records_and_the_settings_leave_no_trace(stream, first, batch):
    sam, host, un = run(stream, batch, unmapped=True)
    assert (sam, host) == first[:2]
    assert not any(at in host for at in UNMAPPED_AT)
    assert len(un) == 1
    data, off = un[0]
    assert data == fastq([batch[at] for at in UNMAPPED_AT])
    assert [u for u in range(len(batch)) if off[u + 1] > off[u]] == list(UNMAPPED_AT)
    again = run(stream, batch)
    assert again == first, "the output without the settings changed after runs with them"
