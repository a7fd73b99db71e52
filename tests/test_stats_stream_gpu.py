"""GPU: the tally of a batch's records made by the device inside kg_stream_map (kg_stream_set_stats; stats_tally_kernel in kart_amd/csrc/stats_kernels.hip).
The expectation needs no model of the mapper: a chunk's row is the plain recount (tests/stats_plain.py) of the chunk's lines of the SAM text of the SAME
map() call, the reads handed back left out -- their records are the caller's to count.  Chunks are eight reads here, so that a small batch has many rows."""
import numpy as np
import pytest

import stats_plain
from test_bam_stream_gpu import fastq, genome, ref_ids  # noqa: F401  (fixtures and builders of the BAM stream test)
from test_md_stream_gpu import multi_hit_batch
from test_un_stream_gpu import build, seedless  # noqa: F401

pytestmark = pytest.mark.gpu

CHUNK = 8


@pytest.fixture(scope="module")
def stream(gpu_index_full):
    from kart_amd import api
    s = api.Stream(gpu_index_full, max_reads=16000, max_window=8 << 20, lanes=1)
    yield s
    s.close()


def run(stream, texts, n_reads, paired, multi_hit=False, stats=True):
    """one batch -> (SAM text per read, reads handed back, last_stats())"""
    try:
        stream.set_stats(stats)
        p = stream.parse(texts[0], texts[1] if len(texts) > 1 else None, paired=paired, chunk_reads=CHUNK, want_reads=(n_reads + CHUNK - 1) // CHUNK * CHUNK)
        assert (p.n_reads, p.stop, p.done) == (n_reads, 0, 1)
        sam, host = stream.map(multi_hit=multi_hit)
        return sam, host, stream.last_stats()
    finally:
        stream.set_stats(False)


def check(sam, host, rows, max_host=None):
    """every chunk's row against the plain recount of its lines; -> the rows' sum"""
    n = len(sam)
    n_chunks = (n + CHUNK - 1) // CHUNK
    assert len(host) <= (n // 2 if max_host is None else max_host)
    assert rows is not None and rows.shape == (n_chunks, stats_plain.WORDS) and rows.dtype == np.uint32
    for c in range(n_chunks):
        text = b"".join(sam[r] for r in range(c * CHUNK, min(n, (c + 1) * CHUNK)) if r not in host)
        want = stats_plain.row(text)
        bad = np.flatnonzero(rows[c] != want)
        assert bad.size == 0, (c, [(int(w), int(rows[c, w]), int(want[w])) for w in bad[:8]])
    return rows.sum(axis=0, dtype=np.int64)


def test_paired_batch_with_a_partial_last_chunk(stream, genome, seedless):
    recs, meant = build(genome, seedless, 129, "alternating", pairs=True)          # 258 reads: 32 chunks and one of two reads
    sam, host, rows = run(stream, [fastq(recs)], len(recs), True)
    total = check(sam, host, rows)
    assert rows.shape[0] == 33 and rows[32, stats_plain.RECORDS] <= 2
    # a condition on the input: mapped pairs with insert sizes, and unmapped ones
    assert total[stats_plain.PROPER] > 20 and total[stats_plain.ISIZE0:].sum() > 10 and total[stats_plain.FLAG0 + 2] > 20
    assert total[stats_plain.CIGAR0] > 2000 and total[stats_plain.MAPQ0:stats_plain.ISIZE0].sum() == total[stats_plain.RECORDS] - total[stats_plain.FLAG0 + 2]


def test_two_files(stream, genome, seedless):
    recs, meant = build(genome, seedless, 65, "one_per_64", pairs=True)
    sam, host, rows = run(stream, [fastq(recs[0::2]), fastq(recs[1::2])], len(recs), True)
    total = check(sam, host, rows)
    assert total[stats_plain.BOTH_MAPPED] > 40


@pytest.mark.parametrize("n_reads", [1, 8, 9, 129])
def test_single_end(n_reads, stream, genome, seedless):
    recs, meant = build(genome, seedless, n_reads, "alternating", pairs=False)
    sam, host, rows = run(stream, [fastq(recs)], len(recs), False)
    total = check(sam, host, rows)
    assert total[stats_plain.FLAG0] == 0 and total[stats_plain.ISIZE0:].sum() == 0          # (no record is paired, none has an insert size)
    assert total[stats_plain.RECORDS] == sum(t.count(b"\n") for r, t in enumerate(sam) if r not in host) > 0


def test_multi_hit_chains_count_for_their_reads_chunk(stream, genome, seedless):
    chains = multi_hit_batch(genome)
    extra, meant = build(genome, seedless, 40, "alternating", pairs=True)
    recs = chains[:18] + extra + chains[18:]
    sam, host, rows = run(stream, [fastq(recs)], len(recs), True, multi_hit=True)
    assert any(t.count(b"\n") >= 2 for t in sam), "no read with two or more records"
    total = check(sam, host, rows)
    assert total[stats_plain.RECORDS] == sum(t.count(b"\n") for r, t in enumerate(sam) if r not in host) > len(recs) - len(host)


def test_a_chunk_of_random_reads_is_all_unmapped(stream, genome, seedless):
    mapped, _ = build(genome, seedless, CHUNK, "none", pairs=True)
    random_reads, _ = build(genome, seedless, CHUNK // 2, "all", pairs=True)          # one chunk of eight reads
    recs = mapped + random_reads + mapped[:6]
    sam, host, rows = run(stream, [fastq(recs)], len(recs), True)
    check(sam, host, rows)
    c = len(mapped) // CHUNK
    assert not any(r in host for r in range(c * CHUNK, (c + 1) * CHUNK))
    assert rows[c, stats_plain.RECORDS] == CHUNK == rows[c, stats_plain.FLAG0 + 2] == rows[c, stats_plain.FLAG0 + 3]
    assert rows[c, stats_plain.CIGAR0:].sum() == 0                                  # no CIGAR, no MAPQ, no insert size


def test_off_gives_no_rows_and_the_same_text_and_the_setting_leaves_no_trace(stream, genome, seedless):
    recs, meant = build(genome, seedless, 129, "alternating", pairs=True)
    texts = [fastq(recs)]
    off = run(stream, texts, len(recs), True, stats=False)
    assert off[2] is None                                    # kg_stream_result::chunk_tally is NULL
    on = run(stream, texts, len(recs), True)
    assert on[:2] == off[:2], "the SAM text changed under the setting"
    check(*on)
    again = run(stream, texts, len(recs), True, stats=False)
    assert again[2] is None and again[:2] == off[:2]
    once_more = run(stream, texts, len(recs), True)
    assert (once_more[2] == on[2]).all()


def test_the_kernel_is_timed_and_the_rows_are_counted(stream, genome, seedless):
    recs, _ = build(genome, seedless, 64, "none", pairs=True)
    stream.timing(reset=True)
    run(stream, [fastq(recs)], len(recs), True, stats=False)
    t = stream.timing(reset=True)
    assert t["stats_kernel_launches"] == 0 and t["stats_bytes"] == 0
    run(stream, [fastq(recs)], len(recs), True)
    t = stream.timing(reset=True)
    assert t["stats_bytes"] == 4 * stats_plain.WORDS * (len(recs) // CHUNK)
    assert t["stats_kernel_launches"] in (0, 1)             # (1 where the stream's workspaces are profiled)
