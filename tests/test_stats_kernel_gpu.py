"""GPU: stats_tally_kernel (kart_amd/csrc/stats_kernels.hip) through kg_tally_records, on records no mapping run produces: every shape at which the
kernel can go wrong -- chunks of 1, 2, 4000 and 4000 + 2 reads, a chunk handed back whole, records that print nothing, -m chains through `next` into the
records behind the reads, every FLAG bit, the MAPQ and insert-size bins' edges, the shortest and longest CIGAR text, 4000 identical reads on one bin --
against a recount of the same records in Python (tests/stats_plain.py counts; this file only says what each record prints).  Rows are equal word for
word.  No index is needed."""
import numpy as np
import pytest

import stats_plain

pytestmark = pytest.mark.gpu

NONE, UNMAPPED, MAPPED, HOST = 0, 1, 2, 3
CIGAR_MAX = 48


def rec(kind=MAPPED, flag=0, mapq=60, tlen=0, has_mate=0, cigar=b"100M"):
    return (kind, flag, mapq, tlen, has_mate, cigar)


def layout(chains, tails_reversed=True):
    """chains[r]: the records printed for read r, its own first -> (ALN_DT array, n_reads): the own records in front, the others behind them, linked
    through `next`; tails_reversed: the later reads' tails lie first, so that a chain's tail is nowhere near its read"""
    from kart_amd import api
    n = len(chains)
    order = [(r, k) for r in (reversed(range(n)) if tails_reversed else range(n)) for k in range(1, len(chains[r]))]
    at = {rk: n + i for i, rk in enumerate(order)}
    a = np.zeros(n + len(order), dtype=api.ALN_DT)
    a["next"] = -1
    for r, chain in enumerate(chains):
        for k, (kind, flag, mapq, tlen, has_mate, cigar) in enumerate(chain):
            i = r if k == 0 else at[(r, k)]
            a[i]["kind"], a[i]["flag"], a[i]["mapq"], a[i]["tlen"], a[i]["has_mate"] = kind, flag, mapq, tlen, has_mate
            assert len(cigar) < CIGAR_MAX
            a[i]["cigar"], a[i]["cigar_len"] = cigar, len(cigar)
            a[i]["pos"], a[i]["mate_pos"], a[i]["score"] = 1000 + i, 2000 + i, 90
            if k + 1 < len(chain):
                a[i]["next"] = at[(r, k + 1)]
    return a, n


def printed(r):
    """the SAM columns stats_plain counts, of one record that is printed"""
    kind, flag, mapq, tlen, has_mate, cigar = r
    if kind == UNMAPPED:
        return [b"r", b"%d" % flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0"]
    return [b"r", b"%d" % flag, b"c", b"1", b"%d" % mapq, cigar or b"*", b"=" if has_mate else b"*", b"1" if has_mate else b"0", b"%d" % (tlen if has_mate else 0)]


def recount(chains, chunk_off):
    rows = []
    for c in range(len(chunk_off) - 1):
        cnt = stats_plain.Count()
        for chain in chains[chunk_off[c]:chunk_off[c + 1]]:
            if chain[0][0] == HOST:
                continue                # the caller's read: nothing of it is counted here
            for r in chain:
                if r[0] in (UNMAPPED, MAPPED):
                    cnt.add(printed(r))
        rows.append(stats_plain.row_of(cnt))
    return np.array(rows, dtype=np.uint32).reshape(len(chunk_off) - 1, stats_plain.WORDS)


def check(chains, chunk_off, **kw):
    from kart_amd import api
    a, n = layout(chains, **kw)
    rows = api.tally_records(a, n, chunk_off)
    want = recount(chains, chunk_off)
    assert rows.shape == want.shape and rows.dtype == np.uint32
    bad = np.argwhere(rows != want)
    assert bad.size == 0, [(int(c), int(w), int(rows[c, w]), int(want[c, w])) for c, w in bad[:8]]
    return rows


LONGEST = b"1S2M3I4D5M6I7D8M9S10M11I12D13M14N15M16H17M18=9X"          # 47 characters
assert len(LONGEST) == CIGAR_MAX - 1

EDGE_RECORDS = (
    [rec(flag=1 << b) for b in range(12)] + [rec(flag=0xfff), rec(flag=0), rec(UNMAPPED, flag=4), rec(UNMAPPED, flag=0x4 | 0x1 | 0x8 | 0x40), rec(UNMAPPED, flag=0x85)] +
    [rec(flag=99, has_mate=1, tlen=200), rec(flag=147, has_mate=1, tlen=-200), rec(flag=73), rec(flag=0x900 | 1, has_mate=1, tlen=5)] +
    [rec(mapq=q) for q in (0, 1, 59, 60, 62, 63, 64, 255)] +
    [rec(flag=97, has_mate=1, tlen=t) for t in (1, 2, 2047, 2048, 2049, 100000, 0, -1, -300)] +
    [rec(flag=97, has_mate=0, tlen=t) for t in (1, 300, 2048)] +          # no mate: RNEXT is "*", not an insert size
    [rec(flag=0, has_mate=1, tlen=300)] +                                 # not paired: neither
    [rec(cigar=c) for c in (b"M", b"1M", b"150M", LONGEST, b"10M5N10M", b"3H40M", b"20=1X20=", b"5S90M2I3D53M", b"0M", b"999999M", b"")] +
    [rec(UNMAPPED, flag=4, mapq=37, tlen=99, has_mate=1, cigar=b"77M"),    # an unmapped-kind record prints none of its other fields ...
     rec(UNMAPPED, flag=1, mapq=37, tlen=99, has_mate=1, cigar=b"77M"),    # ... even where its FLAG lacks the bit
     rec(NONE, flag=99, has_mate=1, tlen=5), rec(HOST, flag=99, has_mate=1, tlen=5)])


PRINTED = [r for r in EDGE_RECORDS if r[0] in (UNMAPPED, MAPPED)]


def varied(n, seed):
    """n reads drawn from the edge records, chains of 1, 2 and 9 records among them"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(EDGE_RECORDS), n)
    chains = []
    for r in range(n):
        length = 9 if r % 97 == 5 else 2 if r % 7 == 3 else 1
        # (behind a read's own record only records that are printed: a handed-back read has no chain)
        chains.append([EDGE_RECORDS[int(pick[r])]] + [PRINTED[(int(pick[r]) + 5 * k) % len(PRINTED)] for k in range(1, length)])
    return chains


def test_the_row_layout_is_the_documented_one():
    from kart_amd import api
    assert (api.KG_STATS_RECORDS, api.KG_STATS_FLAG0, api.KG_STATS_PROPER, api.KG_STATS_BOTH_MAPPED, api.KG_STATS_SINGLETON, api.KG_STATS_CIGAR0, api.KG_STATS_MAPQ0,
            api.KG_STATS_ISIZE0, api.KG_STATS_WORDS) == (stats_plain.RECORDS, stats_plain.FLAG0, stats_plain.PROPER, stats_plain.BOTH_MAPPED, stats_plain.SINGLETON,
                                                         stats_plain.CIGAR0, stats_plain.MAPQ0, stats_plain.ISIZE0, stats_plain.WORDS)


@pytest.mark.parametrize("k", range(len(EDGE_RECORDS)), ids=lambda k: "rec%d" % k)
def test_one_chunk_of_one_read(k):
    rows = check([[EDGE_RECORDS[k]]], [0, 1])
    assert rows[0, 0] == (1 if EDGE_RECORDS[k][0] in (UNMAPPED, MAPPED) else 0)


def test_one_chunk_of_two_reads():
    check([[EDGE_RECORDS[17]], [EDGE_RECORDS[18]]], [0, 2])
    check([[EDGE_RECORDS[17], EDGE_RECORDS[40]], [EDGE_RECORDS[2]] * 9], [0, 2])


def test_every_edge_record_in_one_chunk_and_one_per_chunk():
    chains = [[r] for r in EDGE_RECORDS]
    check(chains, [0, len(chains)])
    check(chains, list(range(len(chains) + 1)))


def test_4000_reads():
    rows = check(varied(4000, 1), [0, 4000])
    assert rows[0, 0] > 4000                                 # (the chains' records count too)


def test_4000_and_2_reads_as_two_chunks():
    chains = varied(4002, 2)
    chains[4000:] = [[rec(flag=83, has_mate=1, tlen=-412)], [rec(flag=163, has_mate=1, tlen=412), rec(flag=163 | 256, has_mate=1, tlen=2048)]]
    rows = check(chains, [0, 4000, 4002])
    assert rows[1, 0] == 3 and rows[1, stats_plain.ISIZE0 + 412] == 1 and rows[1, stats_plain.ISIZE0 + 2048] == 1


def test_a_middle_chunk_handed_back_whole_gives_a_zero_row():
    chains = varied(900, 3)
    rng = np.random.default_rng(33)
    for r in range(300, 600):
        chains[r] = [rec(HOST, flag=int(rng.integers(0, 4096)), has_mate=1, tlen=int(rng.integers(1, 3000)), mapq=int(rng.integers(0, 70)))]
    rows = check(chains, [0, 300, 600, 900])
    assert not rows[1].any() and rows[0].any() and rows[2].any()


def test_a_handed_back_record_carries_no_link():
    """its `next` is whatever the slot held: nothing behind it is read"""
    from kart_amd import api
    chains = [[rec(HOST)], [rec(flag=16)], [rec(flag=0), rec(flag=256)]]
    a, n = layout(chains)
    a[0]["next"] = 3                                         # (the third read's second record)
    rows = api.tally_records(a, n, [0, 3])
    assert (rows == recount(chains, [0, 3])).all() and rows[0, 0] == 3
    # ... and a link that leaves the records behind the reads ends its chain
    for stray in (0, 1, 4, -7, 2 ** 31 - 1):
        a[1]["next"] = stray
        assert (api.tally_records(a, n, [0, 3]) == rows).all()


def test_records_that_print_nothing():
    chains = [[rec(NONE)] if r % 3 == 0 else [EDGE_RECORDS[r % len(EDGE_RECORDS)]] for r in range(500)]
    chains[7] = [rec(NONE), rec(flag=16), rec(flag=256)]     # (the chain behind such a record is still walked, as the printer walks it)
    rows = check(chains, [0, 256, 500])
    assert rows[:, 0].sum() < 500


@pytest.mark.parametrize("reversed_tails", [False, True])
def test_chains_of_1_2_and_9_records_across_chunks(reversed_tails):
    """a chain's records count for the chunk of its read, wherever they lie behind the reads"""
    chains = []
    for r in range(24):
        length = (1, 2, 9)[r % 3]
        chains.append([rec(flag=(0 if k == 0 else 256) | (16 if r & 1 else 0), mapq=r, cigar=b"%dM" % (r + 1)) for k in range(length)])
    rows = check(chains, [0, 8, 16, 24], tails_reversed=reversed_tails)
    assert [int(x) for x in rows[:, 0]] == [sum(len(c) for c in chains[i:i + 8]) for i in (0, 8, 16)]
    for r in range(24):
        assert rows[r // 8, stats_plain.MAPQ0 + r] == len(chains[r])


@pytest.mark.parametrize("record", [rec(flag=99, mapq=60, has_mate=1, tlen=300, cigar=b"150M"), rec(UNMAPPED, flag=77), rec(flag=97, has_mate=1, tlen=9999, mapq=255, cigar=LONGEST)],
                         ids=["mapped", "unmapped", "overflow_bins"])
def test_4000_identical_reads_on_one_bin(record):
    rows = check([[record]] * 4000, [0, 4000])
    assert rows[0, 0] == 4000 and rows[0].max() >= 4000


def test_empty_chunks_and_no_chunks():
    from kart_amd import api
    rows = check([[EDGE_RECORDS[0]]] * 5, [0, 0, 5, 5])
    assert not rows[0].any() and not rows[2].any() and rows[1, 0] == 5
    assert api.tally_records(np.zeros(0, dtype=api.ALN_DT), 0, [0]).shape == (0, api.KG_STATS_WORDS)
    with pytest.raises(api.KartAmdError):
        api.tally_records(np.zeros(3, dtype=api.ALN_DT), 3, [0, 4])          # a chunk beyond the reads
