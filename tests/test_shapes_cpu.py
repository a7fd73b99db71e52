"""CPU: the indel-shape fixture (tests/golden/sam/shape_*; oracle/make_golden_shapes.py).  tests/report_plain.py -- GenMappingReport for one candidate, a
column at a time -- reproduces the reference's SAM line of EVERY read of the fixture under -g 5 and -g 20 (every read has exactly one candidate), so the
shape descriptors it leaves are those of the reference's own alignments; the classes counted from them on the committed reads equal the committed
class table and meet their least counts; the classes of shape_fixture.wanted_classes() that cannot occur hold no read.  (The host pipeline on the three SAMs:
tests/test_host_pipeline.py, cases shape_se, shape_pe, shape_se_g20.)"""
import os

import numpy as np
import pytest

import report_plain as P
import shape_fixture as S


@pytest.fixture(scope="module")
def shape(oracle_small):
    """the committed reads and the model's report of each under both MaxGaps (computed once, shared, never modified)"""
    names, s1, s2 = S.load_reads()
    gen = S.plain_genome(oracle_small)
    reports = {run: [S.model(oracle_small, gen, r, mg) for r in s1] for run, mg in S.RUNS.items()}
    return {"names": names, "reads": s1, "mates": s2, "gen": gen, "reports": reports, "lim": S.limits()}


def test_fixture_sizes(shape):
    assert len(shape["names"]) == len(set(shape["names"])) < 2500                 # ONE chunk of the reference, single-end and paired (2 x 2500 > 4000 would not be:
    assert 2 * len(shape["names"]) <= 4000                                        #  the paired library stays below 4000 reads too)
    assert {len(r) for r in shape["reads"]} == {150, 300}
    assert all(len(a) == len(b) for a, b in zip(shape["reads"], shape["mates"]))
    for f in ("shape_1.fq.gz", "shape_2.fq.gz", "shape_se.sam.gz", "shape_pe.sam.gz", "shape_se_g20.sam.gz"):
        assert os.path.getsize(os.path.join(S.SAM, f)) < 300000, f
        assert os.path.getsize(os.path.join(S.SAM, f)) <= max(os.path.getsize(os.path.join(S.SAM, g)) for g in ("rep_1.fq.gz", "rep_2.fq.gz", "rep.sam.gz", "rep_m.sam.gz")), f
    assert os.path.getsize(S.CLASS_TABLE) < 300000
    assert len(S.sam_lines(S.load_sam("shape_pe"))) == 2 * len(shape["names"])


@pytest.mark.parametrize("run", sorted(S.RUNS))
def test_report_plain_reproduces_the_reference(run, shape):
    """strand, RNAME, POS, CIGAR, AS and NM of every read, none left out"""
    lines = S.sam_lines(S.load_sam("shape_" + run))
    assert len(lines) == len(shape["names"])
    for name, read, rep in zip(shape["names"], shape["reads"], shape["reports"][run]):
        assert rep is not None, (name, "not exactly one candidate")
        assert S.model_columns(rep, len(read)) == S.line_columns(lines[(name, 0)]), (run, name)


def test_class_table_and_least_counts(shape):
    """Counted on the committed reads (688) through the oracle and report_plain under -g 5; the committed table says the same.  Each class holds at
    least 4 reads (2 where strand or contig is itself the class); the generator kept a read while one of its classes held fewer than 8, and a read
    counts for every class it has."""
    lim = shape["lim"]
    table = S.load_class_table()
    wanted = S.wanted_classes(lim)
    count = {c: 0 for c in wanted}
    assert set(table) == set(shape["names"])
    for name, rep in zip(shape["names"], shape["reports"]["se"]):
        reverse, contig = S.strand_and_contig(name)
        cls = S.fixture_classes(rep, lim, reverse, contig)
        assert cls == table[name], (name, sorted(cls ^ table[name]))
        assert cls, name
        for c in cls:
            count[c] += 1
    print("reads per class:", " ".join("%s=%d" % kv for kv in sorted(count.items())))
    for c, least in wanted.items():
        if c in S.UNREACHABLE:
            assert count[c] == 0, (c, count[c])
        else:
            assert count[c] >= least, (c, count[c], least)
    strands = {S.strand_and_contig(n) for n in shape["names"]}
    assert strands == {(False, "chrA"), (True, "chrA"), (False, "chrB"), (True, "chrB")}


def _end_clip(rep, role):
    """the soft clip the printed CIGAR shows at the read's head / tail (0 without one): the CIGAR runs backwards on the reverse strand"""
    import re
    ops = re.findall(r"(\d+)([MIDS])", rep["cigar"])
    n, op = ops[0 if (role == "head") == rep["fwd"] else -1]
    return int(n) if op == "S" else 0


def test_length_thresholds_and_long_ends_hold_passing_alignments(shape):
    """A head of 50 / a tail of 100 read bases is aligned, one of 51 / 101 is clipped -- and a whole-fragment S after a FAILED quality check would look the
    same.  So the classes at the limit hold only pairs whose alignment passes (no clip of the whole pair in the printed CIGAR), the classes one above it
    only pairs that are clipped although their alignment would have passed; the long heads and tails (the most tiles the finish pass walks for an end
    pair) pass as well, four or more of each with a trimmed run.  From the committed table and the model's descriptors, which the test above holds to
    the reference's lines."""
    table, n = S.load_class_table(), {}
    for name, rep in zip(shape["names"], shape["reports"]["se"]):
        for role, r, limit in (("head", "H", 50), ("tail", "T", 100)):
            ds = [d for d in rep["shapes"] if d["role"] == role]
            at, above, long_, trim = ("%s.rLen%d" % (r, limit), "%s.rLen%d" % (r, limit + 1), r + ".long", r + ".long+trim")
            for c in table[name] & {at, above, long_, trim}:
                n[c] = n.get(c, 0) + 1
                assert len(ds) == 1 and rep["score"] > 0, (name, c)
            if not ds:
                continue
            d = ds[0]
            if at in table[name]:
                assert d["rLen"] == limit and d["decided"] == "aligned" and d["ok"] and _end_clip(rep, role) == d["trim"][1] < limit, (name, at)
            if above in table[name]:
                assert d["rLen"] == limit + 1 and d["decided"] == "S-length" and d["ok_if_aligned"] and _end_clip(rep, role) == limit + 1, (name, above)
            if long_ in table[name]:
                tiles = -(-d["L"] // S.TILE)
                assert d["decided"] == "aligned" and d["ok"] and tiles >= (6 if r == "H" else 12) and _end_clip(rep, role) == d["trim"][1], (name, long_)
            if trim in table[name]:
                assert long_ in table[name] and sum(d["trim"]) > 0, (name, trim)
    print("reads per class:", sorted(n.items()))
    assert all(n.get("%s%s" % (r, c), 0) >= 4 for r in "HT" for c in (".long", ".long+trim")) and all(n.get(c, 0) >= 4 for c in ("H.rLen50", "H.rLen51", "T.rLen100", "T.rLen101")), n


def test_classes_that_cannot_occur(shape, oracle_small):
    """oracle/make_golden_shapes.py's docstring: a head pair has at least 8 bases and a middle pair's read side has 1 base or at least 9 because every
    7-mer occurs in the text (a search runs as long as the read's bases occur ANYWHERE, and the next one starts one base behind it); no middle pair is
    without read bases; no head has leading gaps on both sides.  Asserted on every aligned pair of the fixture, under both MaxGaps, whatever its class."""
    text = np.frombuffer(shape["gen"].text, np.uint8)
    code = np.full(256, 4, np.int64)
    for k, c in enumerate(b"ACGT"):
        code[c] = k
    v = code[text]
    kmers = sum(v[i:len(v) - 6 + i] * 4 ** i for i in range(7))
    assert (v < 4).all() and len(np.unique(kmers)) == 4 ** 7
    for run in S.RUNS:
        for rep in shape["reports"][run]:
            for d in rep["shapes"]:
                if d["role"] == "head":
                    assert d["rLen"] >= 8
                    if d["decided"] == "aligned" and d["ok"]:
                        assert not (d["trim"][0] > 0 and d["trim"][1] > 0)
                if d["role"] == "middle":
                    assert d["rLen"] == 1 or d["rLen"] >= 9 or (d["rLen"] > 0 and d["decided"] == "I")
                    assert d["rLen"] > 0
                    if run == "se" and d["decided"] == "aligned":
                        assert d["L"] != S.TILE


def test_envelope_limits_come_from_the_sources(shape):
    lim = shape["lim"]
    assert lim["cigar_text"] + 1 > 40 and lim["seeds"] > lim["gaps"] > 0
    reasons = [S.host_reason(rep, lim) for rep in shape["reports"]["se"]]
    table = S.load_class_table()
    for name, why in zip(shape["names"], reasons):
        envelope_only = all(c.startswith("E.") for c in table[name])
        assert (why is not None) <= envelope_only, name
    assert {6, 7, 10} <= set(reasons)


def test_plain_pieces_on_hand_made_alignments():
    """the column loops on strings small enough to check by eye"""
    a1, a2 = b"--ACGT-A", b"TTAC-TCA"
    assert P.column_classes(a1, a2) == list("DDMMIMDM")
    assert P.class_runs(a1, a2) == [("D", 0, 2), ("M", 2, 2), ("I", 4, 1), ("M", 5, 1), ("D", 6, 1), ("M", 7, 1)]
    assert P.local_alignment_quality(a1, a2) == (False, 6, 4, 0)
    cig = []
    assert P.add_new_cigar_elements(a1, a2, cig) == 4 and cig == [(2, "D"), (2, "M"), (1, "I"), (1, "M"), (1, "D"), (1, "M")]
    assert P.generate_cigar([(3, "M"), (2, "M"), (1, "I"), (4, "M")]) == "5M1I4M"
    assert P.local_alignment_quality(b"ACGTACGTAC", b"TGCTACGTAC") == (False, 1, 10, 3)       # 3 >= (int)(10 * 0.3)
    assert P.local_alignment_quality(b"ACGTACGTACGTAC", b"TGCTACGTACGTAC") == (True, 1, 14, 3)  # 3 < (int)(14 * 0.3)
    assert P.within_mismatch_rule(4, 4, b"ACGT", b"ACGA") == (False, 1) and P.within_mismatch_rule(5, 5, b"ACGTA", b"ACGAA") == (True, 1)
    assert P.within_mismatch_rule(10, 10, b"ACGTACGTAC", b"TCGTACGTAG") == (True, 2) and P.within_mismatch_rule(9, 9, b"ACGTACGTA", b"TCGTACGTT") == (False, 2)
    assert (P.leading(b"--A-"), P.trailing(b"--A-"), P.leading(b"A"), P.trailing(b"")) == (2, 1, 0, 0)
