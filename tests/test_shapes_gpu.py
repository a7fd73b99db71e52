"""GPU: the planning and finish kernels of the alignment stage (aln_plan_fast_kernel, aln_plan_kernel, aln_partition_kernel, aln_finish_group_kernel) on the
indel-shape fixture (tests/golden/sam/shape_*; tests/test_shapes_cpu.py asserts the classes it holds): every record of the whole fixture against the
reference's line, single-end under -g 5 and -g 20 and paired; the reads handed back are exactly the fixture's envelope classes, by reason; the same eight
reads in every position of a wave and in batches on both sides of a wave's size.  (Through the product binary: tests/test_sam_gpu.py, cases shape_*.)"""
from collections import Counter

import numpy as np
import pytest

import rep_fixture as F
import shape_fixture as S
from aln_records import chain_of, compare_pairs_with_reference, line_columns, record_columns
from test_host_pipeline import UNSET_FLAG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shape(gpu_index_full, oracle_small):
    """the committed reads, the model's report and the oracle's candidates of each under both MaxGaps (computed once, shared, never modified), one workspace"""
    names, s1, s2 = S.load_reads()
    gen, lim = S.plain_genome(oracle_small), S.limits()
    cands = {mg: [S.map_read(oracle_small, r, mg) for r in s1] for mg in set(S.RUNS.values())}
    reports = {mg: [S.model(oracle_small, gen, r, mg) for r in s1] for mg in set(S.RUNS.values())}
    ws = gpu_index_full.workspace(16384, 4 << 20)
    d = {"ix": gpu_index_full, "names": names, "single": [np.frombuffer(r, np.uint8) for r in s1], "reads": F.held_reads(s1, s2), "never": set(), "lim": lim,
         "cands": cands, "reports": reports, "why": {mg: [S.host_reason(r, lim) for r in reports[mg]] for mg in reports}, "table": S.load_class_table(), "ws": ws}
    yield d
    ws.close()


def _align(shape, reads, paired=False, max_gaps=5):
    """seed_batch (characters) + candidates_batch + align_batch on the reads as ONE chunk -> (records, chunk_stats[0], candidates per read, growth of align_reasons())"""
    from kart_amd import api
    ws = shape["ws"]
    chars, off = api.concat_reads(reads)
    so, _ = ws.seed_batch(chars, off, api.KG_MODE_FAST | api.KG_INPUT_ASCII)
    cands = ws.candidates_batch(so, False, max_gaps)
    before = ws.align_reasons()
    recs, stats = ws.align_batch([0, len(reads)], [1 if paired else 0], est_distance=1500, max_insert=1500, max_gaps=max_gaps, multi_hit=False, unset_flag=UNSET_FLAG)
    return recs, stats[0], cands, (ws.align_reasons() - before).astype(np.int64)[:13]


def _same_candidates(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for (gs, gp, gv), (ws_, wp, wv) in zip(got, want):
        assert (gs, gp) == (ws_, wp), what
        assert len(gv) == len(wv) and (gv["gPos"] == wv["gPos"]).all() and (gv["rPos"] == wv["rPos"]).all() and (gv["len"] == wv["rLen"]).all(), what


def _expected_reasons(why):
    want = np.zeros(13, np.int64)
    for w, n in Counter(x for x in why if x is not None).items():
        want[w] = n
    return want


def _single_key(shape, rec, rlen):
    """everything a read's record says, for the comparison between arrangements"""
    from kart_amd import api
    if rec["kind"] == api.KG_ALN_HOST:
        return "host"
    return record_columns(shape, rec, rlen) + (int(rec["kind"]), int(rec["flip"]), int(rec["primary"]), int(rec["next"]))


@pytest.fixture(scope="module")
def whole(shape):
    """the whole fixture as one single-end chunk under each MaxGaps"""
    return {run: _align(shape, shape["single"], False, mg) for run, mg in S.RUNS.items()}


@pytest.mark.parametrize("run", sorted(S.RUNS))
def test_single_end_records_equal_the_reference(run, shape, whole):
    """FLAG, RNAME, POS, MAPQ, CIGAR, the mate columns, AS, XS, NM and the strand shown of every read; a read is handed back exactly when the model puts it
    outside the envelope (13 seeds, 9 gap pairs, a CIGAR text one character too long), under the reason that says so and no other; the 8-gap and
    longest-CIGAR reads are decided here; the candidates are the oracle's.
    A candidate of exactly 12 seeds is NOT decided here, and cannot be: two searches of IdentifySeedPairs_FastMode never touch in the read (the next one
    starts one base behind the last, src/AlignmentCandidates.cpp:74), so 12 seeds have 11 gap pairs between them and the read goes back under [7]; only
    the 13-seed reads, which aln_plan_kernel refuses before it counts gap pairs, go back under [6]."""
    from kart_amd import api, synth
    mg = S.RUNS[run]
    recs, stats, cands, reasons = whole[run]
    sam = F.sam_records(S.load_sam("shape_" + run))
    why = shape["why"][mg]
    differ = []                                                   # (every differing read is shown, the shortest first: the smallest read that shows a fault)
    for k, name in enumerate(shape["names"]):
        _same_candidates(cands[k], shape["cands"][mg][k], (run, name))
        if (recs[k]["kind"] == api.KG_ALN_HOST) != (why[k] is not None):
            differ.append((len(shape["single"][k]), name, "kind %d, expected reason %s" % (int(recs[k]["kind"]), why[k]), sorted(shape["table"][name])))
        if why[k] is not None or recs[k]["kind"] == api.KG_ALN_HOST:
            continue
        read, lines, chain = shape["single"][k], sam.get((name, 0), []), chain_of(recs, k)
        assert len(chain) == len(lines) == 1, (run, name, len(chain), len(lines))
        got, want = record_columns(shape, chain[0], len(read)), line_columns(lines[0][1])
        if got != want:
            differ.append((len(read), name, got, want, sorted(shape["table"][name])))
        elif chain[0]["kind"] == api.KG_ALN_MAPPED:
            assert lines[0][1][9] == (synth.revcomp(read) if chain[0]["flip"] else read).tobytes(), (run, name)
    print("reasons (%s):" % run, reasons.tolist())
    assert not differ, (len(differ), sorted(differ)[:12])
    assert (reasons == _expected_reasons(why)).all(), (reasons.tolist(), _expected_reasons(why).tolist())
    assert int(stats["host_pairs"]) == sum(1 for w in why if w is not None)
    if run == "se":
        lim, table = shape["lim"], shape["table"]
        for cls, reason in (("E.seeds%d" % (lim["seeds"] + 1), 6), ("E.gaps%d" % (lim["gaps"] + 1), 7), ("E.cigar-over", 10)):
            members = [k for k, n in enumerate(shape["names"]) if cls in table[n]]
            assert len(members) >= 4 and all(why[k] == reason for k in members), cls
        for cls in ("E.gaps%d" % lim["gaps"], "E.cigar-longest"):
            members = [k for k, n in enumerate(shape["names"]) if cls in table[n] and why[k] is None]
            assert len(members) >= 4, cls                       # (decided on the device and equal to the reference: the loop above)
        members = [k for k, n in enumerate(shape["names"]) if "E.seeds%d" % lim["seeds"] in table[n]]
        assert len(members) >= 4 and all(why[k] == 7 and shape["reports"][mg][k]["gap_pairs"] == lim["seeds"] - 1 for k in members)
        assert sorted({w for w in why if w is not None}) == [6, 7, 10]


def test_paired_records_equal_the_reference(shape):
    """the fixture with its error-free mates as one paired chunk under EstDistance 1500: both records of every pair, the mate columns among them; a pair
    comes back exactly when its mate 1 is outside the envelope"""
    n = len(shape["names"])
    recs, stats, cands, reasons = _align(shape, shape["reads"], True, 5)
    for k in range(n):
        _same_candidates(cands[2 * k], shape["cands"][5][k], shape["names"][k])
    host = compare_pairs_with_reference(shape, F.sam_records(S.load_sam("shape_pe")), list(range(n)), recs, False)
    why = shape["why"][5]
    print("reasons (pe):", reasons.tolist())
    assert host == [k for k in range(n) if why[k] is not None]
    assert (reasons == _expected_reasons(why)).all(), (reasons.tolist(), _expected_reasons(why).tolist())
    assert int(stats["host_pairs"]) == 2 * len(host)


def _eight_of_different_shapes(shape):
    """eight reads decided on the device whose candidates differ in the pairs they hold and in which of them are aligned (the eight groups of a wave diverge)"""
    picked, seen = [], set()
    for k, rep in enumerate(shape["reports"][5]):
        if shape["why"][5][k] is not None or rep["score"] <= 0:
            continue
        sig = (rep["seeds"],) + tuple((d["role"], d["decided"]) for d in rep["shapes"])
        if sig in seen or not any(d["decided"] == "aligned" for d in rep["shapes"]):
            continue
        if len({s[1:] for s in seen} | {sig[1:]}) == len(seen) + 1:          # (the roles and decisions differ, not only the number of seeds)
            seen.add(sig)
            picked.append(k)
        if len(picked) == 8:
            break
    assert len(picked) == 8 and len({shape["reports"][5][k]["seeds"] + len(shape["reports"][5][k]["shapes"]) for k in picked}) >= 3, picked
    return picked


def test_records_do_not_depend_on_the_place_in_the_wave(shape, whole):
    """Eight lanes take a candidate, a wave holds eight groups and every ballot is shifted by the group's first lane.  Eight reads of eight different shapes in
    all eight rotations; alone; in batches of 7, 9, 64 and 65 shape reads; interleaved one to one with error-free reads (the plan kernels list the others
    densely); as the last reads behind 60 error-free ones.  Every read's record equals the whole-fixture run's -- which the test above holds to the reference."""
    _, seqs = S.genome()
    recs = whole["se"][0]
    key = [_single_key(shape, recs[k], len(shape["single"][k])) for k in range(len(shape["names"]))]
    eight = _eight_of_different_shapes(shape)
    others = [k for k in range(len(shape["names"])) if k not in eight]
    pool = eight + others
    clean = [seqs["chrA"][1000 + 137 * i:1150 + 137 * i] for i in range(60)]
    arrangements = {"rotation_%d" % r: eight[r:] + eight[:r] for r in range(8)}
    arrangements.update({"alone_%d" % i: [k] for i, k in enumerate(eight)})
    arrangements.update({"batch_%d" % n: pool[:n] for n in (7, 9, 64, 65)})
    arrangements.update({"interleaved": [x for k in eight for x in (k, None)], "shifted": [None] + [x for k in eight for x in (k, None)], "last_behind_60": [None] * 60 + eight})
    for name, idx in arrangements.items():
        reads, c = [], 0
        for k in idx:
            if k is None:
                reads.append(clean[c])
                c += 1
            else:
                reads.append(shape["single"][k])
        got, _, _, _ = _align(shape, reads, False, 5)
        for at, k in enumerate(idx):
            if k is None:
                assert bytes(got[at]["cigar"])[:int(got[at]["cigar_len"])] == b"150M", (name, at)
            else:
                assert _single_key(shape, got[at], len(reads[at])) == key[k], (name, at, shape["names"][k], sorted(shape["table"][shape["names"][k]]))
