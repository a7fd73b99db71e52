"""GPU: the wave-cooperative forms of the chaining and pairing kernels on the repeat-family fixture (tests/golden/rep.fa.gz, tests/golden/sam/rep_*;
tests/test_rep_cpu.py asserts the classes it holds).  chain_read_wave (reads of 17..64 seeds) against the CPU oracle bit for bit, in every position
of a wave; pair_front_wave / pair_back_wave / rescue_windows_wave / remove_redundant_wave (pairs of more than 32 candidate pairs, the pre-pass
above 1000) through kg_align_batch against the reference's SAM record by record, in several arrangements of the same pairs; and every
alternative form of the stage (the KG_ALN_* / KG_RESCUE_SCAN switches) through the product binary against the same SAM."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import rep_fixture as F
from aln_records import chain_of as _chain_of, compare_pairs_with_reference, record_columns as _record_columns
from conftest import ROOT, SMALL_PREFIX
from test_host_pipeline import CASES, UNSET_FLAG, assert_sam_equals_reference_with_its_own_mask, materialise

pytestmark = pytest.mark.gpu
KART_AMD = os.path.join(ROOT, "kart_amd", "bin", "kart-amd")
ALLOWED_REASONS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10)


@pytest.fixture(scope="module")
def rep(built_lib, tmp_path_factory):
    """the index of the committed genome built on the device the tests run on, the held reads, their seeds and candidates from the CPU oracle
    (computed once, shared, never modified), the reference's records per read"""
    from kart_amd import api, synth
    from oracle import oracle as O
    if api.device_count() <= 0:
        pytest.fail("no HIP device visible: -m gpu tests must run on the GPU box (there is no CPU fallback)")
    tmp = str(tmp_path_factory.mktemp("rep"))
    prefix = F.build_rep_index(tmp, device=None)
    names, reads = F.load_reads()
    orc = O.Oracle(prefix)
    so, seeds, cands = F.oracle_chain(orc, reads)
    ix = api.Index(prefix, 0, api.KG_SA_FULL)
    never = F.never_assigned_lines()
    d = {"tmp": tmp, "prefix": prefix, "names": names, "reads": reads, "enc": [synth.encode(r) for r in reads], "so": so, "seeds": seeds, "cands": cands,
         "orc": orc, "ix": ix, "never": never, "sam": F.sam_records(F.load_sam("rep")), "sam_m": F.sam_records(F.load_sam("rep_m"), never)}
    yield d
    ix.close()
    orc.close()


# ---- chaining ------------------------------------------------------------------------------------------------------------------------------
def _chain_batches(ns):
    """read index lists: a heavy read (17..64 seeds: chain_read_wave's) alone, in lane 0 and in lane 63 of a wave of light reads, as the last read of a
    batch of 129, as all 64 reads of a wave, and next to reads of 16 and 65 seeds (the lanes' loop on both sides of the thresholds)"""
    pick = lambda m: [int(i) for i in np.flatnonzero(m)]
    heavy, light, big = pick((ns >= 17) & (ns <= 64)), pick(ns < 16), pick(ns > 65)
    s16, s17, s64, s65 = (pick(ns == k) for k in (16, 17, 64, 65))
    assert len(heavy) >= 64 and len(light) >= 128 and min(len(x) for x in (s16, s17, s64, s65)) >= 3
    mixed = [(light + big)[i % (len(light) + len(big))] for i in range(0, 128 * 3, 3)]
    edge = []
    for k in range(16):                                        # 64 lanes: 16, 17, 65, 64 seeds side by side
        edge += [s16[k % len(s16)], s17[k % len(s17)], s65[k % len(s65)], s64[k % len(s64)]]
    return {"alone": [heavy[0]], "alone_17": [s17[0]], "alone_64": [s64[0]], "lane_0": [heavy[1]] + light[:63], "lane_63": light[:63] + [heavy[2]],
            "last_of_129": mixed + [s64[1]], "whole_wave": heavy[:64], "two_waves_and_a_half": heavy[:160][::-1], "thresholds": edge,
            "everything": list(range(len(ns)))}


@pytest.mark.parametrize("max_gaps", [0, 5, 30])
def test_chaining_thresholds_equal_the_oracle(max_gaps, rep):
    """kg_candidates_batch == GenerateAlignmentCandidateForIlluminaSeq of the oracle, bit for bit: scores, PosDiff, every seed of every candidate"""
    from kart_amd import api
    ix, orc = rep["ix"], rep["orc"]
    ns = np.diff(rep["so"])
    want_all = rep["cands"] if max_gaps == 5 else [orc.candidates(len(rep["reads"][i]), rep["seeds"][rep["so"][i]:rep["so"][i + 1]], False, max_gaps)
                                                     for i in range(len(ns))]
    for name, idx in _chain_batches(ns).items():
        enc, off = api.concat_reads([rep["enc"][i] for i in idx])
        ws = ix.workspace(len(idx), len(enc))
        so, seeds = ws.seed_batch(enc, off, api.KG_MODE_FAST)
        assert (np.diff(so) == ns[idx]).all(), name
        got = ws.candidates_batch(so, False, max_gaps)
        for k, i in enumerate(idx):
            assert (seeds[so[k]:so[k + 1]] == rep["seeds"][rep["so"][i]:rep["so"][i + 1]].astype(api.SEED_DT)).all(), (name, k)
            want = want_all[i]
            assert len(got[k]) == len(want), (name, k, int(ns[i]), len(got[k]), len(want))
            for (gs, gp, gv), (ws_, wp, wv) in zip(got[k], want):
                assert (gs, gp) == (ws_, wp), (name, k, int(ns[i]))
                assert len(gv) == len(wv) and (gv["gPos"] == wv["gPos"]).all() and (gv["rPos"] == wv["rPos"]).all() and (gv["len"] == wv["rLen"]).all(), (name, k)


# ---- pairing, record level -----------------------------------------------------------------------------------------------------------------
def _align(rep, pairs, multi_hit=False, est_distance=1500, ws=None):
    """seed_batch (characters) + candidates_batch + align_batch on the given pairs as ONE paired chunk.  Returns (records, chunk_stats[0],
    candidates per read, growth of align_reasons())"""
    from kart_amd import api
    idx = [r for q in pairs for r in (2 * q, 2 * q + 1)]
    chars, off = api.concat_reads([rep["reads"][i] for i in idx])
    # (a workspace sized like the product's, far above the chunk: with -m the chained records of a read take slots behind the per-read ones, as many
    #  as the workspace's record arrays hold -- the fixture prints 4.7 records per read, a workspace of just the chunk's size runs out of them)
    ws = ws or rep["ix"].workspace(16384, 4 << 20)
    so, _ = ws.seed_batch(chars, off, api.KG_MODE_FAST | api.KG_INPUT_ASCII)
    cands = ws.candidates_batch(so, False, 5)
    before = ws.align_reasons()
    recs, stats = ws.align_batch([0, len(idx)], [1], est_distance=est_distance, max_insert=1500, max_gaps=5, multi_hit=multi_hit, unset_flag=UNSET_FLAG)
    return recs, stats[0], cands, (ws.align_reasons() - before).astype(np.int64)[:13]          # ([0..12] are the reasons, include/kart_amd.h)


def _pair_key(rep, recs, k):
    """everything the two reads' records say, for the comparison between arrangements"""
    from kart_amd import api
    out = []
    for r in (k, k + 1):
        if recs[r]["kind"] == api.KG_ALN_HOST:
            out.append("host")
        else:
            out.append([_record_columns(rep, x, 150) + (int(x["flip"]), int(x["primary"])) for x in _chain_of(recs, r)] + [int(recs[r]["rescue"]), int(recs[r]["est_lo"]), int(recs[r]["est_hi"])])
    return out


def _compare_with_reference(rep, pairs, recs, multi_hit):
    """every read decided on the device against its lines of the reference's SAM; returns the pairs handed back"""
    return compare_pairs_with_reference(rep, rep["sam_m"] if multi_hit else rep["sam"], pairs, recs, multi_hit)


def _classes(cands, n_pairs):
    nc = np.array([len(c) for c in cands])
    return nc[0::2][:n_pairs] * nc[1::2][:n_pairs]


@pytest.fixture(scope="module")
def whole(rep):
    """the whole fixture as one paired chunk, without and with -m: (records, stats, candidates, reasons) each"""
    pairs = list(range(len(rep["names"])))
    return {m: _align(rep, pairs, multi_hit=m) for m in (False, True)}


@pytest.mark.parametrize("multi_hit", [False, True])
def test_records_of_the_whole_fixture_equal_the_reference(multi_hit, rep, whole):
    """Every read whose record is not KG_ALN_HOST: POS, FLAG, MAPQ, CIGAR, contig, mate position, TLEN, AS, XS, NM and the strand shown equal the
    reference's line(s); the candidates behind the classes equal the oracle's; in each of the classes 33..1000 and 1001..4096 at most half of the
    pairs are handed back; the handed-back pairs are exactly the growth of align_reasons(), only the reasons a pair may have grow, and no device list
    was full.
    Measured shares of pairs handed back, by n1 x n2 (MI355X; the test prints them), the same without and with -m:
        2..32: 0 of 147      33..1000: 0 of 305      1001..4096: 0 of 113
    One pair of the 786 comes back in either run, for reason [10] (CIGAR too long); its product is below 2, so it is in none of the classes."""
    from kart_amd import api
    recs, stats, cands, reasons = whole[multi_hit]
    pairs = list(range(len(rep["names"])))
    for i, (g, w) in enumerate(zip(cands, rep["cands"])):       # (the class of a pair is taken from this call's candidates: they are the oracle's)
        assert [(c[0], c[1]) for c in g] == [(c[0], c[1]) for c in w], i
    host = _compare_with_reference(rep, pairs, recs, multi_hit)
    prod = _classes(cands, len(pairs))
    is_host = np.zeros(len(pairs), bool)
    is_host[host] = True
    shares = {}
    for name, lo, hi in (("2..32", 2, 32), ("33..1000", 33, 1000), ("1001..4096", 1001, 4096)):
        m = (prod >= lo) & (prod <= hi)
        shares[name] = (int((m & is_host).sum()), int(m.sum()))
    print("handed back per class (multi_hit=%d):" % multi_hit, shares, "reasons", reasons.tolist())
    for name in ("33..1000", "1001..4096"):
        assert shares[name][1] > 0 and 2 * shares[name][0] <= shares[name][1], shares
    assert len(host) == int(reasons.sum()), (len(host), reasons.tolist())
    assert reasons[9] == 0 and all(reasons[i] == 0 for i in range(13) if i not in ALLOWED_REASONS), reasons.tolist()
    assert int(stats["host_pairs"]) == 2 * len(host)
    # the heavy classes were really decided here, rescued ones among them
    heavy_dev = [q for q in pairs if prod[q] > 32 and not is_host[q]]
    assert sum(1 for q in heavy_dev if recs[2 * q]["rescue"]) >= 5, "no heavy pair went through the rescue windows on the device"


def test_chunk_statistics_equal_the_reference(rep, whole):
    """paired / distance / unmapped / unique of kg_chunk_stats against the same quantities counted from the reference's SAM over the reads decided on the
    device (src/Mapping.cpp:209-213, 183, 197); (lo, hi] holds the EstDistance of the call, and further calls under other values inside it -- both of its
    ends and a value half way to each -- give the records of the first.
    Above 1500 every pair is compared: the rescue windows are min(EstDistance, MaxInsertSize) long (src/AlignmentRescue.cpp:95) and stay what they were.
    BELOW 1500 THE PAIRS WITH `rescue` SET ARE LEFT OUT: (lo, hi] speaks for the "dist < EstiDistance" tests of CheckPairedAlignmentCandidates alone
    (include/kart_amd.h, kg_chunk_stats), while the windows RescueUnpairedAlignment searches shrink with EstDistance, so that such a pair's records may
    rightly change inside the interval; the record says so itself (`rescue`), and chunk_stats marks a chunk that holds such pairs (rescue_wanted).  At least one
    further call must have run: an interval of 1500 alone would leave this part of the test empty.  Measured: (1493, 1501], calls under 1494, 1497
    and 1501, 130 pairs decided on the device with `rescue` set."""
    from kart_amd import api
    recs, stats, _, _ = whole[False]
    paired = distance = unmapped = unique = 0
    for q, name in enumerate(rep["names"]):
        if recs[2 * q]["kind"] == api.KG_ALN_HOST:
            continue
        for m in (0, 1):
            lines = rep["sam"].get((name, m), [])
            if not lines:
                continue                                   # (a read the reference prints nothing for counts nowhere)
            f = lines[0][1]
            unmapped += f[2] == b"*"
            unique += f[2] != b"*" and int(f[4]) == 60
            if m == 0 and f[2] != b"*" and f[6] == b"=":
                paired += 2
                distance += abs(int(f[8])) if abs(int(f[8])) < 10000 else 0
    assert (int(stats["paired"]), int(stats["distance"]), int(stats["unmapped"]), int(stats["unique"])) == (paired, distance, unmapped, unique)
    lo, hi = int(stats["lo"]), int(stats["hi"])
    assert lo < 1500 <= hi, (lo, hi)
    pairs = list(range(len(rep["names"])))
    first = [_pair_key(rep, recs, 2 * k) for k in range(len(pairs))]
    n_rescue = sum(1 for q in pairs if recs[2 * q]["rescue"] and recs[2 * q]["kind"] != api.KG_ALN_HOST)
    assert n_rescue == 0 or int(stats["rescue_wanted"]) != 0             # (the statistics announce that the chunk holds such pairs)
    top = min(hi, 20000)                                                 # (hi is "no upper end" where no candidate pair lies beyond 1500)
    probes = sorted({lo + 1, (lo + 1 + 1500) // 2, (1500 + top) // 2, top} - {1500})
    assert probes, (lo, hi)
    print("EstDistance interval (%d, %d], further calls under" % (lo, hi), probes, "; pairs with rescue set:", n_rescue)
    for est in probes:
        assert lo < est <= hi
        again, again_stats, _, _ = _align(rep, pairs, est_distance=est)
        differ = [q for q in pairs if not (est < 1500 and recs[2 * q]["rescue"]) and _pair_key(rep, again, 2 * q) != first[q]]
        assert not differ, (est, differ[:5])


def test_records_do_not_depend_on_the_arrangement(rep, whole):
    """the same pairs alone, at the end of a partial wave, filling waves, heavy and light pairs that both want rescue windows interleaved (the
    wave_reserve hand-over between the lanes' loop and the wave's), and the whole fixture twice on one workspace: a pair's records stay what they
    were in the whole fixture -- which the test above holds to the reference"""
    from kart_amd import api
    for multi_hit in (False, True):
        recs, _, cands, _ = whole[multi_hit]
        n = len(rep["names"])
        prod = _classes(cands, n)
        ref_key = [_pair_key(rep, recs, 2 * q) for q in range(n)]
        dev = np.array([recs[2 * q]["kind"] != api.KG_ALN_HOST for q in range(n)])
        resc = np.array([bool(recs[2 * q]["rescue"]) for q in range(n)])
        pick = lambda m: [int(i) for i in np.flatnonzero(m)]
        heavy, light = pick((prod > 32) & dev), pick((prod <= 32) & dev)
        very = pick((prod > 1000) & dev)
        heavy_r, light_r = pick((prod > 32) & resc & dev), pick((prod <= 32) & resc & dev)
        assert len(heavy) >= 64 and len(light) >= 63 and len(very) >= 5 and len(heavy_r) >= 5 and len(light_r) >= 8, (len(heavy), len(light), len(very), len(heavy_r), len(light_r))
        inter = [x for p in zip((heavy_r * 32)[:32], (light_r * 32)[:32]) for x in p]   # heavy, light, heavy, light ... 64 pairs, all wanting windows
        arrangements = {"alone": [heavy[0]], "alone_above_1000": [very[0]], "alone_rescue": [heavy_r[0]], "last_of_a_partial_wave": light[:36] + [heavy[1]],
                        "last_of_a_partial_wave_rescue": light[:20] + [heavy_r[1]], "32_heavy": heavy[:32], "64_heavy": heavy[:64], "64_above_1000": (very * 13)[:64],
                        "interleaved_rescue": inter, "interleaved_rescue_shifted": light[:1] + inter[:-1]}
        for name, pairs in arrangements.items():
            got, _, _, _ = _align(rep, pairs, multi_hit=multi_hit)
            for k, q in enumerate(pairs):
                assert _pair_key(rep, got, 2 * k) == ref_key[q], (multi_hit, name, k, q, int(prod[q]))
        ws = api.Workspace(rep["ix"], 16384, 4 << 20)                                    # stale per-candidate state of the batch before
        try:
            for it in range(2):
                got, _, _, _ = _align(rep, list(range(n)), multi_hit=multi_hit, ws=ws)
                assert [_pair_key(rep, got, 2 * q) for q in range(n)] == ref_key, (multi_hit, it)
            got, _, _, _ = _align(rep, heavy[:5], multi_hit=multi_hit, ws=ws)
            assert [_pair_key(rep, got, 2 * k) for k in range(5)] == [ref_key[q] for q in heavy[:5]]
        finally:
            ws.close()


# ---- every alternative form of the stage, through the product binary -----------------------------------------------------------------------------
FORMS = [{"KG_ALN_NO_HEAVY": "1"}, {"KG_ALN_PAIR_HEAVY": "1"}, {"KG_ALN_PAIR_HEAVY": "1000000"}, {"KG_ALN_NO_TRIVIAL": "1"}, {"KG_ALN_NO_FAST": "1"},
         {"KG_ALN_NO_BINS": "1"}, {"KG_RESCUE_SCAN": "1"}, {}, {"KART_AMD_NO_STREAM": "1"}]


@pytest.fixture(scope="module")
def rep_files(rep):
    return [F.gunzip_to(os.path.join(F.SAM, "rep_%d.fq.gz" % m), os.path.join(rep["tmp"], "rep_%d.fq" % m)) for m in (1, 2)]


ABNORMAL = []                # the first child of this module that ended abnormally: no child is started after it
CHILD_SECONDS = 120          # (a run takes a second or two: a child that is still there after this hangs)


def _child(cmd, env):
    """One child process of the product under its own time limit.  A child that a signal ended (a fault, an abort), or that the time limit
    ended (a hang), is the LAST one this module starts on the card: every later launch fails before it starts.  Returns (stdout, stderr)."""
    assert not ABNORMAL, "no further child: %s" % ABNORMAL[0]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_SECONDS, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired:
        ABNORMAL.append("%s under %s was still running after %d s" % (" ".join(cmd[-8:]), env, CHILD_SECONDS))
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        ABNORMAL.append("%s under %s ended with status %d" % (" ".join(cmd[-8:]), env, r.returncode))
    assert r.returncode == 0, (env, r.returncode, r.stderr.decode()[-600:])
    return r.stdout.decode(), r.stderr.decode()


def _device_report(log):
    """(reads decided on the device, reads mapped by the host stages) of a KART_AMD_VERBOSE run"""
    m = re.search(r"device report: (\d+) reads decided on the device, (\d+) mapped by the host stages", log)
    assert m, log[-600:]
    return int(m.group(1)), int(m.group(2))


def _run_product(rep, rep_files, env, multi_hit):
    """the fixture through the product binary in a child of its own (the switches are read once per process); returns (SAM, log)"""
    assert os.path.exists(KART_AMD), "kart_amd/bin/kart-amd missing: __graft_entry__.build() builds it"
    out = os.path.join(rep["tmp"], "product.sam")
    if os.path.exists(out):
        os.remove(out)
    log, _ = _child([KART_AMD, "-silent", "-t", "4", "-i", rep["prefix"], "-f", rep_files[0], "-f2", rep_files[1], "-o", out] + (["-m"] if multi_hit else []),
                    dict(env, KART_AMD_UNSET_FLAG=str(UNSET_FLAG), KART_AMD_VERBOSE="1"))
    return open(out, "rb").read(), log


@pytest.mark.parametrize("env", FORMS, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) or "default")
def test_every_form_of_the_stage_writes_the_reference_sam(env, rep, rep_files):
    """each run against the reference's own file, never against another form's output -- and, since the host's stages write the same text, with
    reads decided on the device in every form: a form that handed every pair back would otherwise pass"""
    n_reads = len(rep["reads"])
    got, log = _run_product(rep, rep_files, env, False)
    assert got == F.load_sam("rep"), env
    dev, host = _device_report(log)
    print("form", env, "reads decided on the device: %d of %d" % (dev, n_reads))
    assert dev > 0 and dev + host == n_reads, (env, dev, host)
    got, log = _run_product(rep, rep_files, env, True)
    assert_sam_equals_reference_with_its_own_mask(F.load_sam("rep_m").split(b"\n"), rep["never"], got)
    dev, host = _device_report(log)
    print("form", env, "-m, reads decided on the device: %d of %d" % (dev, n_reads))
    assert dev > 0 and dev + host == n_reads, (env, dev, host)


def test_device_records_equal_the_host_report_on_the_fixture(rep, rep_files):
    """KART_AMD_CHECK_ALIGN: every read mapped on the host as well, the text of each device record compared with the host's"""
    for multi_hit in (False, True):
        _, log = _run_product(rep, rep_files, {"KART_AMD_CHECK_ALIGN": "1"}, multi_hit)
        line = [l for l in log.splitlines() if l.startswith("CHECK_ALIGN")]
        assert line and line[0].endswith(" 0 differ") and not line[0].startswith("CHECK_ALIGN: 0 device"), line


@pytest.mark.parametrize("case", ["pe", "pe_m", "pe_interleaved", "edge_pe"])
def test_wave_form_on_every_multi_candidate_pair_of_the_small_genome(case, built_lib, tmp_path):
    """KG_ALN_PAIR_HEAVY=1: every pair with more than one candidate pair goes through the wave's form (a child like the ones above: its own
    time limit, none started after an abnormal end)"""
    tmp = str(tmp_path)
    args = [materialise(tmp, a) if a.endswith((".fq", ".fa", ".gz")) else a for a in CASES[case]]
    out = os.path.join(tmp, case + ".sam")
    _child([KART_AMD, "-silent", "-t", "4", "-i", SMALL_PREFIX] + args + ["-o", out], {"KG_ALN_PAIR_HEAVY": "1"})
    assert open(out, "rb").read() == gzip.open(os.path.join(F.SAM, case + ".sam.gz")).read()
