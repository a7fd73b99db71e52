"""CPU: the repeat-family fixture (tests/golden/rep.fa.gz, tests/golden/sam/rep_*; oracle/make_golden_rep.py) holds the classes of reads and
pairs that tests/test_rep_gpu.py needs -- counted here from the committed files through the CPU oracle, so that the fixture cannot lose them
unnoticed -- and the host pipeline on the CPU oracle backend reproduces the reference's SAM for it."""
import os
import subprocess

import numpy as np
import pytest

import rep_fixture as F
from conftest import ROOT
from test_host_pipeline import UNSET_FLAG, assert_sam_equals_reference_with_its_own_mask


@pytest.fixture(scope="module")
def rep(tmp_path_factory):
    """the index of the committed genome (CPU build), the held reads, their seeds and candidates from the oracle"""
    from oracle import oracle as O
    tmp = str(tmp_path_factory.mktemp("rep"))
    prefix = F.build_rep_index(tmp, device="cpu")
    names, reads = F.load_reads()
    orc = O.Oracle(prefix)
    so, seeds, cands = F.oracle_chain(orc, reads)
    orc.close()
    return {"tmp": tmp, "prefix": prefix, "names": names, "reads": reads, "so": so, "cands": cands}


def test_fixture_sizes():
    import gzip
    text = gzip.open(F.REP_FA).read()
    assert text.count(b">") == 3 and len(text) < 310000          # the family contig, a unique contig, the decoy; about 300 kb
    names, reads = F.load_reads()
    assert len(reads) == 2 * len(names) <= 4000                  # ONE chunk of the reference: EstDistance stays MaxInsertSize
    largest = os.path.getsize(os.path.join(F.SAM, "pe_fasta.sam.gz"))
    for f in ("rep_1.fq.gz", "rep_2.fq.gz", "rep.sam.gz", "rep_m.sam.gz"):
        assert os.path.getsize(os.path.join(F.SAM, f)) < largest, f
    assert os.path.getsize(F.REP_FA) < largest


def test_fixture_holds_every_class(rep):
    """The classes the wave-cooperative forms are chosen by, from the oracle alone (counted on the committed files, in brackets):
    reads of exactly 16 / 17 / 64 / 65 seeds (chain_read_wave takes 17..64) [9 / 10 / 11 / 8], 18..63 [458], above 65 [419];
    pairs by n1 x n2: 25..32 [41], 33..40 [101] (the wave forms take > 32), 900..1000 [29], 1001..4096 [113] (remove_redundant_wave's pre-pass),
    33..1000 in all [305]; a pair whose mate 2 has more than 64 candidates [66: the `j += 64` loops take a second round]; heavy pairs (> 32) whose
    chained lists pair nothing and which the reference reports as a proper pair -- RescueUnpairedAlignment's records -- [28]; heavy pairs with
    more than one record per read under -m [167].
    The committed selection holds 786 pairs.
    PRODUCT ABOVE 4096 (the hand-back WHY_PAIR_PRODUCT, align_reasons()[0]) IS NOT COVERED.  The generator's pool was 18 100 pairs, 12 100 of them
    drawn from inside single families, the family of 100 copies among them.  The largest n1 x n2 of any pair of the pool is 2520; the largest
    n1 x n2 among the 786 committed pairs is 1804 (asserted below to stay at most 4096, so that this paragraph cannot go stale unnoticed).  A
    search piece locates at most OCC_Thr = 50 hits, so a read's candidate list stays below 70 whatever the copy count (66 is the longest here), and no
    pair of the pool had both of its lists that long at once; the genome is at its size limit."""
    so, cands = rep["so"], rep["cands"]
    ns = np.diff(so)
    nc = np.array([len(c) for c in cands])
    prod = nc[0::2] * nc[1::2]
    n_pairs = len(prod)
    count = {k: int((ns == k).sum()) for k in (16, 17, 64, 65)}
    mid, above = int(((ns >= 18) & (ns <= 63)).sum()), int((ns > 65).sum())
    in_range = lambda lo, hi: int(((prod >= lo) & (prod <= hi)).sum())
    pairing = np.array([F.chained_lists_pair(cands[2 * q], cands[2 * q + 1]) for q in range(n_pairs)])
    recs = F.sam_records(F.load_sam("rep"))
    recs_m = F.sam_records(F.load_sam("rep_m"), F.never_assigned_lines())

    def proper(q):
        x, y = recs.get((rep["names"][q], 0), []), recs.get((rep["names"][q], 1), [])
        return len(x) == 1 and len(y) == 1 and int(x[0][1][1]) & 2 and int(y[0][1][1]) & 2

    rescued = sum(1 for q in range(n_pairs) if prod[q] > 32 and not pairing[q] and proper(q))
    multi = sum(1 for q in range(n_pairs) if prod[q] > 32 and max(len(recs_m.get((rep["names"][q], m), [])) for m in (0, 1)) > 1)
    print("seeds", count, mid, above, "products", in_range(25, 32), in_range(33, 40), in_range(900, 1000), in_range(1001, 4096), in_range(33, 1000),
          "largest", int(prod.max()), "largest mate-2 list", int(nc[1::2].max()), "rescued", rescued, "multi", multi)
    assert all(v >= 3 for v in count.values()), count
    assert mid >= 20 and above >= 20
    assert in_range(25, 32) >= 3 and in_range(33, 40) >= 3 and in_range(900, 1000) >= 3
    assert in_range(1001, 4096) >= 5 and in_range(33, 1000) >= 50
    assert int(nc[1::2].max()) > 64
    assert int(prod.max()) <= 4096                               # (the docstring: no pair of the fixture is handed back for its product)
    assert rescued >= 10 and multi >= 10


@pytest.fixture(scope="module")
def host_oracle_binary():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_backend")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "_build", "kart-host-oracle")


@pytest.mark.parametrize("multi_hit", [False, True])
def test_host_pipeline_reproduces_the_reference(multi_hit, rep, host_oracle_binary):
    """rep.sam.gz byte for byte; rep_m.sam.gz with UNSET_FLAG on exactly the lines whose FLAG the reference never assigns"""
    tmp = rep["tmp"]
    f1, f2 = (F.gunzip_to(os.path.join(F.SAM, "rep_%d.fq.gz" % m), os.path.join(tmp, "rep_%d.fq" % m)) for m in (1, 2))
    out = os.path.join(tmp, "host_m.sam" if multi_hit else "host.sam")
    r = subprocess.run([host_oracle_binary, "-silent", "-t", "3", "-i", rep["prefix"], "-f", f1, "-f2", f2, "-o", out] + (["-m"] if multi_hit else []),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, KART_AMD_UNSET_FLAG=str(UNSET_FLAG)), timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-400:]
    got = open(out, "rb").read()
    if multi_hit:
        never = F.never_assigned_lines()
        assert assert_sam_equals_reference_with_its_own_mask(F.load_sam("rep_m").split(b"\n"), never, got) == len(never) > 0
    else:
        assert got == F.load_sam("rep")
