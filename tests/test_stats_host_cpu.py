"""CPU: -stats through the HOST pipeline (the product's host code bound to the CPU oracle backend, tests/_build/kart-host-oracle): every record the host
prints -- mapped by itself, from a device-style record, -pacbio with its CIGAR from the pool, the line readers -- is tallied at the printer's record sites
(host/detail/tally.inc).  Expected bytes come from tests/stats_plain.py, a plain recount of a SAM text the existing suite already holds to the reference
(the golden, or the same run's main output); stats_plain itself is held to a file written out by hand.  In every case the main output is the one of the
run without the flag, byte for byte."""
import gzip
import os
import subprocess

import pytest

import stats_plain
from conftest import ROOT, SMALL_PREFIX
from test_host_pipeline import CASES, SAM, materialise


@pytest.fixture(scope="module")
def binary():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_backend")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "_build", "kart-host-oracle")


def files_of(case, tmp):
    return [materialise(str(tmp), a) if a.endswith((".fq", ".fa", ".gz")) else a for a in CASES[case]]


def run(binary, args, out_flag, out, env=None):
    r = subprocess.run([binary, "-silent", "-i", SMALL_PREFIX] + args + [out_flag, str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stdout.decode()[-500:]
    return open(out, "rb").read()


def run_with_stats(binary, args, tmp, out_flag="-o", env=None, tag="st"):
    """-> (main output, the -stats file)"""
    path = tmp / (tag + ".stats")
    main = run(binary, args + ["-stats", str(path)], out_flag, tmp / (tag + ".out"), env)
    return main, path.read_bytes()


# ---- the plain recount against a file written by hand ------------------------------------------------------------------------------------------------
def sam_line(name, flag, pos, mapq, cigar, rnext, pnext, tlen):
    rname = "*" if flag & 4 else "chr1"
    return "\t".join([name, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), "ACGT", "FFFF", "NM:i:0", "AS:i:4", "XS:i:0"]) + "\n"


HAND_SAM = ("@PG\tID:kart\tPN:Kart\tVN:2.5.6\n@SQ\tSN:chr1\tLN:100000\n" +
            sam_line("u1", 4, 0, 0, "*", "*", 0, 0) +                          # an unmapped single
            sam_line("p1", 99, 100, 60, "100M", "=", 250, 250) +               # a proper pair ...
            sam_line("p1", 147, 250, 60, "100M", "=", 100, -250) +             # ... whose second record has the negative TLEN: not an insert size
            sam_line("s1", 73, 500, 0, "5S90M2I3D53M", "*", 0, 0) +            # a singleton, MAPQ 0 ...
            sam_line("s1", 133, 0, 0, "*", "*", 0, 0) +                        # ... and its unmapped mate
            sam_line("q1", 97, 1000, 60, "50M", "=", 3000, 2048) +             # TLEN 2048: the first of the overflow row
            sam_line("q1", 145, 3000, 60, "48M", "=", 1000, -2048) +
            sam_line("r1", 97, 1000, 30, "20M10N20M", "=", 6000, 5000) +       # TLEN 5000: the same row; N is "other"
            sam_line("r1", 145, 6000, 70, "2H48M", "=", 1000, -5000)).encode()  # MAPQ 70: bin 63; H is "other"

HAND_STATS = b"""# kart-amd stats 1
SN\trecords\t9
SN\tmapped\t7
SN\tunmapped\t2
SN\tproper_pair\t2
SN\tboth_mapped\t6
SN\tsingleton\t1
FL\t0x1\t8
FL\t0x2\t2
FL\t0x4\t2
FL\t0x8\t1
FL\t0x10\t3
FL\t0x20\t3
FL\t0x40\t4
FL\t0x80\t4
FL\t0x100\t0
FL\t0x200\t0
FL\t0x400\t0
FL\t0x800\t0
MQ\t0\t1
MQ\t30\t1
MQ\t60\t4
MQ\t63\t1
IS\t250\t1
IS\t>=2048\t2
CG\tM\t529\t9
CG\tI\t2\t1
CG\tD\t3\t1
CG\tS\t5\t1
CG\tother\t12\t2
"""

ZERO_STATS = ("# kart-amd stats 1\n" + "".join("SN\t%s\t0\n" % k for k in ("records", "mapped", "unmapped", "proper_pair", "both_mapped", "singleton")) +
              "".join("FL\t0x%x\t0\n" % (1 << b) for b in range(12)) + "".join("CG\t%s\t0\t0\n" % k for k in ("M", "I", "D", "S", "other"))).encode()


def test_the_plain_recount_against_a_file_written_by_hand():
    assert stats_plain.text(HAND_SAM) == HAND_STATS
    assert stats_plain.text(b"@PG\tID:kart\tPN:Kart\tVN:2.5.6\n") == ZERO_STATS == stats_plain.text(b"")
    # the row of the same records: the words the file's numbers come from
    r = stats_plain.row(HAND_SAM)
    assert r.sum() == 9 + 27 + 2 + 6 + 1 + (529 + 9 + 3 + 4 + 6 + 14) + 7 + 3 and r[stats_plain.ISIZE0 + 2048] == 2 and r[stats_plain.MAPQ0 + 63] == 1


# ---- golden cases ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["edge_pe", "edge_se", "edge_se_m", "edge_multi_lib", "se_fasta", "pacbio"])
def test_golden_cases(case, binary, tmp_path):
    args = files_of(case, tmp_path)
    want = gzip.open(os.path.join(SAM, case + ".sam.gz")).read()
    main, stats = run_with_stats(binary, args, tmp_path)
    assert main == want == run(binary, args, "-o", tmp_path / "plain.sam")
    assert stats == stats_plain.text(want)
    assert b"SN\trecords\t%d\n" % len(stats_plain.records(want)) in stats and len(stats_plain.records(want)) > 0


def test_edge_pe_has_insert_sizes_and_its_45_unmapped_records(binary, tmp_path):
    _, stats = run_with_stats(binary, files_of("edge_pe", tmp_path), tmp_path)
    lines = stats.decode().split("\n")
    assert "SN\tunmapped\t45" in lines
    assert sum(1 for ln in lines if ln.startswith("IS\t")) > 0


@pytest.mark.parametrize("case", ["edge_pe", "pe"])
def test_the_line_readers_and_small_batches(case, binary, tmp_path):
    """the getline() / gzgets() readers instead of the mapped file, and a batch per chunk: the chunks' tallies are summed in output order all the same
    (pe: 2.25 chunks, EstDistance switches from 1500 to the estimate on the way)"""
    args = files_of(case, tmp_path)
    want = gzip.open(os.path.join(SAM, case + ".sam.gz")).read()
    for env in ({"KART_AMD_NO_MMAP": "1"}, {"KART_AMD_BATCH_READS": "4000"}, {"KART_AMD_BATCH_READS": "4000", "KART_AMD_NO_MMAP": "1"}):
        main, stats = run_with_stats(binary, args, tmp_path, env=env)
        assert main == want and stats == stats_plain.text(want)


@pytest.mark.parametrize("case", ["edge_pe", "edge_se_m", "pacbio"])
def test_bam_output_writes_the_same_file(case, binary, tmp_path):
    args = files_of(case, tmp_path)
    bam_plain = run(binary, args, "-bo", tmp_path / "plain.bam")
    _, stats_sam = run_with_stats(binary, args, tmp_path, tag="sam")
    bam, stats_bam = run_with_stats(binary, args, tmp_path, out_flag="-bo", tag="bam")
    assert bam == bam_plain and stats_bam == stats_sam and len(stats_sam) > len(ZERO_STATS)


def test_unmapped_files_and_stats_together(binary, tmp_path):
    args = files_of("edge_pe", tmp_path)
    un = ["-un", str(tmp_path / "u1"), "-un2", str(tmp_path / "u2")]
    plain = run(binary, args + un, "-o", tmp_path / "un.sam")
    u1, u2 = (tmp_path / "u1").read_bytes(), (tmp_path / "u2").read_bytes()
    _, stats_alone = run_with_stats(binary, args, tmp_path, tag="alone")
    main, stats = run_with_stats(binary, args + un, tmp_path, tag="both")
    assert main == plain and stats == stats_alone and len(u1) > 0
    assert ((tmp_path / "u1").read_bytes(), (tmp_path / "u2").read_bytes()) == (u1, u2)


def test_an_empty_read_file_gives_the_all_zero_file(binary, tmp_path):
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    main, stats = run_with_stats(binary, ["-f", str(empty)], tmp_path)
    assert stats == ZERO_STATS and stats_plain.records(main) == []


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def bad_lines(fq1, fq2, tmp):
    """-> {what: (arguments, output flag, output name)}"""
    st, out = str(tmp / "s.txt"), str(tmp / "never.sam")
    return {
        "no value": (["-f", fq1, "-o", out, "-stats"], None, None),
        "the -o name": (["-f", fq1, "-stats", out], "-o", out),
        "the -bo name": (["-f", fq1, "-stats", out], "-bo", out),
        "the -un name": (["-f", fq1, "-un", st, "-stats", st], "-o", out),
        "the -un2 name": (["-f", fq1, "-f2", fq2, "-un", str(tmp / "u1"), "-un2", st, "-stats", st], "-o", out),
        "a device list": (["-f", fq1, "-stats", st, "-gpu", "0,1"], "-o", out),
        "a shard": (["-f", fq1, "-stats", st, "-shard", "0/2", "-rendezvous", str(tmp / "rdv")], "-o", out),
    }


@pytest.mark.parametrize("what", sorted(bad_lines("a", "b", __import__("pathlib").Path("."))))
def test_rejected_command_lines(what, binary, tmp_path):
    fq1, fq2 = materialise(str(tmp_path), "edge_1.fq"), materialise(str(tmp_path), "edge_2.fq")
    args, flag, name = bad_lines(fq1, fq2, tmp_path)[what]
    r = subprocess.run([binary, "-silent", "-i", SMALL_PREFIX] + args + ([flag, name] if flag else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = r.stdout.decode()
    assert r.returncode != 0, text[-300:]
    assert "Error! " in text and "-stats" in text.split("Usage:")[0] and "Usage:" in text
    assert not (tmp_path / "never.sam").exists() and not (tmp_path / "s.txt").exists()


def test_a_name_that_cannot_be_opened_fails_before_anything_is_mapped(binary, tmp_path):
    fq1 = materialise(str(tmp_path), "edge_1.fq")
    out = tmp_path / "never.sam"
    r = subprocess.run([binary, "-silent", "-i", SMALL_PREFIX, "-f", fq1, "-stats", str(tmp_path / "no_such_dir" / "s.txt"), "-o", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode != 0 and "s.txt" in r.stdout.decode() and not out.exists()


def test_the_usage_text_lists_the_flag(binary):
    text = subprocess.run([binary, "-h"], stdout=subprocess.PIPE).stdout.decode()
    assert "-stats FILE" in text
