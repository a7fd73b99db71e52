"""CPU: -R through the HOST pipeline (the product's host code bound to the CPU oracle backend, tests/_build/kart-host-oracle).  A run with
-R '@RG\\tID:g1\\tSM:s' is the golden SAM with exactly one more header line behind the last @SQ and "\\tRG:Z:g1" before the line feed of EVERY record line,
unmapped ones included; with -md the field stands behind MD:Z; -bo holds the same header text and the same records; two libraries take two read groups;
the command line rejects what is no read group line."""
import gzip
import os
import re
import subprocess

import pytest

from conftest import ROOT, SMALL_PREFIX
from test_host_pipeline import CASES, SAM, materialise
from test_md_host_cpu import bam_records, sam_as_bam_shows_it

RG_CASES = ["pe", "se", "se_m", "pe_m", "se_fasta", "pacbio", "edge_pe", "pe_interleaved"]
RG_ARG = "@RG\\tID:g1\\tSM:s"                      # as a shell hands it over: backslash, t
RG_LINE = "@RG\tID:g1\tSM:s"
RG_FIELD = re.compile(r"\tRG:Z:[^\t\n]*")


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


def with_read_group(plain: bytes, header_lines, ids=None) -> bytes:
    """the file a -R run must give: `plain` with header_lines behind its last @SQ line and RG:Z:<id> on every record line (ids: one per record line,
    or None for "g1" on all)"""
    out, k, in_header = [], 0, True
    for ln in plain.decode("latin-1").split("\n")[:-1]:
        if in_header and not ln.startswith("@"):
            out.extend(header_lines)
            in_header = False
        if ln.startswith("@") and in_header:
            assert ln.startswith(("@PG", "@SQ"))
            out.append(ln)
            continue
        out.append(ln + "\tRG:Z:" + ("g1" if ids is None else ids[k]))
        k += 1
    if in_header:
        out.extend(header_lines)
    return ("\n".join(out) + "\n").encode("latin-1")


def record_lines(text: bytes):
    return [ln for ln in text.decode("latin-1").split("\n") if ln and not ln.startswith("@")]


@pytest.mark.parametrize("case", RG_CASES)
def test_rg_run_is_the_golden_sam_with_one_header_line_and_the_field_on_every_record(case, binary, tmp_path):
    args = files_of(case, tmp_path)
    want = gzip.open(os.path.join(SAM, case + ".sam.gz")).read()
    got = run(binary, args + ["-R", RG_ARG], "-o", tmp_path / "rg.sam")
    assert got == with_read_group(want, [RG_LINE])
    header = [ln for ln in got.decode("latin-1").split("\n") if ln.startswith("@")]
    assert header[-1] == RG_LINE and header[-2].startswith("@SQ") and header.count(RG_LINE) == 1
    # without the flag nothing changes
    plain = run(binary, args, "-o", tmp_path / "plain.sam")
    assert plain == want and b"RG:Z" not in plain and b"@RG" not in plain


def test_the_cases_hold_mapped_and_unmapped_records():
    """(a condition on the inputs, not on the product: both kinds of record are covered by the test above)"""
    mapped = unmapped = 0
    for case in RG_CASES:
        for ln in record_lines(gzip.open(os.path.join(SAM, case + ".sam.gz")).read()):
            if ln.split("\t")[2] == "*":
                unmapped += 1
            else:
                mapped += 1
    assert mapped > 0 and unmapped > 0


@pytest.mark.parametrize("case", ["pe", "se_m", "se_fasta", "edge_pe"])
def test_rg_stands_behind_md(case, binary, tmp_path):
    args = files_of(case, tmp_path)
    md = run(binary, args + ["-md"], "-o", tmp_path / "md.sam")
    both = run(binary, args + ["-md", "-R", RG_ARG], "-o", tmp_path / "both.sam")
    n_mapped = n_unmapped = 0
    for ln in record_lines(both):
        f = ln.split("\t")
        assert f[-1] == "RG:Z:g1", ln
        if f[2] == "*":
            assert f[-2] == "XS:i:0", ln
            n_unmapped += 1
        else:
            assert f[-2].startswith("MD:Z:") and f[-3].startswith("XS:i:"), ln
            n_mapped += 1
    assert n_mapped > 0 and (n_unmapped > 0 or case != "edge_pe")          # (edge_pe holds reads that stay unmapped)
    # with the RG field cut, the file is the -md file
    cut = RG_FIELD.sub("", both.decode("latin-1")).replace(RG_LINE + "\n", "", 1).encode("latin-1")
    assert cut == md


@pytest.mark.parametrize("md", [False, True], ids=["plain", "md"])
@pytest.mark.parametrize("case", ["pe", "se_m", "edge_pe"])
def test_bam_holds_the_header_line_and_the_same_records(case, md, binary, tmp_path):
    args = files_of(case, tmp_path) + (["-md"] if md else []) + ["-R", RG_ARG]
    sam = run(binary, args, "-o", tmp_path / "rg.sam")
    blob = run(binary, args, "-bo", tmp_path / "rg.bam")
    raw = gzip.decompress(blob)
    l_text = int.from_bytes(raw[4:8], "little")
    text = raw[8:8 + l_text].decode()
    assert text == "".join(ln + "\n" for ln in sam.decode("latin-1").split("\n") if ln.startswith("@"))
    assert text.endswith(RG_LINE + "\n")
    _, recs = bam_records(blob)
    lines = record_lines(sam)
    assert len(lines) == len(recs) > 0
    for ln, rec in zip(lines, recs):
        assert sam_as_bam_shows_it(ln) == rec
        assert rec[-1] == "RG:Z:g1"
        assert not md or rec[2] == "*" or rec[-2].startswith("MD:Z:")


def test_two_libraries_two_read_groups(binary, tmp_path):
    args = files_of("edge_multi_lib", tmp_path)
    f1, f2 = args[1], args[2]
    a, b = "@RG\tID:laneA\tSM:s", "@RG\tID:laneB\tSM:s\tPL:ILLUMINA"
    lib1 = run(binary, ["-f", f1], "-o", tmp_path / "l1.sam")
    lib2 = run(binary, ["-f", f2], "-o", tmp_path / "l2.sam")
    n1, n2 = len(record_lines(lib1)), len(record_lines(lib2))
    plain = run(binary, args, "-o", tmp_path / "plain.sam")
    assert plain == gzip.open(os.path.join(SAM, "edge_multi_lib.sam.gz")).read()
    assert record_lines(plain) == record_lines(lib1) + record_lines(lib2)
    # one per library: the k-th for the k-th (real TABs are taken as they are)
    got = run(binary, args + ["-R", a.replace("\t", "\\t"), "-R", b], "-o", tmp_path / "two.sam")
    assert got == with_read_group(plain, [a, b], ["laneA"] * n1 + ["laneB"] * n2)
    # one for all
    got = run(binary, args + ["-R", a], "-o", tmp_path / "one.sam")
    assert got == with_read_group(plain, [a], ["laneA"] * (n1 + n2))
    # the same line twice: one read group, one header line
    got = run(binary, args + ["-R", a, "-R", a], "-o", tmp_path / "same.sam")
    assert got == with_read_group(plain, [a], ["laneA"] * (n1 + n2))


@pytest.mark.parametrize("case", ["pe", "edge_pe"])
def test_thread_counts_give_the_same_file(case, binary, tmp_path):
    args = files_of(case, tmp_path) + ["-md", "-R", RG_ARG]
    one = run(binary, args + ["-t", "1"], "-o", tmp_path / "t1.sam")
    eight = run(binary, args + ["-t", "8"], "-o", tmp_path / "t8.sam")
    assert one == eight and one.count(b"\tRG:Z:g1\n") == len(record_lines(one))


@pytest.mark.parametrize("out_flag", ["-o", "-bo"])
@pytest.mark.parametrize("case", ["pe_plain", "edge_multi_lib"])
def test_sharded_run_gives_the_unsharded_file(case, out_flag, binary, tmp_path):
    """-gpu 0,1,2: plain FASTQ of one library is split between three processes, two libraries are mapped by shard 0 alone; rank 0 writes the header, alone"""
    args = files_of(case, tmp_path) + ["-R", RG_ARG]
    whole = run(binary, args + ["-t", "6"], out_flag, tmp_path / "whole.out")
    parts = run(binary, args + ["-t", "6", "-gpu", "0,1,2"], out_flag, tmp_path / "sharded.out")
    if out_flag == "-bo":
        whole, parts = gzip.decompress(whole), gzip.decompress(parts)
    assert parts == whole and whole.count(RG_LINE.encode()) == 1 and whole.count(b"RG:Z:g1" if out_flag == "-o" else b"RGZg1\0") > 0


BAD = {
    "no @RG prefix": (["-R", "ID:g1\\tSM:s"], 1),
    "no ID": (["-R", "@RG\\tSM:s"], 1),
    "empty ID": (["-R", "@RG\\tID:\\tSM:s"], 1),
    "256-byte ID": (["-R", "@RG\\tID:" + "x" * 256], 1),
    "ID with a space": (["-R", "@RG\\tID:g 1\\tSM:s"], 1),
    "embedded LF": (["-R", "@RG\\tID:g1\nSM:s"], 1),
    "embedded CR": (["-R", "@RG\\tID:g1\\tSM:s\r"], 1),
    "two for three libraries": (["-R", "@RG\\tID:a", "-R", "@RG\\tID:b"], 3),
    "one ID, two texts": (["-R", "@RG\\tID:a\\tSM:s", "-R", "@RG\\tID:a\\tSM:t"], 2),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_bad_read_group_lines_are_usage_errors(what, binary, tmp_path):
    extra, n_libs = BAD[what]
    fq = materialise(str(tmp_path), "edge_1.fq")
    out = tmp_path / "never.sam"
    r = subprocess.run([binary, "-silent", "-i", SMALL_PREFIX, "-f"] + [fq] * n_libs + extra + ["-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = r.stdout.decode()
    assert r.returncode == 1, text[-300:]
    assert "Error! -R expects" in text and "Usage:" in text
    assert not out.exists()


def test_a_255_byte_id_is_taken(binary, tmp_path):
    fq = materialise(str(tmp_path), "edge_1.fq")
    rg_id = "".join(chr(33 + i % 94) for i in range(255))          # every accepted byte
    got = run(binary, ["-f", fq, "-R", "@RG\tID:" + rg_id], "-o", tmp_path / "long.sam")
    lines = record_lines(got)
    assert lines and all(ln.endswith("\tRG:Z:" + rg_id) for ln in lines)


def test_read_groups_are_listed_by_the_usage_text(binary):
    r = subprocess.run([binary, "-h"], stdout=subprocess.PIPE)
    text = r.stdout.decode()
    assert "-R STR" in text and "@RG" in text and "RG:Z" in text
