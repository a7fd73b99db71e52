"""CPU: -un / -un2 through the HOST pipeline (the product's host code bound to the CPU oracle backend, tests/_build/kart-host-oracle): every reader of
the host -- mapped FASTQ, inflated gz text, the getline() and gzgets() line readers -- keeps the bytes of the records it takes, and the chunk stage
writes those of the unmapped units.  Expected bytes come from tests/un_plain.py over the input files and a SAM text the existing suite already holds to
the reference: the golden, or the same run's main output.  In every case the main output is the one of the run without the flags, byte for byte."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import un_plain
from conftest import ROOT, SMALL_PREFIX
from test_host_pipeline import CASES, SAM, materialise


@pytest.fixture(scope="module")
def binary():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_backend")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "_build", "kart-host-oracle")


def files_of(case, tmp):
    return [materialise(str(tmp), a) if a.endswith((".fq", ".fa", ".gz")) else a for a in CASES[case]]


def text_of(path):
    return gzip.open(path).read() if path.endswith(".gz") else open(path, "rb").read()


def run(binary, args, out_flag, out, env=None):
    r = subprocess.run([binary, "-silent", "-i", SMALL_PREFIX] + args + [out_flag, str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stdout.decode()[-500:]
    return open(out, "rb").read()


def run_with_un(binary, args, tmp, out_flag="-o", env=None, tag="un"):
    """-> (main output, -un bytes, -un2 bytes or None)"""
    two = "-f2" in args
    un1, un2 = tmp / (tag + ".1"), tmp / (tag + ".2")
    main = run(binary, args + ["-un", str(un1)] + (["-un2", str(un2)] if two else []), out_flag, tmp / (tag + ".out"), env)
    assert not two or un2.exists()
    return main, un1.read_bytes(), un2.read_bytes() if two else None


def library_of(args):
    """(files 1, files 2) of a command line"""
    f1, f2, into = [], [], None
    for a in args:
        if a in ("-f", "-f2"):
            into = f1 if a == "-f" else f2
        elif a.startswith("-"):
            into = None
        elif into is not None:
            into.append(a)
    return f1, f2


def expected_of(args, sam_text):
    f1, f2 = library_of(args)
    assert len(f1) == 1
    two = bool(f2)
    texts = [text_of(f1[0])] + ([text_of(f2[0])] if two else [])
    return un_plain.expected(texts, sam_text, two or "-p" in args, two, fasta=texts[0][:1] == b">")


# ---- golden cases ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["edge_pe", "edge_se", "edge_se_m"])
def test_golden_cases(case, binary, tmp_path):
    args = files_of(case, tmp_path)
    want = gzip.open(os.path.join(SAM, case + ".sam.gz")).read()
    main, un1, un2 = run_with_un(binary, args, tmp_path)
    assert main == want == run(binary, args, "-o", tmp_path / "plain.sam")
    e1, e2 = expected_of(args, want)
    assert un1 == e1 and (un2 is None or un2 == e2) and len(e1) > 0


def test_edge_pe_writes_exactly_its_twenty_both_unmapped_pairs(binary, tmp_path):
    args = files_of("edge_pe", tmp_path)
    want = gzip.open(os.path.join(SAM, "edge_pe.sam.gz")).read()
    recs = [ln.split(b"\t") for ln in want.split(b"\n") if ln and not ln.startswith(b"@")]
    unmapped = [f for f in recs if int(f[1]) & 4]
    both = [f for f in unmapped if int(f[1]) & 8]
    assert (len(unmapped), len(both)) == (45, 40)
    _, un1, un2 = run_with_un(binary, args, tmp_path)
    r1, r2 = un_plain.records(un1, False), un_plain.records(un2, False)
    assert len(r1) == len(r2) == 20
    assert [un_plain.name_of(r) for r in r1] == [f[0] for f in both if int(f[1]) & 0x40] == [un_plain.name_of(r) for r in r2]
    # the five unmapped reads with a mapped mate are not among them
    lone = {(f[0], f[9]) for f in unmapped if not int(f[1]) & 8}
    assert len(lone) == 5
    written = {(un_plain.name_of(r), r.split(b"\n")[1]) for r in r1 + r2}
    assert not any(name in {n for n, _ in written} for name, _ in lone)


def test_several_libraries_append_in_order(binary, tmp_path):
    args = files_of("edge_multi_lib", tmp_path)
    want = gzip.open(os.path.join(SAM, "edge_multi_lib.sam.gz")).read()
    main, un1, _ = run_with_un(binary, args, tmp_path)
    assert main == want
    parts = []
    for k, f in enumerate(library_of(args)[0]):
        lib_sam = run(binary, ["-f", f], "-o", tmp_path / ("lib%d.sam" % k))
        parts.append(un_plain.expected([text_of(f)], lib_sam, False, False)[0])
    assert all(parts) and un1 == parts[0] + parts[1]


@pytest.mark.parametrize("case", ["pe", "se_fasta", "pacbio"])
def test_files_exist_and_are_empty_when_nothing_is_unmapped(case, binary, tmp_path):
    args = files_of(case, tmp_path)
    want = gzip.open(os.path.join(SAM, case + ".sam.gz")).read()
    assert not any(int(ln.split(b"\t")[1]) & 4 for ln in want.split(b"\n") if ln and not ln.startswith(b"@"))
    main, un1, un2 = run_with_un(binary, args, tmp_path)
    assert main == want and un1 == b"" and un2 in (None, b"")


# ---- constructed inputs: the fixtures' reads with seeded random reads mixed in ------------------------------------------------------------------------
def fastq_records(path):
    return un_plain.records(text_of(path), False)


def random_record(rng, k, mate):
    n = int(rng.integers(60, 140))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    return b"@rnd%d comment %d/%d\n" % (k, k, mate) + (seq.lower() if k % 3 == 0 else seq) + b"\n+" + (b"rnd%d" % k if k % 2 else b"") + b"\n" + b"F" * n + b"\n"


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """300 pairs of the pe fixture with 100 random pairs among them -> the two mate files' records"""
    tmp = tmp_path_factory.mktemp("mixed")
    m1, m2 = fastq_records(materialise(str(tmp), "pe_1.fq")), fastq_records(materialise(str(tmp), "pe_2.fq"))
    rng = np.random.default_rng(15)
    r1, r2 = [], []
    for k in range(300):
        r1.append(m1[k]); r2.append(m2[k])
        if k % 3 == 1:
            r1.append(random_record(rng, k, 1)); r2.append(random_record(rng, k, 2))
    return r1, r2


def as_fasta(records, width):
    out = b""
    for r in records:
        head, seq = r.split(b"\n")[:2]
        out += b">" + head[1:] + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))
    return out


def write_form(form, mixed, tmp):
    """-> the command line's input part"""
    r1, r2 = mixed

    def put(name, data):
        p = str(tmp / name)
        with (gzip.open(p, "wb") if name.endswith(".gz") else open(p, "wb")) as f:
            f.write(data)
        return p
    if form == "plain":
        return ["-f", put("a_1.fq", b"".join(r1)), "-f2", put("a_2.fq", b"".join(r2))]
    if form == "gz":
        return ["-f", put("a_1.fq.gz", b"".join(r1)), "-f2", put("a_2.fq.gz", b"".join(r2))]
    if form == "interleaved":
        return ["-f", put("a_i.fq", b"".join(a + b for a, b in zip(r1, r2))), "-p"]
    if form == "single_end":
        return ["-f", put("a_s.fq", b"".join(r1))]
    if form == "fasta60":
        return ["-f", put("a_s.fa", as_fasta(r1, 60))]
    if form == "fasta_gz":
        return ["-f", put("a_s.fa.gz", as_fasta(r1, 1 << 20))]          # (gzGetNextEntry takes one sequence line per entry)
    if form == "no_final_lf":
        return ["-f", put("a_1.fq", b"".join(r1)[:-1]), "-f2", put("a_2.fq", b"".join(r2)[:-1])]
    if form == "fasta60_no_final_lf":
        return ["-f", put("a_s.fa", as_fasta(r1, 60)[:-1])]
    raise KeyError(form)


def check_constructed(binary, args, tmp, env=None):
    plain = run(binary, args, "-o", tmp / "plain.sam", env)
    main, un1, un2 = run_with_un(binary, args, tmp, env=env)
    assert main == plain
    e1, e2 = expected_of(args, plain)
    assert un1 == e1 and (un2 is None or un2 == e2)
    # the condition on the input: units of both kinds, so that neither side of the selection passes empty
    f1, _ = library_of(args)
    step = 2 if ("-p" in args and "-f2" not in args) else 1
    n_units = len(un_plain.records(text_of(f1[0]), f1[0].endswith((".fa", ".fa.gz")))) // step
    n_sel = len(un_plain.records(un1, un1[:1] == b">")) // step
    assert n_sel >= 50 and n_units - n_sel >= 50, (n_sel, n_units)
    return plain, un1, un2


@pytest.mark.parametrize("form", ["plain", "gz", "interleaved", "single_end", "fasta60", "fasta_gz", "no_final_lf", "fasta60_no_final_lf"])
def test_constructed_input_forms(form, mixed, binary, tmp_path):
    _, un1, un2 = check_constructed(binary, write_form(form, mixed, tmp_path), tmp_path)
    assert un1.endswith(b"\n") and (un2 is None or un2.endswith(b"\n"))


def test_the_getline_reader_of_plain_fastq(mixed, binary, tmp_path):
    check_constructed(binary, write_form("plain", mixed, tmp_path), tmp_path, env={"KART_AMD_NO_MMAP": "1"})


@pytest.mark.parametrize("extra", [["-m"], ["-md"], ["-R", "@RG\\tID:g1"], ["-m", "-md", "-R", "@RG\\tID:g1"], ["-t", "8"]], ids=lambda e: "".join(e[:1]) + str(len(e)))
def test_flag_combinations(extra, mixed, binary, tmp_path):
    args = write_form("plain", mixed, tmp_path)
    base = check_constructed(binary, args, tmp_path)
    got = check_constructed(binary, args + extra, tmp_path)
    assert got[1:] == base[1:]          # (-md and -R change no FLAG; -m adds records to mapped reads only)


def test_bam_output(mixed, binary, tmp_path):
    args = write_form("plain", mixed, tmp_path)
    sam = run(binary, args, "-o", tmp_path / "plain.sam")
    bam_plain = run(binary, args, "-bo", tmp_path / "plain.bam")
    bam, un1, un2 = run_with_un(binary, args, tmp_path, out_flag="-bo")
    assert bam == bam_plain
    assert (un1, un2) == expected_of(args, sam) and len(un1) > 0


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def bad_lines(fq1, fq2, tmp):
    u1, u2 = str(tmp / "u1"), str(tmp / "u2")
    return {
        "-un2 without a two-file library": ["-f", fq1, "-un", u1, "-un2", u2],
        "-un2 with an interleaved library": ["-f", fq1, "-p", "-un", u1, "-un2", u2],
        "-un2 alone": ["-f", fq1, "-un2", u2],
        "two files, only -un": ["-f", fq1, "-f2", fq2, "-un", u1],
        "two files, only -un2": ["-f", fq1, "-f2", fq2, "-un2", u2],
        "a device list": ["-f", fq1, "-un", u1, "-gpu", "0,1"],
        "a shard": ["-f", fq1, "-un", u1, "-shard", "0/2", "-rendezvous", str(tmp / "rdv")],
        "two files and a device list": ["-f", fq1, "-f2", fq2, "-un", u1, "-un2", u2, "-gpu", "0,1,2"],
    }


@pytest.mark.parametrize("what", sorted(bad_lines("a", "b", __import__("pathlib").Path("."))))
def test_rejected_command_lines(what, binary, tmp_path):
    fq1, fq2 = materialise(str(tmp_path), "edge_1.fq"), materialise(str(tmp_path), "edge_2.fq")
    out = tmp_path / "never.sam"
    r = subprocess.run([binary, "-silent", "-i", SMALL_PREFIX] + bad_lines(fq1, fq2, tmp_path)[what] + ["-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = r.stdout.decode()
    assert r.returncode == 1, text[-300:]
    assert "Error! " in text and "-un" in text and "Usage:" in text
    assert not out.exists() and not (tmp_path / "u1").exists() and not (tmp_path / "u2").exists()


def test_the_usage_text_lists_the_flags(binary):
    text = subprocess.run([binary, "-h"], stdout=subprocess.PIPE).stdout.decode()
    assert "-un FILE" in text and "-un2 FILE2" in text
