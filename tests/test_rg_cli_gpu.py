"""GPU: kart-amd -R as a user runs it.  The device stream's file (the field copied by the format kernels) against the file of the host's reader and
printer (KART_AMD_NO_STREAM=1) for -o, -bo and -bo -bz device, with and without -md; one stream run whose short device lists hand reads back, so that
host-made and device-made records stand in one file; two libraries with a read group each; and the run without the flag."""
import gzip
import os
import re
import subprocess

import pytest

from conftest import SMALL_PREFIX
from test_md_cli_gpu import KART_AMD, library, stream_reads  # noqa: F401  (the 3000-pair library of the -md test)
from test_md_host_cpu import bam_records, sam_as_bam_shows_it

pytestmark = pytest.mark.gpu
RG_ARG = "@RG\\tID:lane1.x\\tSM:na12878\\tPL:ILLUMINA"
RG_LINE = RG_ARG.replace("\\t", "\t")
RG_ID = "lane1.x"


_RUNS = {}          # (files, flags, env) -> (file, log): the tests share their runs, a fresh process each


def run_files(files, out, flags, env=None):
    key = (tuple(files), tuple(flags), tuple(sorted((env or {}).items())))
    if key not in _RUNS:
        _RUNS[key] = run_fresh(files, out, flags, env)
    return _RUNS[key]


def run_fresh(files, out, flags, env=None):
    r = subprocess.run([KART_AMD, "-silent", "-i", SMALL_PREFIX] + files + ["-t", "4"] + flags + [out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, KART_AMD_VERBOSE="1", **(env or {})))
    assert r.returncode == 0, r.stdout.decode()[-600:]
    return open(out, "rb").read(), r.stdout.decode()


def run(library, out, flags, env=None):
    return run_files(["-f", library[0], "-f2", library[1]], out, flags, env)


def sam_parts(text):
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    return [ln for ln in lines[:-1] if ln.startswith("@")], [ln for ln in lines[:-1] if not ln.startswith("@")]


def check_sam(text, rg_id=RG_ID, rg_line=RG_LINE, md=False):
    header, records = sam_parts(text)
    assert header[-1] == rg_line and header[-2].startswith("@SQ") and header.count(rg_line) == 1
    assert len(records) >= 6000
    for ln in records:
        f = ln.split("\t")
        assert f[-1] == "RG:Z:" + rg_id, ln
        if md and f[2] != "*":
            assert f[-2].startswith("MD:Z:"), ln
        else:
            assert f[-2].startswith("XS:i:"), ln
    return records


@pytest.mark.parametrize("md", [False, True], ids=["plain", "md"])
def test_sam_stream_and_host_files_agree(md, library, tmp_path):
    flags = (["-md"] if md else []) + ["-R", RG_ARG, "-o"]
    a, log_a = run(library, str(tmp_path / "s.sam"), flags)
    b, _ = run(library, str(tmp_path / "h.sam"), flags, {"KART_AMD_NO_STREAM": "1"})
    assert stream_reads(log_a)[0] > 5000
    assert a == b
    check_sam(a, md=md)
    if not md:
        # without the flag: no header line, no such field, and every other byte the same
        c, _ = run(library, str(tmp_path / "p.sam"), ["-o"])
        assert b"RG:Z" not in c and b"@RG" not in c
        assert c == re.sub(rb"\tRG:Z:[^\t\n]*", b"", a).replace(RG_LINE.encode() + b"\n", b"", 1)


@pytest.mark.parametrize("md", [False, True], ids=["plain", "md"])
@pytest.mark.parametrize("bz", ["host", "device"])
def test_bam_stream_and_host_files_agree(bz, md, library, tmp_path):
    tags = (["-md"] if md else []) + ["-R", RG_ARG]
    a, log_a = run(library, str(tmp_path / "s.bam"), tags + ["-bz", bz, "-bo"])
    b, _ = run(library, str(tmp_path / "h.bam"), tags + ["-bo"], {"KART_AMD_NO_STREAM": "1"})
    assert stream_reads(log_a)[0] > 5000
    if bz == "device":
        assert re.search(r"device deflate: [1-9]\d* of", log_a), log_a[-400:]
    raw = gzip.decompress(a)
    assert raw == gzip.decompress(b)
    l_text = int.from_bytes(raw[4:8], "little")
    assert raw[8:8 + l_text].decode().endswith("\n" + RG_LINE + "\n") and raw.count(RG_LINE.encode()) == 1
    (_, ra), (_, rb) = bam_records(a), bam_records(b)
    assert ra == rb and all(r[-1] == "RG:Z:" + RG_ID for r in ra)
    sam, _ = run(library, str(tmp_path / "s.sam"), tags + ["-o"])
    assert [sam_as_bam_shows_it(ln) for ln in check_sam(sam, md=md)] == ra


def test_reads_handed_back_get_their_field_from_the_host(library, tmp_path):
    """the alignment stage's lists a few entries long (KG_DBG_*_CAPACITY): the candidates beyond them go back to the host inside a stream run"""
    env = {"KG_DBG_JOB_CAPACITY": "40", "KG_DBG_OPS_CAPACITY": "700", "KG_DBG_SPILL_CAPACITY": "30"}
    flags = ["-md", "-R", RG_ARG, "-o"]
    a, log_a = run(library, str(tmp_path / "s.sam"), flags, env)
    on_device, by_host = stream_reads(log_a)
    assert on_device > 0 and by_host > 0, (on_device, by_host)
    b, _ = run(library, str(tmp_path / "h.sam"), flags, {"KART_AMD_NO_STREAM": "1"})
    assert a == b
    check_sam(a, md=True)


@pytest.mark.parametrize("out_flag", ["-o", "-bo"])
def test_two_libraries_two_read_groups(out_flag, library, tmp_path):
    """the mate files as two single-end libraries: the stream serves both, with another read group each"""
    files = ["-f", library[0], library[1]]
    la, lb = "@RG\tID:A\tSM:s", "@RG\tID:" + "B" * 40 + "\tSM:s"
    flags = ["-R", la, "-R", lb, out_flag]
    a, log_a = run_files(files, str(tmp_path / "s.out"), flags)
    b, _ = run_files(files, str(tmp_path / "h.out"), flags, {"KART_AMD_NO_STREAM": "1"})
    assert stream_reads(log_a)[0] > 5000
    if out_flag == "-bo":
        raw = gzip.decompress(a)
        assert raw == gzip.decompress(b)          # (the two writers cut their BGZF blocks differently)
        l_text = int.from_bytes(raw[4:8], "little")
        assert raw[8:8 + l_text].decode().endswith("\n" + la + "\n" + lb + "\n")
        ids = [r[-1] for r in bam_records(a)[1]]
    else:
        assert a == b
        header, records = sam_parts(a)
        assert header[-2:] == [la, lb] and header[-3].startswith("@SQ")
        ids = [ln.split("\t")[-1] for ln in records]
    assert ids == ["RG:Z:A"] * 3000 + ["RG:Z:" + "B" * 40] * 3000
