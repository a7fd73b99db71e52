"""GPU: kart-amd -stats as a user runs it, on the small index: the library of tests/test_un_cli_gpu.py -- three chunks (12 000 reads) with random pairs
among simulated ones, so that several batches go through the device stream and the commit maps a chunk again (which must count once, under its final
records).  The expected file is tests/stats_plain.py over the run's own SAM text (which the existing suite holds to the reference); the host's reader
and printer (KART_AMD_NO_STREAM=1), a run whose short device lists hand reads back to the host and a -bo run must write the same file; -m writes the
file of its own SAM; and the main output is the one of the run without the flag."""
import os
import re
import subprocess

import pytest

import stats_plain
from conftest import SMALL_PREFIX
from test_md_cli_gpu import KART_AMD, stream_reads
from test_un_cli_gpu import library  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_RUNS = {}          # the tests share their runs, a fresh process each


def run(files, tmp, tag, flags, env=None, stats=True):
    """-> (main output, the -stats file, log)"""
    key = (tuple(files), tuple(flags), tuple(sorted((env or {}).items())), stats)
    if key not in _RUNS:
        out, st = str(tmp / (tag + ".out")), str(tmp / (tag + ".stats"))
        r = subprocess.run([KART_AMD, "-silent", "-i", SMALL_PREFIX, "-f", files[0], "-f2", files[1], "-t", "4"] + (["-stats", st] if stats else []) + flags + [out],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, KART_AMD_VERBOSE="1", **(env or {})), timeout=300)
        assert r.returncode == 0, r.stdout.decode()[-600:]
        _RUNS[key] = (open(out, "rb").read(), open(st, "rb").read() if stats else None, r.stdout.decode())
    return _RUNS[key]


@pytest.fixture(scope="module")
def stream_run(library, tmp_path_factory):
    return run(library, tmp_path_factory.mktemp("stats_stream"), "s", ["-o"])


def test_stream_run_writes_the_recount_of_its_own_sam(library, stream_run, tmp_path):
    sam, stats, log = stream_run
    assert stats == stats_plain.text(sam)
    lines = stats.decode().split("\n")
    assert "SN\trecords\t12000" in lines and sum(ln.startswith("IS\t") for ln in lines) > 50 and sum(ln.startswith("MQ\t") for ln in lines) >= 2
    # what the run must have gone through: the device stream, in several batches, with a chunk mapped again
    on_device, by_host = stream_reads(log)
    assert on_device > 6000 and by_host > 0
    m = re.search(r"device stream: (\d+) batches", log)
    assert m and int(m.group(1)) >= 2, log[-800:]
    m = re.search(r"chunks re-mapped after EstDistance speculation: (\d+)", log)
    assert m and int(m.group(1)) >= 1, log[-800:]
    # and the main output is the run's without the flag
    plain = run(library, tmp_path, "p", ["-o"], stats=False)
    assert plain[0] == sam


def test_host_reader_and_printer_write_the_same_file(library, stream_run, tmp_path):
    h = run(library, tmp_path, "h", ["-o"], {"KART_AMD_NO_STREAM": "1"})
    assert "device stream:" not in h[2]
    assert h[:2] == stream_run[:2]


def test_reads_handed_back_are_counted_by_the_host(library, stream_run, tmp_path):
    """the alignment stage's lists a few entries long (KG_DBG_*_CAPACITY): pairs go back to the host inside a stream run; the device's rows leave them out"""
    env = {"KG_DBG_JOB_CAPACITY": "40", "KG_DBG_OPS_CAPACITY": "700", "KG_DBG_SPILL_CAPACITY": "30"}
    a = run(library, tmp_path, "k", ["-o"], env)
    on_device, by_host = stream_reads(a[2])
    assert on_device > 0 and by_host > 0, (on_device, by_host)
    assert a[:2] == stream_run[:2]


def test_bam_run_writes_the_same_file(library, stream_run, tmp_path):
    b = run(library, tmp_path, "b", ["-bz", "device", "-bo"])
    plain = run(library, tmp_path, "bp", ["-bz", "device", "-bo"], stats=False)
    assert b[0] == plain[0] and b[1] == stream_run[1]


def test_multi_hit_run_writes_the_file_of_its_own_sam(library, tmp_path):
    m = run(library, tmp_path, "m", ["-m", "-o"])
    assert m[1] == stats_plain.text(m[0])
    assert len(stats_plain.records(m[0])) > 12000          # (a condition on the input: some read has more than one record)
