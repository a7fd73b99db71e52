"""GPU: kart-amd -un / -un2 as a user runs it, on the small index: a library of three chunks (12 000 reads) with random pairs among simulated ones, so
that several batches go through the device stream and the commit maps a chunk again.  The expected files come from tests/un_plain.py over the input and
the run's own SAM text (which the existing suite holds to the reference); the host's reader and printer (KART_AMD_NO_STREAM=1), the bgzip-ped input
inflated on the device (-fz device), a -bo run and a run whose short device lists hand reads back to the host must write the same files; and the main
output is the one of the run without the flags."""
import os
import re
import subprocess

import numpy as np
import pytest

import un_plain
from bgzf_util import bgzf
from conftest import GOLDEN, SMALL_PREFIX
from test_md_cli_gpu import KART_AMD, stream_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def library(built_lib, tmp_path_factory):
    """4500 simulated pairs of the small genome and 1500 pairs of random sequence, one behind every third: (file 1, file 2)"""
    from kart_amd import synth
    from kart_amd.index_build import read_fasta
    genome = {n: s for n, _, s in read_fasta(os.path.join(GOLDEN, "small.fa"))}
    names, r1, r2 = synth.simulate_pairs(genome, 4500, seed=77, err=0.02, mut=0.003, indel_frac=0.3, n_frac=0.0005)
    d = tmp_path_factory.mktemp("un_cli")
    s1, s2 = str(d / "sim_1.fq"), str(d / "sim_2.fq")
    synth.write_fastq(s1, names, r1, mate=1)
    synth.write_fastq(s2, names, r2, mate=2)
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = [[], []]
    sim = [un_plain.records(open(p, "rb").read(), False) for p in (s1, s2)]
    for k in range(4500):
        for f in range(2):
            out[f].append(sim[f][k])
            if k % 3 == 2:
                n = int(rng.integers(50, 151))
                out[f].append(b"@rnd%d/%d extra\n" % (k, f + 1) + acgt[rng.integers(0, 4, n)].tobytes() + b"\n+\n" + b"G" * n + b"\n")
    f1, f2 = str(d / "a_1.fq"), str(d / "a_2.fq")
    for p, recs in ((f1, out[0]), (f2, out[1])):
        with open(p, "wb") as f:
            f.write(b"".join(recs))
    return f1, f2


_RUNS = {}          # the tests share their runs, a fresh process each


def run(files, tmp, tag, flags, env=None, un=True):
    """-> (main output, -un bytes, -un2 bytes, log)"""
    key = (tuple(files), tuple(flags), tuple(sorted((env or {}).items())), un)
    if key not in _RUNS:
        out, u1, u2 = str(tmp / (tag + ".out")), str(tmp / (tag + ".un1")), str(tmp / (tag + ".un2"))
        r = subprocess.run([KART_AMD, "-silent", "-i", SMALL_PREFIX, "-f", files[0], "-f2", files[1], "-t", "4"] + (["-un", u1, "-un2", u2] if un else []) + flags + [out],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, KART_AMD_VERBOSE="1", **(env or {})))
        assert r.returncode == 0, r.stdout.decode()[-600:]
        _RUNS[key] = (open(out, "rb").read(), open(u1, "rb").read() if un else None, open(u2, "rb").read() if un else None, r.stdout.decode())
    return _RUNS[key]


@pytest.fixture(scope="module")
def stream_run(library, tmp_path_factory):
    return run(library, tmp_path_factory.mktemp("un_stream"), "s", ["-o"])


def test_stream_run_writes_what_the_plain_specification_says(library, stream_run, tmp_path):
    sam, un1, un2, log = stream_run
    texts = [open(p, "rb").read() for p in library]
    e1, e2 = un_plain.expected(texts, sam, True, True)
    assert (un1, un2) == (e1, e2)
    n_sel = len(un_plain.records(un1, False))
    assert 1000 <= n_sel <= 5000 and len(un_plain.records(un2, False)) == n_sel          # (units of both kinds take part)
    # what the run must have gone through: the device stream, in several batches, with a chunk mapped again
    on_device, by_host = stream_reads(log)
    assert on_device > 6000 and by_host > 0          # (most of the 12 000 reads are the device's; the pairs mapped again and handed back are the host's)
    m = re.search(r"device stream: (\d+) batches", log)
    assert m and int(m.group(1)) >= 2, log[-800:]
    m = re.search(r"chunks re-mapped after EstDistance speculation: (\d+)", log)
    assert m and int(m.group(1)) >= 1, log[-800:]
    # and the main output is the run's without the flags
    plain = run(library, tmp_path, "p", ["-o"], un=False)
    assert plain[0] == sam


def test_host_reader_and_printer_write_the_same_files(library, stream_run, tmp_path):
    h = run(library, tmp_path, "h", ["-o"], {"KART_AMD_NO_STREAM": "1"})
    assert "device stream:" not in h[3]
    assert h[:3] == stream_run[:3]


def test_bgzipped_input_inflated_on_the_device_gives_the_same_files(library, stream_run, tmp_path):
    packed = []
    for k, p in enumerate(library):
        packed.append(str(tmp_path / ("a_%d.fq.gz" % (k + 1))))
        with open(packed[-1], "wb") as f:
            f.write(bgzf(open(p, "rb").read()))
    z = run(packed, tmp_path, "z", ["-fz", "device", "-o"])
    assert re.search(r"device inflate: [1-9]\d* of", z[3]), z[3][-600:]
    assert z[:3] == stream_run[:3]


def test_reads_handed_back_get_their_bytes_from_the_host(library, stream_run, tmp_path):
    """the alignment stage's lists a few entries long (KG_DBG_*_CAPACITY): pairs go back to the host inside a stream run, and their bytes are spliced in"""
    env = {"KG_DBG_JOB_CAPACITY": "40", "KG_DBG_OPS_CAPACITY": "700", "KG_DBG_SPILL_CAPACITY": "30"}
    a = run(library, tmp_path, "k", ["-o"], env)
    on_device, by_host = stream_reads(a[3])
    assert on_device > 0 and by_host > 0, (on_device, by_host)
    assert a[:3] == stream_run[:3]


def test_bam_run_writes_the_same_files(library, stream_run, tmp_path):
    b = run(library, tmp_path, "b", ["-bz", "device", "-bo"])
    plain = run(library, tmp_path, "bp", ["-bz", "device", "-bo"], un=False)
    assert b[0] == plain[0] and b[1:3] == stream_run[1:3]
