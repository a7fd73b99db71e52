"""GPU: kart-amd -md as a user runs it.  The device stream's file (MD made by the format kernels) against the file of the host's reader and printer
(KART_AMD_NO_STREAM=1: MD made by host/detail/md.inc) for -o, -bo and -bo -bz device, every MD against tests/md_plain.py, and one stream run whose short
device lists hand reads back, so that host-made and device-made MD stand in one file."""
import gzip
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT, SMALL_PREFIX
from md_plain import MD_RE, md_of, reference_at
from test_md_host_cpu import bam_records, read_fasta, sam_as_bam_shows_it

pytestmark = pytest.mark.gpu
KART_AMD = os.path.join(ROOT, "kart_amd", "bin", "kart-amd")


@pytest.fixture(scope="module")
def library(built_lib, tmp_path_factory):
    """3000 pairs of the small genome with sequencing errors, variants and indels"""
    from kart_amd import synth
    from kart_amd.index_build import read_fasta as read_fasta_np
    genome = {n: s for n, _, s in read_fasta_np(os.path.join(GOLDEN, "small.fa"))}
    names, r1, r2 = synth.simulate_pairs(genome, 3000, seed=41, err=0.02, mut=0.003, indel_frac=0.3, n_frac=0.0005)
    d = tmp_path_factory.mktemp("md_cli")
    f1, f2 = str(d / "a_1.fq"), str(d / "a_2.fq")
    synth.write_fastq(f1, names, r1, mate=1)
    synth.write_fastq(f2, names, r2, mate=2)
    return f1, f2, read_fasta(os.path.join(GOLDEN, "small.fa"))


def run(library, out, flags, env=None):
    f1, f2, _ = library
    r = subprocess.run([KART_AMD, "-silent", "-i", SMALL_PREFIX, "-f", f1, "-f2", f2, "-t", "4"] + flags + [out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, KART_AMD_VERBOSE="1", **(env or {})))
    assert r.returncode == 0, r.stdout.decode()[-600:]
    return open(out, "rb").read(), r.stdout.decode()


def stream_reads(log):
    m = re.search(r"device report: (\d+) reads decided on the device, (\d+) mapped by the host stages", log)
    assert m, log[-600:]
    return int(m.group(1)), int(m.group(2))


def check_lines(lines, fa):
    n = 0
    for f in lines:
        if f[2] == "*":
            assert not any(x.startswith("MD:Z:") for x in f[11:])
            continue
        assert f[-1].startswith("MD:Z:") and MD_RE.fullmatch(f[-1][5:]), f[:9]
        assert f[-1][5:] == md_of(f[9], f[5], reference_at(fa[f[2]], int(f[3]))), (f[:9], f[-1])
        n += 1
    return n


def test_sam_stream_and_host_files_agree(library, tmp_path):
    a, log_a = run(library, str(tmp_path / "s.sam"), ["-md", "-o"])
    b, log_b = run(library, str(tmp_path / "h.sam"), ["-md", "-o"], {"KART_AMD_NO_STREAM": "1"})
    assert stream_reads(log_a)[0] > 5000
    assert a == b
    lines = [ln.split("\t") for ln in a.decode().split("\n") if ln and not ln.startswith("@")]
    assert check_lines(lines, library[2]) > 5000
    # without the flag: no such field, and every other byte the same
    c, _ = run(library, str(tmp_path / "p.sam"), ["-o"])
    assert b"MD:Z" not in c
    assert c == re.sub(rb"\tMD:Z:[^\t\n]*", b"", a)


@pytest.mark.parametrize("bz", ["host", "device"])
def test_bam_stream_and_host_files_agree(bz, library, tmp_path):
    a, log_a = run(library, str(tmp_path / "s.bam"), ["-md", "-bz", bz, "-bo"])
    b, _ = run(library, str(tmp_path / "h.bam"), ["-md", "-bo"], {"KART_AMD_NO_STREAM": "1"})
    assert stream_reads(log_a)[0] > 5000
    if bz == "device":
        assert re.search(r"device deflate: [1-9]\d* of", log_a), log_a[-400:]
        assert gzip.decompress(a) == gzip.decompress(b)
    (_, ra), (_, rb) = bam_records(a), bam_records(b)
    assert ra == rb
    assert check_lines(ra, library[2]) > 5000
    sam, _ = run(library, str(tmp_path / "s.sam"), ["-md", "-o"])
    lines = [ln for ln in sam.decode().split("\n") if ln and not ln.startswith("@")]
    assert [sam_as_bam_shows_it(ln) for ln in lines] == ra


def test_reads_handed_back_get_their_md_from_the_host(library, tmp_path):
    """the alignment stage's lists a few entries long (KG_DBG_*_CAPACITY): the candidates beyond them go back to the host inside a stream run"""
    env = {"KG_DBG_JOB_CAPACITY": "40", "KG_DBG_OPS_CAPACITY": "700", "KG_DBG_SPILL_CAPACITY": "30"}
    a, log_a = run(library, str(tmp_path / "s.sam"), ["-md", "-o"], env)
    on_device, by_host = stream_reads(log_a)
    assert on_device > 0 and by_host > 0, (on_device, by_host)
    b, _ = run(library, str(tmp_path / "h.sam"), ["-md", "-o"], {"KART_AMD_NO_STREAM": "1"})
    assert a == b
