"""CPU: tests/fasta_reads.py -- the reference's FASTA reader restated in Python, the yardstick of the device stream's FASTA tests -- against the
host pipeline bound to the CPU oracle backend (tests/cpu_backend), on a small file that uses every rule of the reader: 60-column wrapping, CR LF
line ends, a blank line inside a sequence, no final newline, headers cut at ' ', '/' and a tab.  The names and sequences of the SAM must be the
helper's."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT, SMALL_PREFIX
from fasta_reads import fasta_reads, held, wrap


@pytest.fixture(scope="module")
def host_oracle_binary():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_backend")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "_build", "kart-host-oracle")


def every_rule_fasta():
    from kart_amd.index_build import read_fasta
    genome = {n: bytes(s) for n, _, s in read_fasta(os.path.join(GOLDEN, "small.fa"))}
    g = genome["chrA"].upper()
    reads = [g[3000 + 977 * k:3000 + 977 * k + 100 + 13 * k] for k in range(12)]
    assert all(set(r) <= set(b"ACGT") for r in reads)
    t = b""
    for k in range(4):                                      # 60-column wrapping
        t += b">wrapped%d\n" % k + wrap(reads[k], 60)
    for k in range(4, 7):                                   # CR LF: the '\r' of every line stays in the sequence
        t += b">crlf%d\r\n" % k + wrap(reads[k], 60, b"\r\n")
    t += b">blank\n" + reads[7][:60] + b"\n\n" + reads[7][60:] + b"\n"     # a blank line adds nothing
    t += b">name with words\n" + reads[8] + b"\n"           # the name ends at ' ' ...
    t += b">>mate/1\n" + reads[9] + b"\n"                    # ... at '/' (and starts behind every '>')
    t += b">tab\tbed\n" + wrap(reads[10], 31)                # ... at a tab
    t += b">last\n" + wrap(reads[11], 60)[:-1]              # no final newline: the last base is lost
    return t, reads


def test_helper_reads_the_rules():
    t, reads = every_rule_fasta()
    got = fasta_reads(t)
    assert [n for n, _ in got] == [b"wrapped0", b"wrapped1", b"wrapped2", b"wrapped3", b"crlf4\r", b"crlf5\r", b"crlf6\r", b"blank", b"name", b"mate", b"tab", b"last"]
    # (a name ends in front of the line's last byte: the '\r' of a CR LF header belongs to it)
    assert [s for _, s in got[:4]] == reads[:4] and got[7][1] == reads[7] and got[10][1] == reads[10]
    assert got[4][1] == wrap(reads[4], 60, b"\r")            # a '\r' behind every line's bases
    assert got[11][1] == reads[11][:-1]


def test_host_pipeline_reads_fasta_as_the_helper_does(host_oracle_binary, tmp_path):
    t, _ = every_rule_fasta()
    path, out = str(tmp_path / "rules.fa"), str(tmp_path / "rules.sam")
    open(path, "wb").write(t)
    r = subprocess.run([host_oracle_binary, "-silent", "-i", SMALL_PREFIX, "-f", path, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-500:]
    # (a '\r' is a character of the sequence: the records are cut at line feeds only)
    recs = [l.split(b"\t") for l in open(out, "rb").read().split(b"\n") if l and not l.startswith(b"@")]
    want = fasta_reads(t)
    assert len(recs) == len(want)
    for f, (name, seq) in zip(recs, want):
        assert f[0] == name
        assert f[9] == held(seq, bool(int(f[1]) & 16)), name      # shown on the other strand: its reverse complement
        assert f[10] == b"*"
    assert sum(f[2] != b"*" for f in recs) >= 8                   # (the reads map: the sequences were not merely passed through)
