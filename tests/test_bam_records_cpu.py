"""CPU: the records of a -bo file, byte for byte, against tests/bam_encode.py -- an encoder of a printed SAM line written from the SAM/BAM
specification.  tests/test_bam_output.py decodes the file and compares fields; this one pins the BYTES of every record (bin, the smallest tag
types, the packed bases, the quality bytes, a quality column shorter than its read), which is what the device's BAM kernels are held to
(tests/test_bam_stream_gpu.py)."""
import gzip
import struct
import subprocess

import pytest

from bam_encode import bam_record, ref_ids_of_header
from conftest import SMALL_PREFIX
from test_host_pipeline import CASES, host_oracle_binary, materialise  # noqa: F401  (fixture)


def bam_body(path):
    """the inflated file behind its header: the records"""
    raw = gzip.open(path, "rb").read()
    assert raw[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at); at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        at += 4 + l_name + 4
    return raw[at:]


@pytest.mark.parametrize("case", ["pe", "pe_m", "edge_pe"])
def test_bam_records_equal_the_encoded_sam_lines(case, host_oracle_binary, tmp_path):
    args = [materialise(str(tmp_path), a) if a.endswith((".fq", ".fa", ".gz")) else a for a in CASES[case]]
    sam, bam = str(tmp_path / "o.sam"), str(tmp_path / "o.bam")
    for flag, out in (("-o", sam), ("-bo", bam)):
        r = subprocess.run([host_oracle_binary, "-silent", "-t", "3", "-i", SMALL_PREFIX] + args + [flag, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()[-400:]
    text = open(sam, "rb").read()
    lines = [l for l in text.split(b"\n") if l]
    ids = ref_ids_of_header(b"\n".join(l for l in lines if l.startswith(b"@")).decode())
    records = [l for l in lines if not l.startswith(b"@")]
    assert len(records) > 100
    want = b"".join(bam_record(l, ids) for l in records)
    got = bam_body(bam)
    if got != want:          # name the first record that differs
        at = 0
        for i, l in enumerate(records):
            w = bam_record(l, ids)
            assert got[at:at + len(w)] == w, (i, l[:100], got[at:at + len(w)].hex(), w.hex())
            at += len(w)
    assert got == want
