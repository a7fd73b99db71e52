#!/usr/bin/env python3
"""The paired FASTA fixtures of tests/test_fasta_stream_gpu.py: the reads of tests/golden/sam/pe_1.fq.gz / pe_2.fq.gz as FASTA -- file 1 with one
sequence line per record, file 2 wrapped at 60 columns -- and the SAM the UNMODIFIED reference mapper (oracle/_ref/kart -t 1, which build() makes
where the reference's sources are at hand) writes for them.  The run is made twice under different MALLOC_PERTURB_ fills and must give the same bytes.

    python tools/make_golden_fasta.py        ->  tests/golden/sam/pe_fasta_1.fa.gz, pe_fasta_2.fa.gz, pe_fasta.sam.gz
"""
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAM = os.path.join(ROOT, "tests", "golden", "sam")
KART = os.path.join(ROOT, "oracle", "_ref", "kart")
PREFIX = os.path.join(ROOT, "tests", "golden", "idx", "small")


def as_fasta(fastq: bytes, cols=None) -> bytes:
    lines = fastq.split(b"\n")
    out = []
    for i in range(0, len(lines) - 3, 4):
        seq = lines[i + 1]
        out.append(b">" + lines[i][1:] + b"\n" + (b"".join(seq[k:k + cols] + b"\n" for k in range(0, len(seq), cols)) if cols else seq + b"\n"))
    return b"".join(out)


def main():
    if not os.path.exists(KART):
        sys.exit("oracle/_ref/kart is missing: build() makes it where the reference's sources are at hand")
    texts = [as_fasta(gzip.open(os.path.join(SAM, "pe_1.fq.gz")).read()), as_fasta(gzip.open(os.path.join(SAM, "pe_2.fq.gz")).read(), 60)]
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, "pe_fasta_%d.fa" % (f + 1)) for f in range(2)]
        for p, t in zip(paths, texts):
            open(p, "wb").write(t)
        runs = []
        for fill in (85, 170):
            out = os.path.join(tmp, "o%d.sam" % fill)
            subprocess.run([KART, "-silent", "-t", "1", "-i", PREFIX, "-f", paths[0], "-f2", paths[1], "-o", out], check=True,
                           env=dict(os.environ, MALLOC_PERTURB_=str(fill)), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            runs.append(open(out, "rb").read())
    assert runs[0] == runs[1], "the reference's output depends on uninitialised memory for this input"
    for name, data in (("pe_fasta_1.fa", texts[0]), ("pe_fasta_2.fa", texts[1]), ("pe_fasta.sam", runs[0])):
        with gzip.GzipFile(os.path.join(SAM, name + ".gz"), "wb", compresslevel=9, mtime=0) as fh:
            fh.write(data)
    print("pe_fasta: %d lines" % runs[0].count(b"\n"))


if __name__ == "__main__":
    main()
