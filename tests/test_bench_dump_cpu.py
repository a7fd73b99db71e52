"""CPU: bench.py --dump-outputs on a golden SAM of the reference, cut into two rank parts and read in small chunks (lines cross chunk and
file boundaries): every record of the sample parsed as a plain line-by-line reading parses it, the same arrays on a second run."""
import gzip
import os
import zlib

import numpy as np

import bench
from conftest import GOLDEN


def test_dump_outputs_reads_the_sam_stream_record_by_record(tmp_path, monkeypatch):
    text = gzip.open(os.path.join(GOLDEN, "sam", "pe.sam.gz")).read()
    lines = text.split(b"\n")[:-1]
    header = [l for l in lines if l.startswith(b"@")]
    records = lines[len(header):]
    refs = {l.split(b"\t")[1][3:]: i for i, l in enumerate(l for l in header if l.startswith(b"@SQ\t"))}
    cut = text.index(b"\n", len(text) // 2) + 1
    parts = [str(tmp_path / "out.sam.0"), str(tmp_path / "out.sam.1")]
    for p, b in zip(parts, (text[:cut], text[cut:])):
        open(p, "wb").write(b)
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), parts, len(records), chunk=4093)
        runs.append({n: np.load(str(tmp_path / d / ("sam_%s.npy" % n))) for n in bench.DUMP_FIELDS + ("summary",)})
    a, b = runs
    assert all(a[n].dtype == np.float64 and np.array_equal(a[n], b[n]) for n in a)
    assert list(a["summary"]) == [len(records), len(header), len(text), zlib.crc32(text)]
    assert len(a["record"]) == len(records) and list(a["record"]) == list(range(len(records)))    # (fewer records than DUMP_SAMPLE: all of them)
    n_gapped = 0
    for i, line in enumerate(records):
        f = line.split(b"\t")
        tags = {t[:2]: int(t[5:]) for t in f[11:]}
        ops, num = [], ""
        for c in f[5].decode():
            if c.isdigit():
                num += c
            elif c != "*":
                ops.append((int(num), c))
                num = ""
        n_gapped += any(c in "ID" for _, c in ops)
        want = {"flag": int(f[1]), "ref": refs.get(f[2], -1), "pos": int(f[3]), "mapq": int(f[4]), "cigar_ops": len(ops) or -1,
                "cigar_ref_len": sum(k for k, c in ops if c in "MD") if ops else -1, "cigar_query_len": sum(k for k, c in ops if c in "MIS") if ops else -1,
                "mate_ref": refs.get(f[2], -1) if f[6] == b"=" else refs.get(f[6], -1), "mate_pos": int(f[7]), "tlen": int(f[8]),
                "NM": tags.get(b"NM", -1), "AS": tags.get(b"AS", -1), "XS": tags.get(b"XS", -1), "line_crc32": zlib.crc32(line)}
        assert {n: a[n][i] for n in want} == want, i
    assert n_gapped > 0
    # a larger output than the sample: a seeded subset of the record numbers, each with the fields of that record
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 500)
    bench.dump_outputs(str(tmp_path / "c"), parts, len(records), chunk=4093)
    c = {n: np.load(str(tmp_path / "c" / ("sam_%s.npy" % n))) for n in bench.DUMP_FIELDS + ("summary",)}
    at = c["record"].astype(np.int64)
    assert len(at) == 500 and (np.diff(at) > 0).all() and np.array_equal(c["summary"], a["summary"])
    assert all(np.array_equal(c[n], a[n][at]) for n in bench.DUMP_FIELDS)
