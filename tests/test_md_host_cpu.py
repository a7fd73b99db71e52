"""CPU: -md through the HOST pipeline (the product's host code bound to the CPU oracle backend, tests/_build/kart-host-oracle).  On the golden inputs
the host-pipeline tests use -- paired, single, -m, FASTA, -pacbio -- a -md run is the golden SAM with one more field on every mapped record, that field is
the MD tests/md_plain.py computes from the printed SEQ, the CIGAR, POS and tests/golden/small.fa, and -bo -md holds the same records with the same
string.  The small index has a hole of its own (40 N in chrA); a second, synthetic index puts a 1-base N, a 3-base N run and an R under the reads."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, SMALL_PREFIX
from md_plain import MD_RE, cigar_ops, md_of, reference_at
from test_host_pipeline import CASES, SAM, materialise

MD_CASES = ["pe", "se", "se_m", "pe_m", "se_fasta", "pacbio", "edge_pe"]


@pytest.fixture(scope="module")
def binary():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_backend")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "_build", "kart-host-oracle")


def read_fasta(path):
    out, name = {}, None
    for ln in open(path):
        if ln.startswith(">"):
            name = ln[1:].split()[0]
            out[name] = []
        else:
            out[name].append(ln.strip())
    return {k: "".join(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def small_fa():
    return read_fasta(os.path.join(GOLDEN, "small.fa"))


def run(binary, args, out_flag, out):
    r = subprocess.run([binary, "-silent", "-i", SMALL_PREFIX] + args + [out_flag, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-500:]
    return open(out, "rb").read()


def split_md(line):
    """a SAM line -> (the line without its MD field, the MD or None); the field is the record's last"""
    f = line.split("\t")
    if f[-1].startswith("MD:Z:"):
        return "\t".join(f[:-1]), f[-1][5:]
    assert not any(x.startswith("MD:Z:") for x in f[11:]), line
    return line, None


def check_sam_with_md(text, want, fa):
    """text: a -md run; want: the same run without -md.  Returns the number of mapped records"""
    got, ref = text.decode().split("\n"), want.decode().split("\n")
    assert len(got) == len(ref)
    mapped = 0
    for g, w in zip(got, ref):
        if not g or g.startswith("@"):
            assert g == w
            continue
        cut, md = split_md(g)
        assert cut == w, (g[:100], w[:100])
        f = g.split("\t")
        if f[2] == "*":
            assert md is None, g
            continue
        mapped += 1
        assert md is not None and MD_RE.fullmatch(md), g
        assert md == md_of(f[9], f[5], reference_at(fa[f[2]], int(f[3]))), (f[0], f[1], f[2], f[3], f[5], md)
    return mapped


@pytest.mark.parametrize("case", MD_CASES)
def test_md_run_is_the_golden_sam_with_md_of_the_plain_model(case, binary, small_fa, tmp_path):
    args = [materialise(str(tmp_path), a) if a.endswith((".fq", ".fa", ".gz")) else a for a in CASES[case]]
    want = gzip.open(os.path.join(SAM, case + ".sam.gz")).read()
    got = run(binary, args + ["-md"], "-o", str(tmp_path / "md.sam"))
    assert check_sam_with_md(got, want, small_fa) > 0
    # without the flag nothing changes
    plain = run(binary, args, "-o", str(tmp_path / "plain.sam"))
    assert plain == want and b"MD:Z" not in plain


# ---- BAM: a decoder that knows the Z type --------------------------------------------------------------------------------------------------
NT16 = "=ACMGRSVTWYHKDBN"


def bam_records(blob):
    """-> (contig names, records as SAM-like field lists: SEQ in the 4-bit alphabet, QUAL '*' where the record holds 0xFF)"""
    raw = gzip.decompress(blob)                      # BGZF members are gzip members
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    names = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        names.append(raw[at + 4:at + 4 + l_name - 1].decode())
        at += 4 + l_name + 4
    recs = []
    while at < len(raw):
        size, = struct.unpack_from("<i", raw, at)
        rid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, rnext, pnext, tlen = struct.unpack_from("<iiBBHHHiiii", raw, at + 4)
        p = at + 36
        name = raw[p:p + l_name - 1].decode("latin-1")
        p += l_name
        cigar = "".join("%d%s" % (v >> 4, "MIDNSHP=X"[v & 15]) for v in struct.unpack_from("<%dI" % n_cig, raw, p)) or "*"
        p += 4 * n_cig
        seq = "".join(NT16[raw[p + (i >> 1)] >> (4 if i % 2 == 0 else 0) & 15] for i in range(l_seq)) or "*"
        p += (l_seq + 1) >> 1
        q = raw[p:p + l_seq]
        qual = "*" if (l_seq == 0 or q[0] == 0xFF) else bytes(b + 33 for b in q).decode("latin-1")
        p += l_seq
        tags = []
        while p < at + 4 + size:
            tag, ty = raw[p:p + 2].decode(), chr(raw[p + 2])
            p += 3
            if ty == "Z":
                e = raw.index(b"\0", p)
                tags.append("%s:Z:%s" % (tag, raw[p:e].decode()))
                p = e + 1
            else:
                fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty]
                v, = struct.unpack_from(fmt, raw, p)
                tags.append("%s:i:%d" % (tag, v))
                p += struct.calcsize(fmt)
        assert p == at + 4 + size
        recs.append([name, str(flag), names[rid] if rid >= 0 else "*", str(pos + 1), str(mapq), cigar,
                     "*" if rnext < 0 else "=" if rnext == rid else names[rnext], str(pnext + 1), str(tlen), seq, qual] + tags)
        at += 4 + size
    return names, recs


def sam_as_bam_shows_it(line):
    f = line.split("\t")
    f[9] = "".join(c.upper() if c.upper() in NT16 else "N" for c in f[9]) if f[9] != "*" else "*"
    if f[10] != "*" and len(f[10]) != len(f[9]):
        f[10] = "*"
    return f


@pytest.mark.parametrize("case", ["pe", "se_m", "se_fasta"])
def test_bam_with_md_holds_the_same_records_and_the_same_string(case, binary, tmp_path):
    args = [materialise(str(tmp_path), a) if a.endswith((".fq", ".fa", ".gz")) else a for a in CASES[case]]
    sam = run(binary, args + ["-md"], "-o", str(tmp_path / "md.sam")).decode()
    _, recs = bam_records(run(binary, args + ["-md"], "-bo", str(tmp_path / "md.bam")))
    lines = [ln for ln in sam.split("\n") if ln and not ln.startswith("@")]
    assert len(lines) == len(recs)
    n_md = 0
    for ln, rec in zip(lines, recs):
        assert sam_as_bam_shows_it(ln) == rec
        n_md += rec[-1].startswith("MD:Z:")
    assert n_md > 0


def test_md_is_listed_by_the_usage_text(binary):
    r = subprocess.run([binary, "-h"], stdout=subprocess.PIPE)
    text = r.stdout.decode()
    assert "-md" in text and "MD:Z" in text and "NM" in text


# ---- holes ------------------------------------------------------------------------------------------------------------------------------------
HOLES = [(1000, 1, "N"), (1500, 3, "N"), (2000, 1, "R")]          # on contig "h": a 1-base N, a 3-base N run, one R
HOLE_SEED = 7                                                      # (the reads' seed: the batch below meets the conditions asserted on it)


def test_reference_holes_show_their_own_character(binary, tmp_path):
    from kart_amd import index_build, synth
    truth = synth.make_genome([("h", 3000), ("other", 2500)], seed=3)
    fasta = {k: v.copy() for k, v in truth.items()}
    for s, n, ch in HOLES:
        fasta["h"][s:s + n] = ord(ch)
    fa_path, prefix = str(tmp_path / "holes.fa"), str(tmp_path / "holes")
    synth.write_fasta(fa_path, fasta)
    index_build.build_index(fa_path, prefix, device="cpu")
    amb = open(prefix + ".amb").read().split("\n")
    assert amb[0].split()[2] == "3" and amb[1:4] == ["1000 1 N", "1500 3 N", "2000 1 R"]
    # reads of the true sequence (the sequencer saw bases where the assembly has N / R), 100 bases, all over the two short contigs
    names, r1, r2 = synth.simulate_pairs(truth, 150, seed=HOLE_SEED, read_len=100, ins_mean=300.0, ins_sd=20.0, skip=())
    synth.write_fastq(str(tmp_path / "h_1.fq"), names, r1)
    synth.write_fastq(str(tmp_path / "h_2.fq"), names, r2)
    out = str(tmp_path / "h.sam")
    r = subprocess.run([binary, "-silent", "-i", prefix, "-f", str(tmp_path / "h_1.fq"), "-f2", str(tmp_path / "h_2.fq"), "-md", "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-500:]
    fa = {k: v.tobytes().decode() for k, v in fasta.items()}
    over, shown = 0, set()
    for ln in open(out).read().split("\n"):
        if not ln or ln.startswith("@"):
            continue
        f = ln.split("\t")
        if f[2] == "*":
            continue
        _, md = split_md(ln)
        assert md == md_of(f[9], f[5], reference_at(fa[f[2]], int(f[3]))), ln
        beg = int(f[3]) - 1
        end = beg + sum(n for n, op in cigar_ops(f[5]) if op in "MDN=X")
        hit = [ch for s, n, ch in HOLES if f[2] == "h" and s < end and s + n > beg]
        if hit:
            over += 1
            for ch in hit:
                assert ch in md, ln
                shown.add(ch)
    # (a condition on the input, not on the product)
    assert over >= 10 and shown == {"N", "R"}, (over, shown)
