#!/usr/bin/env python3
"""FASTA libraries through the device stream against the host's getline() reader, seeding call and printer (KART_AMD_NO_STREAM=1: the only FASTA path
before kg_stream_set_input), alternating, one fresh process per run -- for -o and -bo, for two-line and 60-column FASTA, and for the FASTQ form of the
same reads beside them.

  python tools/ab_fasta_stream.py [--pairs 10000000] [--runs 3] [--threads 16] [--workdir DIR] [--out profiles/NAME.json] [--step-timeout 600] [--setup-timeout 900]

Reads: benchkit/reads.py (the bench's read model) on the E. coli-sized synthetic genome of bench.py, written as FASTQ and converted.  Every GPU step -- the set-up
(index and reads) and each run, one HostSession.map() -- is a child process under its own `timeout -k 10`; the first that fails ends the script, and the
parent itself never opens the device.  kh_stats_t gives map_seconds,
stream_reads and the stream's kernel_ms ([11] line index + record table + plan, [12] materialise, [9] size + scan, [10] format).  The two paths' files
of every form and format are compared byte for byte.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMS = ("fasta2", "fasta60", "fastq")


def child(a):
    from kart_amd import api
    sess = api.HostSession(a.prefix, 0, a.threads)
    st = sess.map(["-f", a.f1, "-f2", a.f2, "-bo" if a.fmt == "bam" else "-o", a.output])
    sess.close()
    d = st.as_dict()
    print(json.dumps({"leg": a.child, "form": a.form, "fmt": a.fmt, "total_reads": d["total_reads"], "stream_reads": d["stream_reads"], "map_seconds": d["map_seconds"],
                      "parse_ms": d["kernel_ms"][11], "materialise_ms": d["kernel_ms"][12], "size_ms": d["kernel_ms"][9], "format_ms": d["kernel_ms"][10],
                      "text_in_bytes": d["text_in_bytes"], "file_bytes": os.path.getsize(a.output)}))


def setup(a):
    """the index and the FASTQ files (the tool's only other GPU step: a child of its own, so that the parent never opens the device)"""
    import numpy as np
    import torch
    import bench
    from benchkit.reads import write_fastq_pairs
    from kart_amd import index_build, synth
    dev = torch.device("cuda:0")
    genome = bench.make_genome(seed=2, length=bench.GENOME_LEN)
    if not os.path.exists(a.prefix + ".bwt"):
        synth.write_fasta(a.prefix + ".fa", genome)
        index_build.build_index(a.prefix + ".fa", a.prefix, device=str(dev))
    codes = torch.from_numpy(np.concatenate([synth.encode(genome["decoy"]), synth.encode(genome["chrE"])])).to(dev)
    write_fastq_pairs(codes, a.pairs, 11, a.f1, a.f2, dev)


def fastq_to_fasta(src, dst, cols):
    with open(src, "rb") as fi, open(dst, "wb") as fo:
        while True:
            h = fi.readline()
            if not h:
                break
            s = fi.readline().rstrip(b"\n")
            fi.readline(); fi.readline()
            fo.write(b">" + h[1:])
            if cols:
                fo.write(b"".join(s[k:k + cols] + b"\n" for k in range(0, len(s), cols)))
            else:
                fo.write(s + b"\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--setup-timeout", type=int, default=900)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    for k in ("prefix", "f1", "f2", "output", "fmt", "form"):
        ap.add_argument("--" + k, default=None)
    a = ap.parse_args()
    if a.child:
        return setup(a) if a.child == "setup" else child(a)
    work = a.workdir or tempfile.mkdtemp(prefix="ab_fasta_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, "ecoli_like")
    files = {"fastq": (os.path.join(work, "r_1.fq"), os.path.join(work, "r_2.fq"))}

    def step(seconds, args, env=None):
        """one GPU step: a child process under its own time limit; a failure ends the script"""
        r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        if r.returncode != 0:
            sys.exit("step %s failed (%d): %s" % (" ".join(args[:6]), r.returncode, r.stderr.decode()[-800:]))
        return r.stdout.decode()

    step(a.setup_timeout, ["--child", "setup", "--prefix", prefix, "--f1", files["fastq"][0], "--f2", files["fastq"][1], "--pairs", str(a.pairs)])
    for form, cols in (("fasta2", None), ("fasta60", 60)):
        files[form] = tuple(os.path.join(work, "%s_%d.fa" % (form, m)) for m in (1, 2))
        for src, dst in zip(files["fastq"], files[form]):
            fastq_to_fasta(src, dst, cols)

    def run(leg, form, fmt):
        out = os.path.join(work, "%s_%s.%s" % (leg, form, fmt))
        env = dict(os.environ)
        if leg == "host":
            env["KART_AMD_NO_STREAM"] = "1"
        text = step(a.step_timeout, ["--child", leg, "--form", form, "--fmt", fmt, "--prefix", prefix, "--f1", files[form][0], "--f2", files[form][1], "--output", out,
                                     "--threads", str(a.threads)], env)
        return json.loads(text.strip().splitlines()[-1])

    runs, identical = [], {}
    for fmt in ("sam", "bam"):
        for form in FORMS:
            for _ in range(a.runs):
                for leg in ("host", "stream"):
                    runs.append(run(leg, form, fmt))
                    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
            pair = [os.path.join(work, "%s_%s.%s" % (leg, form, fmt)) for leg in ("host", "stream")]
            identical["%s_%s" % (form, fmt)] = subprocess.run(["cmp", "-s"] + pair).returncode == 0
            for p in pair:
                os.remove(p)

    def summary(form, fmt):
        out = {}
        for leg in ("host", "stream"):
            mine = [r for r in runs if (r["leg"], r["form"], r["fmt"]) == (leg, form, fmt)]
            v = sorted(r["total_reads"] / r["map_seconds"] for r in mine)
            out[leg] = {"reads_per_s_median": statistics.median(v), "reads_per_s_min": v[0], "reads_per_s_max": v[-1], "stream_reads": mine[-1]["stream_reads"]}
            if leg == "stream":
                out[leg]["kernel_ms"] = {k: statistics.median(r[k + "_ms"] for r in mine) for k in ("parse", "materialise", "size", "format")}
        out["ratio_stream_over_host"] = out["stream"]["reads_per_s_median"] / out["host"]["reads_per_s_median"]
        return out
    doc = {"reads": 2 * a.pairs, "threads": a.threads, "runs_per_leg": a.runs, "files_identical": identical,
           "results": {"%s_%s" % (form, fmt): summary(form, fmt) for fmt in ("sam", "bam") for form in FORMS}, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
