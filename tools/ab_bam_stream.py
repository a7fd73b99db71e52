#!/usr/bin/env python3
"""-bo through the device stream against -bo through the host's reader, printer and encoder (KART_AMD_NO_STREAM=1: the only -bo path before the
device made BAM records), alternating, one fresh process per run; and the BAM kernels against the SAM kernels on the same reads.

  python tools/ab_bam_stream.py [--pairs 10000000] [--runs 3] [--threads 16] [--workdir DIR] [--out profiles/NAME.json]

Reads: benchkit/reads.py (the bench's read model) on the E. coli-sized synthetic genome of bench.py.  Every run is one HostSession.map() in a
child process (kh_stats_t: map_seconds, stream_reads, kernel_ms[9] = size + scan, kernel_ms[10] = format, text_out_bytes); the two -bo files are
compared byte for byte.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    from kart_amd import api
    sess = api.HostSession(a.prefix, 0, a.threads)
    st = sess.map(["-f", a.f1, "-f2", a.f2, "-bo" if a.fmt == "bam" else "-o", a.output])
    sess.close()
    d = st.as_dict()
    print(json.dumps({"leg": a.child, "fmt": a.fmt, "total_reads": d["total_reads"], "stream_reads": d["stream_reads"], "map_seconds": d["map_seconds"],
                      "size_ms": d["kernel_ms"][9], "format_ms": d["kernel_ms"][10], "text_out_bytes": d["text_out_bytes"], "copy_ms": d["stage_ms"][5],
                      "file_bytes": os.path.getsize(a.output)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    for k in ("prefix", "f1", "f2", "output", "fmt"):
        ap.add_argument("--" + k, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    import torch
    import bench
    from benchkit.reads import write_fastq_pairs
    from kart_amd import index_build, synth
    work = a.workdir or tempfile.mkdtemp(prefix="ab_bam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(work, exist_ok=True)
    dev = torch.device("cuda:0")
    genome = bench.make_genome(seed=2, length=bench.GENOME_LEN)
    prefix = os.path.join(work, "ecoli_like")
    if not os.path.exists(prefix + ".bwt"):
        synth.write_fasta(prefix + ".fa", genome)
        index_build.build_index(prefix + ".fa", prefix, device=str(dev))
    codes = torch.from_numpy(np.concatenate([synth.encode(genome["decoy"]), synth.encode(genome["chrE"])])).to(dev)
    f1, f2 = os.path.join(work, "r_1.fq"), os.path.join(work, "r_2.fq")
    write_fastq_pairs(codes, a.pairs, 11, f1, f2, dev)
    del codes
    torch.cuda.empty_cache()

    def run(leg, fmt):
        out = os.path.join(work, "%s.%s" % (leg, fmt))
        env = dict(os.environ)
        if leg == "host":
            env["KART_AMD_NO_STREAM"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--fmt", fmt, "--prefix", prefix, "--f1", f1, "--f2", f2, "--output", out,
                            "--threads", str(a.threads)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
        if r.returncode != 0:
            sys.exit("the %s / %s run failed (%d): %s" % (leg, fmt, r.returncode, r.stderr.decode()[-800:]))
        return json.loads(r.stdout.decode().strip().splitlines()[-1])

    runs = []
    for _ in range(a.runs):
        for leg in ("host", "stream"):
            runs.append(run(leg, "bam"))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    same = subprocess.run(["cmp", os.path.join(work, "host.bam"), os.path.join(work, "stream.bam")]).returncode == 0
    sam = run("stream", "sam")
    print(json.dumps(sam), file=sys.stderr, flush=True)
    os.remove(os.path.join(work, "stream.sam"))

    def rate(leg):
        v = sorted(r["total_reads"] / r["map_seconds"] for r in runs if r["leg"] == leg)
        return {"reads_per_s_median": statistics.median(v), "reads_per_s_min": v[0], "reads_per_s_max": v[-1]}
    host, stream = rate("host"), rate("stream")
    bam = [r for r in runs if r["leg"] == "stream"][-1]
    doc = {"reads": 2 * a.pairs, "threads": a.threads, "runs_per_leg": a.runs, "host_path": host, "stream_path": stream,
           "ratio_stream_over_host": stream["reads_per_s_median"] / host["reads_per_s_median"], "files_identical": same,
           "bam_kernels_ms": {"size_scan": bam["size_ms"], "format": bam["format_ms"]}, "sam_kernels_ms": {"size_scan": sam["size_ms"], "format": sam["format_ms"]},
           "out_bytes_per_read": {"bam": bam["text_out_bytes"] / bam["total_reads"], "sam": sam["text_out_bytes"] / sam["total_reads"]},
           "copy_out_ms": {"bam": bam["copy_ms"], "sam": sam["copy_ms"]}, "stream_reads": {"bam": bam["stream_reads"], "sam": sam["stream_reads"]}, "runs": runs + [sam]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
