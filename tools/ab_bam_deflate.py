#!/usr/bin/env python3
"""-bo with the BGZF blocks compressed on the device (-bz device) against -bo with the host's zlib (-bz host: what every -bo run did before the
flag), alternating, one fresh process per run; and the deflate kernels alone on 256 MB of the run's BAM records.

  python tools/ab_bam_deflate.py [--pairs 10000000] [--runs 3] [--threads 16] [--alone-mb 256] [--workdir DIR] [--out profiles/NAME.json]

Reads: benchkit/reads.py (the bench's read model) on the E. coli-sized synthetic genome of bench.py.  Every run is one HostSession.map() in a child
process (kh_stats_t: map_seconds, kernel_ms[15] = the BGZF blocks' plan + deflate + pack, bgzf_device_bytes / bgzf_host_bytes); the inflated
streams of the two files are compared by their sha256.  The kernels alone: kg_bgzf_deflate on the first --alone-mb MB of the inflated file, in a
child process under `rocprofv3 --kernel-trace --stats` (kernel time: the trace's; the call's wall time includes its copies in and out).
Prints one JSON document."""
import argparse
import csv
import glob
import gzip
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    from kart_amd import api
    sess = api.HostSession(a.prefix, 0, a.threads)
    st = sess.map(["-f", a.f1, "-f2", a.f2, "-bo", a.output, "-bz", a.child])
    sess.close()
    d = st.as_dict()
    print(json.dumps({"leg": a.child, "total_reads": d["total_reads"], "stream_reads": d["stream_reads"], "map_seconds": d["map_seconds"],
                      "reads_per_s": d["total_reads"] / d["map_seconds"], "bgzf_kernels_ms": d["kernel_ms"][15], "bgzf_launches": d["kernel_launches"][15],
                      "format_stage_ms": d["stage_ms"][4], "copy_ms": d["stage_ms"][5], "records_bytes": d["text_out_bytes"],
                      "bgzf_device_bytes": d["bgzf_device_bytes"], "bgzf_host_bytes": d["bgzf_host_bytes"], "file_bytes": os.path.getsize(a.output)}))


def alone(a):
    """kg_bgzf_deflate on the records in a.output (raw bytes), twice: the second call is the one to read"""
    from kart_amd import api
    raw = open(a.output, "rb").read()
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        bgzf, block_src, _ = api.bgzf_deflate(raw)
        walls.append(time.perf_counter() - t0)
    print(json.dumps({"input_bytes": len(raw), "blocks": len(block_src) - 1, "bgzf_bytes": len(bgzf), "call_seconds": walls}))


def inflated_sha256(path, keep=None, keep_bytes=0):
    h = hashlib.sha256()
    kept = 0
    with gzip.open(path, "rb") as fi, (open(keep, "wb") if keep else open(os.devnull, "wb")) as fo:
        while True:
            b = fi.read(1 << 24)
            if not b:
                break
            h.update(b)
            if kept < keep_bytes:
                fo.write(b[:keep_bytes - kept])
                kept += min(len(b), keep_bytes - kept)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--alone-mb", type=int, default=256)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    for k in ("prefix", "f1", "f2", "output"):
        ap.add_argument("--" + k, default=None)
    a = ap.parse_args()
    if a.child == "alone":
        return alone(a)
    if a.child:
        return child(a)
    import numpy as np
    import torch
    import bench
    from benchkit.reads import write_fastq_pairs
    from kart_amd import index_build, synth
    work = a.workdir or tempfile.mkdtemp(prefix="ab_bz_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
    me = os.path.abspath(__file__)

    def run(leg):
        out = os.path.join(work, leg + ".bam")
        r = subprocess.run([sys.executable, me, "--child", leg, "--prefix", prefix, "--f1", f1, "--f2", f2, "--output", out, "--threads", str(a.threads)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        if r.returncode != 0:
            sys.exit("the -bz %s run failed (%d): %s" % (leg, r.returncode, r.stderr.decode()[-800:]))
        return json.loads(r.stdout.decode().strip().splitlines()[-1])

    runs = []
    for _ in range(a.runs):
        for leg in ("host", "device"):
            runs.append(run(leg))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    records = os.path.join(work, "records.raw")
    sha = {"host": inflated_sha256(os.path.join(work, "host.bam")), "device": inflated_sha256(os.path.join(work, "device.bam"), records, a.alone_mb << 20)}

    # the kernels alone, under the profiler (a run of its own: tracing slows the host)
    trace = os.path.join(work, "trace")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--", sys.executable, me, "--child", "alone", "--output", records],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    if r.returncode != 0:
        sys.exit("the profiled kg_bgzf_deflate run failed (%d): %s" % (r.returncode, r.stderr.decode()[-800:]))
    solo = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    kernels = {}
    for path in glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "bgzf" in row["Name"]:
                kernels[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
    deflate = [v for k, v in kernels.items() if "bgzf_deflate_kernel" in k]
    if deflate:
        per_call_s = deflate[0]["total_ms"] / 1e3 / deflate[0]["calls"]
        solo["deflate_kernel_input_GB_per_s"] = solo["input_bytes"] / per_call_s / 1e9
    solo["kernels"] = kernels
    solo["ratio_bgzf_over_input"] = solo["bgzf_bytes"] / solo["input_bytes"]

    def leg_summary(leg):
        mine = [r for r in runs if r["leg"] == leg]
        v = sorted(r["reads_per_s"] for r in mine)
        return {"reads_per_s_median": statistics.median(v), "reads_per_s_min": v[0], "reads_per_s_max": v[-1],
                "map_seconds_median": statistics.median(r["map_seconds"] for r in mine), "file_bytes": mine[-1]["file_bytes"],
                "bgzf_kernels_ms_median": statistics.median(r["bgzf_kernels_ms"] for r in mine),
                "bgzf_device_bytes": mine[-1]["bgzf_device_bytes"], "bgzf_host_bytes": mine[-1]["bgzf_host_bytes"]}
    host, device = leg_summary("host"), leg_summary("device")
    doc = {"reads": 2 * a.pairs, "threads": a.threads, "runs_per_leg": a.runs, "base": "host (-bz host: the only -bo path before the flag)",
           "host": host, "device": device, "ratio_device_over_host_reads_per_s": device["reads_per_s_median"] / host["reads_per_s_median"],
           "file_size_ratio_device_over_host": device["file_bytes"] / host["file_bytes"], "inflated_sha256": sha, "inflated_streams_equal": sha["host"] == sha["device"],
           "kernels_alone": solo, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
