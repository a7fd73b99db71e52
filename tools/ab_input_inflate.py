#!/usr/bin/env python3
"""bgzip-ped read files inflated on the device (-fz device) against the host's zlib threads (-fz host: what every run did before the flag),
alternating, one fresh process per run; and the inflate kernel alone on 256 MB of the same text.

  python tools/ab_input_inflate.py [--pairs 10000000] [--runs 3] [--threads 16] [--alone-mb 256] [--workdir DIR] [--out profiles/NAME.json] [--step-timeout 600] [--setup-timeout 900]

Reads: benchkit/reads.py (the bench's read model) on the E. coli-sized synthetic genome of bench.py, bgzip-ped by a writer of this tool's own
(Python's zlib on a thread pool, level 6, payloads of 0xff00 bytes, the EOF block at the end).  Every step that uses the GPU is a child process under
its own `timeout -k 10`, and this process never opens the device: the set-up (index and reads), then every run, one HostSession.map() (kh_stats_t: map_seconds, inflate_device_bytes / inflate_host_bytes / inflate_device_ms); the parent takes the
child's user + system CPU seconds from its resource usage and the sha256 of its SAM, which has to be the same in every run.  The kernel alone:
kg_bgzf_inflate on the members of the first --alone-mb MB of mate 1's text, in a child process under `rocprofv3 --kernel-trace --stats` (kernel time:
the trace's; the call's wall time includes its copies in and out).  A run that fails, aborts or meets its time limit ends the tool there.
Prints one JSON document."""
import argparse
import csv
import glob
import hashlib
import json
import os
import resource
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAYLOAD = 0xff00


def member(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(body) + 8 - 1)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def bgzip(src: str, dst: str, threads: int, keep_members_of: int = 0):
    """src -> dst as BGZF; returns the members that hold the first keep_members_of bytes of the text"""
    kept, kept_bytes = [], 0
    with open(src, "rb") as fi, open(dst, "wb") as fo, ThreadPoolExecutor(threads) as pool:
        while True:
            blob = fi.read(PAYLOAD * 64 * threads)
            if not blob:
                break
            for m, n in zip(pool.map(member, (blob[i:i + PAYLOAD] for i in range(0, len(blob), PAYLOAD))), range(0, len(blob), PAYLOAD)):
                fo.write(m)
                if kept_bytes < keep_members_of:
                    kept.append(m); kept_bytes += min(PAYLOAD, len(blob) - n)
        fo.write(member(b""))
    return b"".join(kept)


def child(a):
    from kart_amd import api
    sess = api.HostSession(a.prefix, 0, a.threads)
    st = sess.map(["-f", a.f1, "-f2", a.f2, "-o", a.output, "-fz", a.child])
    sess.close()
    d = st.as_dict()
    print(json.dumps({"leg": a.child, "total_reads": d["total_reads"], "stream_reads": d["stream_reads"], "map_seconds": d["map_seconds"],
                      "reads_per_s": d["total_reads"] / d["map_seconds"], "inflate_device_bytes": d["inflate_device_bytes"],
                      "inflate_host_bytes": d["inflate_host_bytes"], "inflate_device_ms": d["inflate_device_ms"], "sam_bytes": os.path.getsize(a.output)}))


def setup(a):
    """the E. coli-sized synthetic genome's index and the reads of the bench's model, on the device"""
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


def alone(a):
    """kg_bgzf_inflate on the members in a.output, twice: the second call is the one to read"""
    from kart_amd import api
    data = open(a.output, "rb").read()
    member_off, text_off = api.bgzf_members(data)
    walls, bad = [], 0
    for _ in range(2):
        t0 = time.perf_counter()
        text, _, status = api.bgzf_inflate(data, member_off, text_off)
        walls.append(time.perf_counter() - t0)
        bad += int((status != 0).sum())
    print(json.dumps({"member_bytes": len(data), "members": len(member_off) - 1, "text_bytes": len(text), "refused": bad, "call_seconds": walls}))


def sha256_of(path):
    h = hashlib.sha256()
    with open(path, "rb") as fi:
        for b in iter(lambda: fi.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--alone-mb", type=int, default=256)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--setup-timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    for k in ("prefix", "f1", "f2", "output"):
        ap.add_argument("--" + k, default=None)
    a = ap.parse_args()
    if a.child == "alone":
        return alone(a)
    if a.child == "setup":
        return setup(a)
    if a.child:
        return child(a)
    work = a.workdir or tempfile.mkdtemp(prefix="ab_fz_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, "ecoli_like")
    f1, f2 = os.path.join(work, "r_1.fq"), os.path.join(work, "r_2.fq")
    me = os.path.abspath(__file__)
    # index and reads are made on the device: a child step under a time limit like every other one (this process never opens the GPU)
    r = subprocess.run(["timeout", "-k", "10", str(a.setup_timeout), sys.executable, me, "--child", "setup", "--prefix", prefix, "--f1", f1, "--f2", f2,
                        "--pairs", str(a.pairs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.exit("the set-up step failed (%d): %s" % (r.returncode, r.stderr.decode()[-800:]))
    z1, z2, some = f1 + ".gz", f2 + ".gz", os.path.join(work, "members.bgzf")
    with open(some, "wb") as fh:
        fh.write(bgzip(f1, z1, a.threads, a.alone_mb << 20))
    bgzip(f2, z2, a.threads)
    text_bytes, packed_bytes = os.path.getsize(f1) + os.path.getsize(f2), os.path.getsize(z1) + os.path.getsize(z2)
    os.remove(f1); os.remove(f2)

    def run(leg):
        out = os.path.join(work, leg + ".sam")
        before = resource.getrusage(resource.RUSAGE_CHILDREN)
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--child", leg, "--prefix", prefix, "--f1", z1, "--f2", z2, "--output", out,
                            "--threads", str(a.threads)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        after = resource.getrusage(resource.RUSAGE_CHILDREN)
        if r.returncode != 0:
            sys.exit("the -fz %s run failed (%d): %s" % (leg, r.returncode, r.stderr.decode()[-800:]))
        line = json.loads(r.stdout.decode().strip().splitlines()[-1])
        # (the whole child: interpreter, index load and the run)
        line["cpu_seconds"] = (after.ru_utime - before.ru_utime) + (after.ru_stime - before.ru_stime)
        line["sam_sha256"] = sha256_of(out)
        return line

    runs = []
    for _ in range(a.runs):
        for leg in ("host", "device"):
            runs.append(run(leg))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)

    # the kernel alone, under the profiler (a run of its own: tracing slows the host)
    trace = os.path.join(work, "trace")
    r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--", sys.executable, me,
                        "--child", "alone", "--output", some], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.exit("the profiled kg_bgzf_inflate run failed (%d): %s" % (r.returncode, r.stderr.decode()[-800:]))
    solo = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    kernels = {}
    for path in glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "bgzf" in row["Name"]:
                kernels[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
    inflate = [v for k, v in kernels.items() if "bgzf_inflate_kernel" in k]
    if inflate:
        per_call_s = inflate[0]["total_ms"] / 1e3 / inflate[0]["calls"]
        solo["inflate_kernel_text_GB_per_s"] = solo["text_bytes"] / per_call_s / 1e9
    solo["kernels"] = kernels

    def leg_summary(leg):
        mine = [r for r in runs if r["leg"] == leg]
        v = sorted(r["reads_per_s"] for r in mine)
        return {"reads_per_s_median": statistics.median(v), "reads_per_s_min": v[0], "reads_per_s_max": v[-1],
                "map_seconds_median": statistics.median(r["map_seconds"] for r in mine), "cpu_seconds_median": statistics.median(r["cpu_seconds"] for r in mine),
                "inflate_device_ms_median": statistics.median(r["inflate_device_ms"] for r in mine),
                "inflate_device_bytes": mine[-1]["inflate_device_bytes"], "inflate_host_bytes": mine[-1]["inflate_host_bytes"]}
    host, device = leg_summary("host"), leg_summary("device")
    shas = sorted({r["sam_sha256"] for r in runs})
    doc = {"reads": 2 * a.pairs, "threads": a.threads, "runs_per_leg": a.runs, "text_bytes": text_bytes, "bgzf_bytes": packed_bytes,
           "base": "host (-fz host: the only way before the flag)", "host": host, "device": device,
           "ratio_device_over_host_reads_per_s": device["reads_per_s_median"] / host["reads_per_s_median"],
           "cpu_seconds_saved_per_run": host["cpu_seconds_median"] - device["cpu_seconds_median"], "sam_sha256": shas, "sam_equal_in_every_run": len(shas) == 1,
           "kernel_alone": solo, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if len(shas) != 1:
        sys.exit("the runs' SAM files differ")


if __name__ == "__main__":
    main()
