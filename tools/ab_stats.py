#!/usr/bin/env python3
"""What -stats costs: the same FASTQ library mapped by a build of the parent commit, by this build without the flag, and by this build with it for
-o and for -bo; alternating, one fresh process per run.

  python tools/ab_stats.py [--pairs 10000000] [--runs 3] [--threads 16] [--parent-root DIR] [--workdir DIR] [--out profiles/NAME.json] [--step-timeout 600] [--setup-timeout 900]

Reads: benchkit/reads.py (the bench's read model) on the E. coli-sized synthetic genome of bench.py.  Every GPU step -- the set-up (index and reads)
and each run, one HostSession.map() -- is a child process under its own `timeout -k 10`; the first that fails ends the script, and the parent itself
never opens the device.  --parent-root: a directory that holds the kart_amd package of a build without the flag (its api.py and libraries); its leg
"parent" is the regression reference for the leg "plain" (this build, no flag): "plain" has to lie within the spread of "parent"'s runs, and both write
the same file.  The legs "bam_plain" / "bam_stats" are the -bo pair.  kh_stats_t gives map_seconds, stream_reads and the stream's stats_kernel_ms /
stats_kernel_launches / stats_bytes (the rows copied to the host).  Prints one JSON document."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("parent", "plain", "stats", "bam_plain", "bam_stats")


def child(a):
    sys.path.insert(0, a.root)
    from kart_amd import api
    with_stats = a.child in ("stats", "bam_stats")
    path = a.output + ".stats"
    sess = api.HostSession(a.prefix, 0, a.threads)
    st = sess.map(["-f", a.f1, "-f2", a.f2] + (["-stats", path] if with_stats else []) + ["-bo" if a.child.startswith("bam") else "-o", a.output])
    sess.close()
    d = st.as_dict()
    row = {"leg": a.child, "total_reads": d["total_reads"], "unmapped": d["unmapped"], "stream_reads": d["stream_reads"], "map_seconds": d["map_seconds"],
           "respeculated": d["respeculated"], "stats_kernel_ms": d.get("stats_kernel_ms", 0), "stats_kernel_launches": d.get("stats_kernel_launches", 0),
           "stats_row_bytes": d.get("stats_bytes", 0), "file_bytes": os.path.getsize(a.output),
           "stats_file_sha256": hashlib.sha256(open(path, "rb").read()).hexdigest() if with_stats else None}
    if with_stats:
        row["stats_file_head"] = open(path).read().split("\n")[1:7]
        os.remove(path)
    print(json.dumps(row))


def setup(a):
    """the index and the FASTQ files (the tool's only other GPU step: a child of its own, so that the parent never opens the device)"""
    sys.path.insert(0, ROOT)
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


def sha256_of(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--setup-timeout", type=int, default=900)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    for k in ("prefix", "f1", "f2", "output", "root"):
        ap.add_argument("--" + k, default=None)
    a = ap.parse_args()
    if a.child:
        return setup(a) if a.child == "setup" else child(a)
    work = a.workdir or tempfile.mkdtemp(prefix="ab_stats_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, "ecoli_like")
    f1, f2 = os.path.join(work, "r_1.fq"), os.path.join(work, "r_2.fq")

    def step(seconds, args):
        """one GPU step: a child process under its own time limit; a failure ends the script"""
        r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            sys.exit("step %s failed (%d): %s" % (" ".join(args[:4]), r.returncode, r.stderr.decode()[-800:]))
        return r.stdout.decode()

    step(a.setup_timeout, ["--child", "setup", "--prefix", prefix, "--f1", f1, "--f2", f2, "--pairs", str(a.pairs)])
    legs = [leg for leg in LEGS if leg != "parent" or a.parent_root]
    runs, sha = [], {}
    for k in range(a.runs):
        for leg in legs:
            out = os.path.join(work, "out_" + leg)
            root = os.path.abspath(a.parent_root) if leg == "parent" else ROOT
            text = step(a.step_timeout, ["--child", leg, "--root", root, "--prefix", prefix, "--f1", f1, "--f2", f2, "--output", out, "--threads", str(a.threads)])
            runs.append(json.loads(text.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
            if k == 0:
                sha[leg] = sha256_of(out)
            os.remove(out)

    def summary(leg):
        mine = [r for r in runs if r["leg"] == leg]
        v = sorted(r["total_reads"] / r["map_seconds"] for r in mine)
        s = sorted(r["map_seconds"] for r in mine)
        return {"reads_per_s_median": statistics.median(v), "reads_per_s_min": v[0], "reads_per_s_max": v[-1],
                "map_seconds_median": statistics.median(s), "map_seconds_min": s[0], "map_seconds_max": s[-1], "stream_reads": mine[-1]["stream_reads"],
                "stats_kernel_ms_median": statistics.median(r["stats_kernel_ms"] for r in mine), "stats_kernel_launches": mine[-1]["stats_kernel_launches"],
                "stats_row_bytes": mine[-1]["stats_row_bytes"], "file_bytes": mine[-1]["file_bytes"]}
    doc = {"reads": 2 * a.pairs, "threads": a.threads, "runs_per_leg": a.runs, "results": {leg: summary(leg) for leg in legs}, "runs": runs}
    doc["stats_main_file_equals_plain_file"] = sha["stats"] == sha["plain"]
    doc["bam_stats_main_file_equals_bam_plain_file"] = sha["bam_stats"] == sha["bam_plain"]
    doc["one_stats_file_in_all_runs"] = len({r["stats_file_sha256"] for r in runs if r["stats_file_sha256"]}) == 1
    for with_flag, without in (("stats", "plain"), ("bam_stats", "bam_plain")):
        doc[with_flag + "_costs_seconds_median"] = doc["results"][with_flag]["map_seconds_median"] - doc["results"][without]["map_seconds_median"]
    if "parent" in sha:
        doc["plain_file_equals_parent_file"] = sha["parent"] == sha["plain"]
        p, q = doc["results"]["parent"], doc["results"]["plain"]
        # (the regression check: no slower than the slowest of the parent's runs; faster than its fastest is no regression either)
        doc["plain_median_not_below_parent_min"] = q["reads_per_s_median"] >= p["reads_per_s_min"]
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
