#!/usr/bin/env python3
"""Where the writer's drain goes at product scale (MEASUREMENT TOOL, GPU box): the hg38-sized index of bench.py (built or found in its
work directory), N read pairs after bench.py's read model written once, then one HostSession maps them into a fresh SAM file in the
same directory several times with KART_AMD_VERBOSE, alternating between writer configurations in rounds:

    kept        KART_AMD_WRITER_MODE=3: every output window stays mapped until Writer::finish() (the form before windows were released)
    io          windows unmapped once written, the unmapping thread on the writers' CPUs (KART_AMD_UNMAP_CPUS=io, the default)
    lanes       ... the unmapping thread on the lane threads' CPUs (KART_AMD_UNMAP_CPUS=lanes)
    w256        ... 256 MB windows instead of 1024 (KART_AMD_OUT_WINDOW_MB=256)

For every run: the mapping's wall time and the parts of the writer drain from the "stage seconds" line (queue running dry, the
windows unmapped inside finish(), the exact-size ftruncate, and the windows unmapped during the run); the medians per configuration
at the end.

    python tools/probe_writer_tail.py [--pairs 20000000] [--rounds 3] [--configs kept,io,lanes,w256]"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "kept": {"KART_AMD_WRITER_MODE": "3"},
    "io": {"KART_AMD_UNMAP_CPUS": "io"},
    "lanes": {"KART_AMD_UNMAP_CPUS": "lanes"},
    "w256": {"KART_AMD_OUT_WINDOW_MB": "256"},
}
KNOBS = ("KART_AMD_WRITER_MODE", "KART_AMD_UNMAP_CPUS", "KART_AMD_OUT_WINDOW_MB")
DRAIN = re.compile(r"writer drain ([0-9.]+) \(queue running dry ([0-9.]+), unmapping (\d+) windows ([0-9.]+), exact size ([0-9.]+); "
                   r"unmapped during the run: (\d+) windows in ([0-9.]+)\)")


def map_once(sess, f1, f2, out):
    """one mapping run with the library's stdout (the verbose lines) captured"""
    import ctypes
    libc = ctypes.CDLL(None)
    sys.stdout.flush()
    libc.fflush(None)
    with tempfile.TemporaryFile() as cap:
        saved = os.dup(1)
        os.dup2(cap.fileno(), 1)
        try:
            t0 = time.time()
            st = sess.map(["-silent", "-f", f1, "-f2", f2, "-o", out])
            wall = time.time() - t0
        finally:
            libc.fflush(None)
            os.dup2(saved, 1)
            os.close(saved)
        cap.seek(0)
        text = cap.read().decode(errors="replace")
    return st, wall, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="kept,io,lanes,w256")
    ap.add_argument("--threads", type=int, default=None)
    args = ap.parse_args()
    import torch
    import bench
    from kart_amd import api
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import __graft_entry__ as entry
    entry.build()
    ix_args = argparse.Namespace(genome_len=bench.HG38_LEN, bucketed=None, repeat_frac=0.45, sa="auto")
    workdir = bench.pick_workdir(2 * args.pairs * bench.REC_BYTES + 2 * args.pairs * 450 + (12 << 30))
    os.makedirs(workdir, exist_ok=True)
    prefix, codes, t_build = bench.prepare_index(ix_args, dev, 0, workdir, lambda: None)
    f1, f2 = os.path.join(workdir, "probe_tail_1.fq"), os.path.join(workdir, "probe_tail_2.fq")
    out = os.path.join(workdir, "probe_tail_out.sam")
    t0 = time.time()
    bench.write_fastq_pairs(codes, args.pairs, 5, f1, f2, dev, err=0.01)
    bench.release_haplotypes()
    del codes
    torch.cuda.empty_cache()
    print("index %.1f s, %d read pairs written in %.1f s (%s)" % (t_build, args.pairs, time.time() - t0, workdir), flush=True)
    bench.resolved_sa(ix_args, dev)
    threads = args.threads or max(2, bench.effective_cores())
    sess = api.HostSession(prefix, 0, threads)
    names = args.configs.split(",")
    rows = {n: [] for n in names}
    try:
        map_once(sess, f1, f2, out)                       # (warm-up: the lanes' buffers, the first fresh file)
        os.remove(out)
        for rnd in range(args.rounds):
            for name in names:
                for k in KNOBS:
                    os.environ.pop(k, None)
                os.environ.update(CONFIGS[name])
                os.environ["KART_AMD_VERBOSE"] = "1"
                st, wall, text = map_once(sess, f1, f2, out)
                size = os.path.getsize(out)
                os.remove(out)                            # (outside the timed call, as bench.py does between its steps)
                m = DRAIN.search(text)
                if not m or st.total_reads != 2 * args.pairs:
                    print("round %d %-6s: unexpected run (%d reads)\n%s" % (rnd, name, st.total_reads, text[-3000:]), flush=True)
                    return 1
                drain, wait, n_end, unmap, trunc, n_beside, beside = (float(x) for x in m.groups())
                rows[name].append((wall, drain, wait, unmap, trunc, beside))
                print("round %d %-6s: wall %.3f s | SAM %.2f GB | writer drain %.3f = queue %.3f + unmap %.3f (%d windows) + ftruncate %.3f | "
                      "unmapped during the run: %d windows in %.3f s" % (rnd, name, wall, size / 1e9, drain, wait, unmap, n_end, trunc, n_beside, beside), flush=True)
                for line in text.splitlines():
                    if line.startswith(("stage seconds", "cpu seconds")):
                        print("    " + line.strip(), flush=True)
    finally:
        for k in KNOBS + ("KART_AMD_VERBOSE",):
            os.environ.pop(k, None)
        sess.close()
        for f in (f1, f2, out):
            if os.path.exists(f):
                os.remove(f)
    print("medians over %d rounds, %d M reads per run (s): wall | drain | queue | unmap in finish() | ftruncate | unmapped during the run" % (args.rounds, 2 * args.pairs // 1_000_000))
    for name in names:
        med = [statistics.median(col) for col in zip(*rows[name])]
        print("  %-6s %s" % (name, " | ".join("%.3f" % v for v in med)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
