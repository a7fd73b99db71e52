"""CPU: the Writer releases each output window once every byte of it is in the file (kart_amd/csrc/host/detail/writer.inc: complete(),
unmap_loop()).  With the window knob at 1-4 MB (KART_AMD_OUT_WINDOW_MB) small outputs cross many windows, and every place the Writer
is used must still write the same bytes: the golden SAMs at -t 2 / 8, three shards taking turns at one file, -parts, the pwrite-only
and kept-window writer modes; a seeded set of ~30 MB of SAM (dozens of 1 MB windows) against the same run with the default 1 GB
window.  The host pipeline is bound to the CPU oracle backend (tests/cpu_backend)."""
import gzip
import os
import subprocess
import sys

import pytest

import ref_runs
from conftest import GOLDEN, ROOT, SMALL_PREFIX
from test_host_pipeline import materialise, run_case_env
from test_sharded_cpu import moving_estimate_input  # noqa: F401  (the fixture)


@pytest.fixture(scope="module")
def host_oracle_binary():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_backend")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "_build", "kart-host-oracle")


@pytest.fixture(scope="module")
def seeded_pairs(tmp_path_factory):
    """36 k read pairs on the small genome: ~30 MB of SAM"""
    from kart_amd import synth
    from kart_amd.index_build import read_fasta
    tmp = tmp_path_factory.mktemp("windows")
    genome = {n: s for n, _, s in read_fasta(os.path.join(GOLDEN, "small.fa"))}
    names, r1, r2 = synth.simulate_pairs(genome, 36000, seed=77, err=0.02, mut=0.003, indel_frac=0.3)
    f1, f2 = str(tmp / "w_1.fq"), str(tmp / "w_2.fq")
    synth.write_fastq(f1, names, r1, mate=1)
    synth.write_fastq(f2, names, r2, mate=2)
    return f1, f2


def run(binary, args, out, env, extra=()):
    r = subprocess.run([binary, "-silent", "-i", SMALL_PREFIX] + args + list(extra) + ["-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, **env), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-800:]
    return r.stdout.decode()


def read_parts(out, n):
    return b"".join(open("%s.%d" % (out, r), "rb").read() for r in range(n))


@pytest.mark.parametrize("case", ["pe", "se", "pe_m"])
@pytest.mark.parametrize("threads", [2, 8])
@pytest.mark.parametrize("window_mb", [1, 4])
def test_small_windows_match_golden(case, threads, window_mb, host_oracle_binary, tmp_path):
    got, want, _ = run_case_env(host_oracle_binary, case, str(tmp_path), ["-t", str(threads)], {"KART_AMD_OUT_WINDOW_MB": str(window_mb)})
    assert got == want


@pytest.mark.parametrize("env", [{"KART_AMD_WRITER_MODE": "0"}, {"KART_AMD_WRITER_MODE": "2"}, {"KART_AMD_WRITER_MODE": "3"},
                                 {"KART_AMD_PREALLOC": "1"}, {"KART_AMD_PWRITE_THREADS": "3"}, {"KART_AMD_UNMAP_CPUS": "lanes"}])
def test_small_windows_writer_variants_match_golden(env, host_oracle_binary, tmp_path):
    got, want, _ = run_case_env(host_oracle_binary, "pe", str(tmp_path), ["-t", "8"], dict(env, KART_AMD_OUT_WINDOW_MB="1"))
    assert got == want


def test_small_windows_three_shards_one_file_match_golden(host_oracle_binary, tmp_path):
    """three shard processes take turns at one file: each one's text starts and ends inside a window another shard also writes"""
    got, want, _ = run_case_env(host_oracle_binary, "pe", str(tmp_path), ["-gpu", "0,1,2", "-t", "6"], {"KART_AMD_OUT_WINDOW_MB": "1"})
    assert got == want


def test_small_windows_parts_match_golden(host_oracle_binary, tmp_path):
    f1, f2 = materialise(str(tmp_path), "pe_1.fq.gz"), materialise(str(tmp_path), "pe_2.fq.gz")
    out = str(tmp_path / "o.sam")
    run(host_oracle_binary, ["-f", f1, "-f2", f2], out, {"KART_AMD_OUT_WINDOW_MB": "1"}, ["-gpu", "0,1,2", "-parts", "-t", "6"])
    assert read_parts(out, 3) == gzip.open(os.path.join(GOLDEN, "sam", "pe.sam.gz")).read()


@pytest.fixture(scope="module")
def seeded_default(seeded_pairs, host_oracle_binary, tmp_path_factory):
    """the seeded set through the default 1 GB window: the bytes every small-window run must reproduce"""
    out = str(tmp_path_factory.mktemp("windows_default") / "d.sam")
    run(host_oracle_binary, ["-f", seeded_pairs[0], "-f2", seeded_pairs[1]], out, {}, ["-t", "8"])
    data = open(out, "rb").read()
    assert len(data) > 24 << 20
    return data


@pytest.mark.parametrize("threads", [2, 8])
def test_dozens_of_windows_same_bytes(threads, seeded_pairs, seeded_default, host_oracle_binary, tmp_path):
    out = str(tmp_path / "o.sam")
    log = run(host_oracle_binary, ["-f", seeded_pairs[0], "-f2", seeded_pairs[1]], out, {"KART_AMD_OUT_WINDOW_MB": "1", "KART_AMD_VERBOSE": "1"}, ["-t", str(threads)])
    assert open(out, "rb").read() == seeded_default
    # all but the last window or two were unmapped while the run went on
    beside = int(log.split("unmapped during the run: ")[1].split(" windows")[0])
    assert beside >= len(seeded_default) // (1 << 20) - 2, log[-600:]


def test_dozens_of_windows_three_shards_one_file(seeded_pairs, seeded_default, host_oracle_binary, tmp_path):
    out = str(tmp_path / "o.sam")
    run(host_oracle_binary, ["-f", seeded_pairs[0], "-f2", seeded_pairs[1]], out, {"KART_AMD_OUT_WINDOW_MB": "1"}, ["-gpu", "0,1,2", "-t", "6"])
    assert open(out, "rb").read() == seeded_default


def test_dozens_of_windows_parts(seeded_pairs, seeded_default, host_oracle_binary, tmp_path):
    out = str(tmp_path / "o.sam")
    run(host_oracle_binary, ["-f", seeded_pairs[0], "-f2", seeded_pairs[1]], out, {"KART_AMD_OUT_WINDOW_MB": "2"}, ["-gpu", "0,1,2", "-parts", "-t", "6"])
    assert read_parts(out, 3) == seeded_default


def test_small_windows_parts_rewritten_tail(moving_estimate_input, host_oracle_binary, tmp_path):  # noqa: F811
    """-parts whose later shards write their text while mapping and, when settling changed a chunk, cut the part and write its tail
    again through a new Writer that starts inside a window"""
    f1, f2, ref = moving_estimate_input
    out = str(tmp_path / "o.sam")
    log = run(host_oracle_binary, ["-f", f1, "-f2", f2], out, {"KART_AMD_OUT_WINDOW_MB": "1", "KART_AMD_VERBOSE": "1"}, ["-gpu", "0,1,2,3", "-parts", "-t", "8"])
    assert ref_runs.of(read_parts(out, 4)) == ref
    rewritten = sum(int(l.split("chunks mapped again, ")[1].split()[0]) for l in log.splitlines() if l.startswith("shard ") and "chunks of text written again" in l)
    assert rewritten > 0, "the drifting estimate should have changed at least one chunk of a later shard"


def test_small_windows_under_thread_sanitizer():
    """tools/tsan_host.py's short form with 1 MB windows: the writers, the unmapping thread and the shards' turns -- no report"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tsan_host.py"), "--pairs", "12000", "--only", "14"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, KART_AMD_OUT_WINDOW_MB="1"), timeout=1500)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "14 runs, 0 reports or differences" in out, out[-1500:]
