"""CPU: the -fz flag of the command line (kart_amd/csrc/host/cli.cpp): listed in the usage, refused with anything but host / device, and
accepted in front of the run -- which, without a device, ends at the index load as every run does.  A backend without an inflater (the CPU
oracle's) ignores the flag silently: bgzip-ped reads give the golden SAM with it."""
import gzip
import os
import random
import subprocess

import pytest

from conftest import GOLDEN, ROOT, SMALL_PREFIX

KART_AMD = os.path.join(ROOT, "kart_amd", "bin", "kart-amd")
SAM = os.path.join(GOLDEN, "sam")


def run(args):
    r = subprocess.run([KART_AMD] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    return r.returncode, r.stdout.decode()


def test_usage_lists_fz(built_lib):
    rc, out = run(["-h"])
    assert rc == 0
    line = [l for l in out.splitlines() if l.strip().startswith("-fz")]
    assert len(line) == 1 and line[0].strip() == "-fz STR       with bgzip-ped read files: who inflates them, host (zlib) or device [host]", out


def test_fz_takes_host_or_device_only(built_lib):
    unknown_rc, unknown_out = run(["-no-such-flag"])
    assert "Unknown parameter" in unknown_out
    for args in (["-fz", "gpu"], ["-fz"], ["-i", SMALL_PREFIX, "-fz", "zlib", "-f", os.path.join(SAM, "pe_1.fq.gz")]):
        rc, out = run(args)
        assert rc == unknown_rc != 0, out
        lines = out.splitlines()
        assert lines[0] == "Error! -fz expects host or device", out
        assert "Unknown parameter" not in out and any(l.startswith("Usage:") for l in lines[1:]), out


def test_fz_device_and_host_get_past_the_arguments(built_lib, tmp_path):
    from kart_amd import api
    if api.device_count() > 0:
        return                                           # (with a device the run itself is tests/test_bgzf_inflate_gpu.py's business)
    for how in ("device", "host"):
        rc, out = run(["-fz", how, "-i", SMALL_PREFIX, "-f", os.path.join(SAM, "pe_1.fq.gz"), "-o", str(tmp_path / "x.sam")])
        assert rc != 0 and "no HIP device" in out, out
        assert "Unknown parameter" not in out and "-fz expects" not in out and "Usage:" not in out, out


@pytest.fixture(scope="module")
def host_oracle_binary():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpu_backend")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "_build", "kart-host-oracle")


def test_a_backend_without_an_inflater_ignores_fz_device(host_oracle_binary, tmp_path):
    from bgzf_util import bgzf
    rng = random.Random(4)
    files = []
    for m, block in ((1, 0xff00), (2, 3000)):
        raw = gzip.open(os.path.join(SAM, "pe_%d.fq.gz" % m)).read()
        path = str(tmp_path / ("b%d.fq.gz" % m))
        open(path, "wb").write(bgzf(raw, block, rng if m == 2 else None))
        files.append(path)
    want = gzip.open(os.path.join(SAM, "pe.sam.gz")).read()
    for how in ("device", "host"):
        out = str(tmp_path / (how + ".sam"))
        r = subprocess.run([host_oracle_binary, "-i", SMALL_PREFIX, "-fz", how, "-f", files[0], "-f2", files[1], "-t", "4", "-o", out],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0 and r.stderr == b"", (r.stdout + r.stderr).decode()[-600:]
        assert open(out, "rb").read() == want, how
