"""CPU: the -bz flag of the command line (kart_amd/csrc/host/cli.cpp): listed in the usage, refused with anything but host / device, and
accepted in front of the run -- which, without a device, ends at the index load as every run does."""
import os
import subprocess

from conftest import GOLDEN, ROOT, SMALL_PREFIX

KART_AMD = os.path.join(ROOT, "kart_amd", "bin", "kart-amd")


def run(args):
    r = subprocess.run([KART_AMD] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    return r.returncode, r.stdout.decode()


def test_usage_lists_bz(built_lib):
    rc, out = run(["-h"])
    assert rc == 0
    line = [l for l in out.splitlines() if l.strip().startswith("-bz")]
    assert len(line) == 1 and "host" in line[0] and "device" in line[0], out


def test_bz_takes_host_or_device_only(built_lib):
    unknown_rc, unknown_out = run(["-no-such-flag"])
    assert "Unknown parameter" in unknown_out
    for args in (["-bz", "zstd"], ["-bz"], ["-i", SMALL_PREFIX, "-bz", "zstd", "-f", os.path.join(GOLDEN, "sam", "pe_1.fq.gz")]):
        rc, out = run(args)
        assert rc == unknown_rc != 0, out
        lines = out.splitlines()
        assert lines[0] == "Error! -bz expects host or device", out
        assert "Unknown parameter" not in out and any(l.startswith("Usage:") for l in lines[1:]), out


def test_bz_device_and_host_get_past_the_arguments(built_lib, tmp_path):
    from kart_amd import api
    if api.device_count() > 0:
        return                                           # (with a device the run itself is tests/test_bgzf_gpu.py's business)
    for how in ("device", "host"):
        rc, out = run(["-bz", how, "-i", SMALL_PREFIX, "-f", os.path.join(GOLDEN, "sam", "pe_1.fq.gz"), "-bo", str(tmp_path / "x.bam")])
        assert rc != 0 and "no HIP device" in out, out
        assert "Unknown parameter" not in out and "-bz expects" not in out and "Usage:" not in out, out
