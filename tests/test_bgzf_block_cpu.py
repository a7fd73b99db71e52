"""CPU: the device's BGZF block deflater (kart_amd/csrc/kernels/bgzf_block.inc) compiled as a host program (tests/bgzf_block_host.cpp, thread after
thread in the place of a workgroup) with AddressSanitizer and UBSan, on the inputs at which its paths change; the members are read by zlib."""
import os
import random
import struct
import subprocess
import zlib

import pytest

from conftest import ROOT

PAYLOAD = 0xff00
HEAD = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0]) + b"BC" + bytes([2, 0])


@pytest.fixture(scope="module")
def program():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "bgzf_block_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kart_amd", "csrc"), os.path.join(ROOT, "tests", "bgzf_block_host.cpp"), "-o", exe])
    return exe


def inflate(data: bytes):
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 16] == HEAD
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        d = zlib.decompressobj(-15)
        raw = d.decompress(data[at + 18:at + size - 8])
        assert d.eof and d.unused_data == b""
        assert struct.unpack_from("<II", data, at + size - 8) == (zlib.crc32(raw), len(raw))
        out.append((raw, size))
        at += size
    return out


def inputs():
    rng = random.Random(3)
    fib = [1, 2]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    deep = [k + 1 for k, f in enumerate(fib) for _ in range(f)]
    rng.shuffle(deep)
    same = rng.randbytes(300)
    text = open(os.path.join(ROOT, "DESIGN.md"), "rb").read()
    yield "deep", bytes(deep)
    yield "text", text[:3 * PAYLOAD + 11]
    yield "range200", bytes(range(200))
    yield "random", rng.randbytes(PAYLOAD)
    yield "pattern", rng.randbytes(40) * 300
    yield "apart32768", same + rng.randbytes(32768 - 300) + same
    yield "apart32769", same + rng.randbytes(32769 - 300) + same
    for n in (1, 2, 3, 4, 255, 256, 257, 258, 259, 260, 511, 512, 513, PAYLOAD - 1, PAYLOAD, PAYLOAD + 1):
        yield "run%d" % n, b"z" * n
        yield "text%d" % n, text[1000:1000 + n]


def test_members_of_the_host_build_inflate_to_the_input(program, tmp_path):
    sizes = {}
    for name, data in inputs():
        src, dst = str(tmp_path / "in"), str(tmp_path / "out")
        open(src, "wb").write(data)
        subprocess.run([program, src, dst], check=True, timeout=120)
        members = inflate(open(dst, "rb").read())
        assert b"".join(raw for raw, _ in members) == data, name
        assert [len(raw) for raw, _ in members] == [min(PAYLOAD, len(data) - at) for at in range(0, len(data), PAYLOAD)], name
        assert all(size <= len(raw) + 31 for raw, size in members), name        # never larger than the stored member
        sizes[name] = sum(size for _, size in members)
    assert sizes["random"] == PAYLOAD + 31 and sizes["apart32769"] == 32769 + 300 + 31 and sizes["apart32768"] < 32768 + 300 + 31
    assert sizes["run%d" % PAYLOAD] < 400 and sizes["pattern"] < 600
    assert sizes["text"] < (3 * PAYLOAD + 11) * 0.6
