"""CPU: the device's BGZF member inflater (kart_amd/csrc/kernels/bgzf_inflate.inc) compiled as a host program (tests/bgzf_inflate_host.cpp, lane
after lane in the place of a wave) with AddressSanitizer and UBSan: every block shape zlib writes, the project's own deflater's members, a
hand-assembled 15-bit code, a mixed file -- and that file with one member damaged, where the status has to say what Python's zlib says.
Then GzText::fill_bgzf() with a MemberInflater in the place of the zlib threads (tests/bgzf_fill_host.cpp)."""
import os
import subprocess
import zlib

import pytest

import bgzf_inflate_cases as cases
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def program():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "bgzf_inflate_host")
    subprocess.check_call(["g++"] + SAN + ["-I", os.path.join(ROOT, "kart_amd", "csrc"), os.path.join(ROOT, "tests", "bgzf_inflate_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def deflater():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "bgzf_block_host_for_inflate")
    subprocess.check_call(["g++"] + SAN + ["-I", os.path.join(ROOT, "kart_amd", "csrc"), os.path.join(ROOT, "tests", "bgzf_block_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def mixed():
    return cases.mixed_file()


def run(program, tmp_path, data: bytes):
    """the program on a file: ([text piece per member], [status]); it has to exit 0 with nothing on stderr (the sanitizers' reports go there)"""
    src, dst = str(tmp_path / "in.gz"), str(tmp_path / "out")
    open(src, "wb").write(data)
    r = subprocess.run([program, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    status = [int(x) for x in r.stdout.split()]
    text, pieces, at = open(dst, "rb").read(), [], 0
    members = cases.split(data)
    assert len(status) == len(members)
    for m in members:
        n = cases.isize_of(m) if cases.isize_of(m) <= 65536 else 0
        pieces.append(text[at:at + n]); at += n
    assert at == len(text)
    return pieces, status


def test_sound_members_of_every_block_shape(program, tmp_path):
    sound = cases.sound_cases()
    for name, text, m in sound:
        assert cases.accepts(m) == (True, text), name               # (the hand-assembled 15-bit block among them: zlib reads it)
    text15, m15 = cases.fifteen_bit_member()
    d = zlib.decompressobj(-15)
    assert d.decompress(m15[18:-8]) == text15 and d.eof and d.unused_data == b"" and ("fifteen_bits", text15, m15) in sound
    pieces, status = run(program, tmp_path, b"".join(m for _, _, m in sound))
    for (name, text, _), piece, st in zip(sound, pieces, status):
        assert st == cases.OK and piece == text, name


def test_members_of_the_projects_own_deflater(program, deflater, tmp_path):
    from test_bgzf_block_cpu import inputs
    wanted = ("apart32768", "apart32769", "run65280", "pattern", "deep", "text")
    for name, data in inputs():
        if name not in wanted:
            continue
        src, packed = str(tmp_path / "plain"), str(tmp_path / "packed")
        open(src, "wb").write(data)
        subprocess.run([deflater, src, packed], check=True, timeout=120)
        pieces, status = run(program, tmp_path, open(packed, "rb").read())
        assert status == [cases.OK] * len(status) and b"".join(pieces) == data, name


def test_the_mixed_file(program, mixed, tmp_path):
    texts, members = mixed
    assert 250 <= len(members) <= 350 and texts[-1] == b"" and b"" in texts[1:-1]
    pieces, status = run(program, tmp_path, b"".join(members))
    assert status == [cases.OK] * len(members) and pieces == texts


def victim_of(texts):
    return max(range(len(texts) // 2 - 20, len(texts) // 2 - 1), key=lambda i: len(texts[i]))


def test_a_damaged_member_gets_the_status_zlib_gives_it(program, mixed, tmp_path):
    texts, members = mixed
    victim = victim_of(texts)
    lo, hi = 0, len(members)
    for name, bad in cases.damaged_cases(texts, members, victim):
        good, _ = cases.accepts(bad)
        assert not good, name                                   # (the seed of damaged_cases: every case is one zlib refuses)
        pieces, status = run(program, tmp_path, b"".join(members[lo:victim] + [bad] + members[victim + 1:hi]))
        at = victim - lo
        assert status[at] != cases.OK, name
        if name == "crc_bit":
            assert status[at] == cases.CRC
        assert status[:at] + status[at + 1:] == [cases.OK] * (hi - lo - 1), name
        assert pieces[:at] + pieces[at + 1:] == texts[lo:victim] + texts[victim + 1:hi], name


# ---- GzText::fill_bgzf() with an inflater in the place of the zlib threads (tests/bgzf_fill_host.cpp) -----------------------------
@pytest.fixture(scope="module")
def fill_program():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "bgzf_fill_host")
    subprocess.check_call(["g++"] + SAN + ["-fno-omit-frame-pointer", "-Wno-unused-result", "-Wno-unused-function", "-Wno-unused-variable",
                                           os.path.join(ROOT, "tests", "bgzf_fill_host.cpp"), "-o", exe, "-lz", "-lpthread"])
    return exe


def fill_files():
    """{name: (bytes of the file, the text of its sound BGZF members in front of anything else, or None)}"""
    import gzip
    import random
    from bgzf_util import EOF_BLOCK, bgzf
    rng = random.Random(17)
    text = cases.fastq(200000, 4) * 60
    sound = bgzf(text, block=12000, rng=rng)
    members = cases.split(sound)
    assert len(members) >= 2000
    k = len(members) // 2
    bad = bytearray(members[k])
    bad[len(bad) // 2] ^= 0x10
    assert not cases.accepts(bytes(bad))[0]
    return {
        "sound": (sound, text),
        "damaged": (b"".join(members[:k] + [bytes(bad)] + members[k + 1:]), None),
        "foreign": (b"".join(members[:-1]) + gzip.compress(text[:300000]), None),
        "truncated": (sound[:len(sound) // 2 + 7], None),
        "eof_alone": (EOF_BLOCK, b""),
    }


def fill_run(exe, tmp_path, name, data, mode):
    import json
    src, out = str(tmp_path / (name + ".gz")), str(tmp_path / (name + "." + mode))
    if not os.path.exists(src):
        open(src, "wb").write(data)
    r = subprocess.run([exe, src, out, mode, "4"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and r.stderr == b"", (name, mode, r.stderr.decode()[-2000:])
    return open(out + ".fill", "rb").read(), open(out + ".producer", "rb").read(), json.loads(r.stdout)


def test_fill_bgzf_hands_out_the_same_text_with_an_inflater(fill_program, tmp_path):
    for name, (data, text) in fill_files().items():
        plain_fill, plain_producer, plain = fill_run(fill_program, tmp_path, name, data, "none")
        assert plain_fill == plain_producer, name
        assert plain["fill_device_bytes"] == 0 and plain["producer_device_bytes"] == 0, name
        if text is not None:
            assert plain_fill == text and plain["fill_host_bytes"] == len(text), name
        emu_fill, emu_producer, emu = fill_run(fill_program, tmp_path, name, data, "emu")
        assert emu_fill == plain_fill and emu_producer == plain_fill, name
        # who inflated the BGZF members is all that differs: the same bytes of them, the device's where zlib's were
        assert (emu["fill_device_bytes"], emu["fill_host_bytes"]) == (plain["fill_host_bytes"], 0), name
        assert (emu["producer_device_bytes"], emu["producer_host_bytes"]) == (plain["producer_host_bytes"], 0), name
    assert len(plain_fill) == 0                                 # (the EOF block alone)


def test_zlib_finishes_the_file_when_the_inflater_gives_up(fill_program, tmp_path):
    data, text = fill_files()["sound"]
    fill, producer, n = fill_run(fill_program, tmp_path, "sound", data, "emu-fail2")
    assert fill == text and producer == text
    assert 0 < n["fill_device_bytes"] < len(text) and n["fill_device_bytes"] + n["fill_host_bytes"] == len(text)
    # (the producer asks for rounds of 64 MB: this file is one round, which the inflater's first run takes whole)
    assert n["producer_device_bytes"] + n["producer_host_bytes"] == len(text)
