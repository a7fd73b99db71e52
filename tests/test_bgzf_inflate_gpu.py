"""GPU: BGZF members inflated on the device (kernels/bgzf_inflate.inc behind kg_bgzf_inflate / kg_inflater_*), and -fz device through the product.
The members are those of tests/test_bgzf_inflate_cpu.py, which runs the same decoder on them under the sanitizers first: nothing goes to the device
that has not been through it there."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf_inflate_cases as cases
from conftest import GOLDEN, ROOT, SMALL_PREFIX

pytestmark = pytest.mark.gpu
KART_AMD = os.path.join(ROOT, "kart_amd", "bin", "kart-amd")
SAM = os.path.join(GOLDEN, "sam")


@pytest.fixture(scope="module")
def mixed():
    return cases.mixed_file()


def victim_of(texts):
    return max(range(len(texts) // 2 - 20, len(texts) // 2 - 1), key=lambda i: len(texts[i]))


# ---- the decoder alone ------------------------------------------------------------------------------------------------------------
def test_every_sound_member_and_the_mixed_file_in_one_call(built_lib, mixed):
    from kart_amd import api
    sound = cases.sound_cases()
    texts, members = mixed
    want = [t for _, t, _ in sound] + texts
    data = b"".join([m for _, _, m in sound] + members)
    text, text_off, status = api.bgzf_inflate(data)
    assert len(status) == len(want) and not status.any(), np.flatnonzero(status)
    assert text_off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in want])]).tolist()
    assert text == b"".join(want)
    again = api.bgzf_inflate(data)
    assert again[0] == text and again[2].tolist() == status.tolist()


def test_damaged_members_get_the_status_the_host_build_gives_them(built_lib, mixed):
    from kart_amd import api
    texts, members = mixed
    victim = victim_of(texts)
    lo, hi = victim - 3, victim + 3
    at = victim - lo
    for name, bad in cases.damaged_cases(texts, members, victim):
        assert not cases.accepts(bad)[0], name
        text, text_off, status = api.bgzf_inflate(b"".join(members[lo:victim] + [bad] + members[victim + 1:hi]))
        assert status[at] != api.KG_INFLATE_OK, name
        if name == "crc_bit":
            assert status[at] == api.KG_INFLATE_CRC
        assert not np.delete(status, at).any(), name
        pieces = [text[text_off[i]:text_off[i + 1]] for i in range(hi - lo)]
        assert pieces[:at] + pieces[at + 1:] == texts[lo:victim] + texts[victim + 1:hi], name


def test_no_member_one_member_and_the_argument_errors(built_lib, mixed):
    from kart_amd import api
    texts, members = mixed
    text, text_off, status = api.bgzf_inflate(b"")
    assert text == b"" and text_off.tolist() == [0] and len(status) == 0
    text, text_off, status = api.bgzf_inflate(members[0])
    assert text == texts[0] and status.tolist() == [0]
    data = members[0] + members[1]
    m_off, t_off = api.bgzf_members(data)
    for kw, message in (
            (dict(member_off=m_off[::-1].copy(), text_off=t_off), "not from 0 to src_bytes"),
            (dict(member_off=[0, len(data) + 1, len(data)], text_off=t_off), "lie in front of"),
            (dict(member_off=[0, len(members[0]), len(data) - 1], text_off=t_off), "not from 0 to src_bytes"),
            (dict(member_off=m_off, text_off=t_off + 1), "the text begins at 1, not at 0"),
            (dict(member_off=m_off, text_off=[0, len(texts[0]), len(texts[0]) + 65537]), "at most 65536"),
            (dict(member_off=m_off, text_off=t_off, dst_capacity=int(t_off[-1]) - 1), "dst holds")):
        with pytest.raises(api.KartAmdError, match=message):
            api.bgzf_inflate(data, **kw)
    big = members[0] * (65536 // len(members[0]) + 1)
    with pytest.raises(api.KartAmdError, match="at most 65536"):
        api.bgzf_inflate(big, member_off=[0, len(big)], text_off=[0, 10])


def test_round_trip_through_the_projects_own_deflater(built_lib):
    from kart_amd import api
    data = open(os.path.join(ROOT, "DESIGN.md"), "rb").read()[:200000] + random.Random(9).randbytes(65536)
    packed, _, _ = api.bgzf_deflate(data)
    text, _, status = api.bgzf_inflate(packed)
    assert text == data and not status.any()


def test_three_rounds_through_one_inflater(built_lib, mixed):
    """kg_inflater_*: the second round is larger than what the handle was made for -- a run beyond it is KG_ERR_CAPACITY, kg_inflater_reserve grows it"""
    from kart_amd import api
    texts, members = mixed
    rounds = [(members[:3], texts[:3]), (members[3:120], texts[3:120]), (members[200:210], texts[200:210])]
    small = sum(len(m) for m in rounds[0][0])
    k = api.Inflater(small, sum(len(t) for t in rounds[0][1]), 3)
    try:
        for n, (ms, ts) in enumerate(rounds):
            data = b"".join(ms)
            m_off, t_off = api.bgzf_members(data)
            if n == 1:
                with pytest.raises(api.KartAmdError, match="status 4"):
                    k.run(data, m_off, t_off)
                k.reserve(len(data), int(t_off[-1]), len(ms))
            text, status, ms_dev = k.run(data, m_off, t_off)
            assert text == b"".join(ts) and not status.any() and ms_dev > 0, n
    finally:
        k.close()


# ---- the product --------------------------------------------------------------------------------------------------------------------
def cli(args, out, env=None, flag="-o"):
    r = subprocess.run(["timeout", "-k", "10", "300", KART_AMD, "-silent", "-i", SMALL_PREFIX] + args + [flag, out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout.decode()[-400:]
    return open(out, "rb").read()


@pytest.fixture(scope="module")
def pair_files(tmp_path_factory):
    """the files of test_zz_hostpath_gpu.py::test_bgzf_pairs_match_the_golden_sam: mate 1 in members of 0xff00 bytes, mate 2 in random ones"""
    from bgzf_util import bgzf
    d = tmp_path_factory.mktemp("fz")
    rng = random.Random(4)
    files, sizes = [], []
    for m, block in ((1, 0xff00), (2, 3000)):
        raw = gzip.open(os.path.join(SAM, "pe_%d.fq.gz" % m)).read()
        path = str(d / ("b%d.fq.gz" % m))
        open(path, "wb").write(bgzf(raw, block, rng if m == 2 else None))
        files.append(path); sizes.append(len(raw))
    return files, sizes


@pytest.fixture(scope="module")
def session(built_lib):
    """the -fz host side of a comparison: the run the existing tests pin to the reference, made in this process (every -fz device run is a fresh one)"""
    from kart_amd import api
    sess = api.HostSession(SMALL_PREFIX, 0, 16)
    yield sess
    sess.close()


def golden_sam():
    return gzip.open(os.path.join(SAM, "pe.sam.gz")).read()


def test_fz_device_gives_the_golden_sam(built_lib, pair_files, tmp_path):
    files, _ = pair_files
    assert cli(["-f", files[0], "-f2", files[1], "-t", "16", "-fz", "device"], str(tmp_path / "d.sam")) == golden_sam()


def test_fz_device_through_the_general_reader(built_lib, pair_files, tmp_path):
    files, _ = pair_files
    assert cli(["-f", files[0], "-f2", files[1], "-t", "16", "-fz", "device"], str(tmp_path / "g.sam"), {"KART_AMD_NO_STREAM": "1"}) == golden_sam()


def test_an_ordinary_gzip_file_is_not_the_flags_business(built_lib, tmp_path):
    plain = ["-f", os.path.join(SAM, "pe_1.fq.gz"), "-f2", os.path.join(SAM, "pe_2.fq.gz"), "-t", "16", "-fz", "device"]
    assert cli(plain, str(tmp_path / "p.sam")) == golden_sam()


def test_bam_of_fz_device_is_the_file_of_fz_host(built_lib, pair_files, session, tmp_path):
    files, _ = pair_files
    host = str(tmp_path / "h.bam")
    session.map(["-silent", "-f", files[0], "-f2", files[1], "-bo", host, "-fz", "host"])
    assert cli(["-f", files[0], "-f2", files[1], "-t", "16", "-fz", "device"], str(tmp_path / "d.bam"), flag="-bo") == open(host, "rb").read()


STATS_CHILD = """
import json, sys
from kart_amd import api
prefix, runs = sys.argv[1], json.loads(sys.argv[2])
sess = api.HostSession(prefix, 0, 8)
try:
    out = [sess.map(args).as_dict() for args in runs]
finally:
    sess.close()
print(json.dumps([{k: d[k] for k in ("total_reads", "inflate_device_bytes", "inflate_host_bytes", "inflate_device_ms")} for d in out]))
"""


def test_the_stats_say_who_inflated(built_lib, pair_files, tmp_path):
    """kh_stats_t through HostSession.map, in a child process of its own under a time limit"""
    import json
    import sys
    files, sizes = pair_files
    plain = []
    for m in (1, 2):
        plain.append(str(tmp_path / ("p%d.fq" % m)))
        open(plain[-1], "wb").write(gzip.open(os.path.join(SAM, "pe_%d.fq.gz" % m)).read())
    outs = [str(tmp_path / n) for n in ("d.sam", "h.sam", "p.sam")]
    runs = [["-silent", "-f", files[0], "-f2", files[1], "-o", outs[0], "-fz", "device"],
            ["-silent", "-f", files[0], "-f2", files[1], "-o", outs[1], "-fz", "host"],
            ["-silent", "-f", plain[0], "-f2", plain[1], "-o", outs[2], "-fz", "device"]]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", STATS_CHILD, SMALL_PREFIX, json.dumps(runs)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-600:]
    st_d, st_h, st_p = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert (st_d["inflate_device_bytes"], st_d["inflate_host_bytes"]) == (sum(sizes), 0) and st_d["inflate_device_ms"] > 0
    assert (st_h["inflate_device_bytes"], st_h["inflate_host_bytes"], st_h["inflate_device_ms"]) == (0, sum(sizes), 0)
    assert (st_p["inflate_device_bytes"], st_p["inflate_host_bytes"]) == (0, 0)
    want = golden_sam()
    for o in outs:
        assert open(o, "rb").read() == want, o


@pytest.mark.parametrize("name", ["damaged", "foreign", "truncated"])
def test_damaged_foreign_and_truncated_files_give_what_fz_host_gives(built_lib, pair_files, session, tmp_path, name):
    files, _ = pair_files
    data = open(files[0], "rb").read()
    members = cases.split(data)
    k = len(members) // 2
    bad = bytearray(members[k])
    bad[len(bad) // 2] ^= 0x10
    assert not cases.accepts(bytes(bad))[0]
    tail = b"\n".join(gzip.open(os.path.join(SAM, "pe_1.fq.gz")).read().split(b"\n")[:400]) + b"\n"      # a hundred records once more
    blob = {
        "damaged": lambda: b"".join(members[:k] + [bytes(bad)] + members[k + 1:]),
        "foreign": lambda: b"".join(members[:-1]) + gzip.compress(tail),
        "truncated": lambda: data[:len(data) // 2 + 7],
    }[name]()
    path, host = str(tmp_path / (name + ".fq.gz")), str(tmp_path / (name + ".h.sam"))
    open(path, "wb").write(blob)
    st = session.map(["-silent", "-f", path, "-o", host, "-fz", "host"])
    assert st.inflate_device_bytes == 0 and st.inflate_host_bytes > 0
    assert cli(["-f", path, "-t", "16", "-fz", "device"], str(tmp_path / (name + ".d.sam"))) == open(host, "rb").read()
    assert open(host, "rb").read().count(b"\n") > 10
