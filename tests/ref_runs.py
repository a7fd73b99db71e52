"""The unmodified reference's SAM for a test's own (seeded) inputs, also where the reference cannot be run: where oracle/_ref/kart exists
(built from the reference's sources by oracle/Makefile) the run is live and is held to the record in tests/golden/ref_runs.npz; elsewhere
the record stands in for it.  A record is what the tests compare: the exit status, SHA-256 and line count of the SAM and, where a test
compares line by line and the run succeeded, the CRC-32 of every line with and without its FLAG column.  KART_RECORD_REF_RUNS=1 writes
the records of a live run."""
import hashlib
import os
import subprocess
import tempfile
import zlib

import numpy as np

from conftest import GOLDEN, ROOT

KART_REF = os.path.join(ROOT, "oracle", "_ref", "kart")
STORE = os.path.join(GOLDEN, "ref_runs.npz")
CRC_KEYS = ("line_crc", "line_crc_without_flag")


def _crcs(lines):
    return np.array([zlib.crc32(l) for l in lines], dtype="<u4").tobytes()


def _without_flag(line):
    f = line.split(b"\t")
    return b"\t".join(f[:1] + f[2:])


def digest(rc, text, lines=False):
    """the record of one run: exit status and, when the run left a SAM file, its digests"""
    d = {"rc": rc}
    if text is not None:
        d.update(sha256=hashlib.sha256(text).hexdigest(), lines=text.count(b"\n"))
        if lines and rc == 0:
            ls = text.split(b"\n")
            d.update(line_crc=_crcs(ls), line_crc_without_flag=_crcs(_without_flag(l) for l in ls))
    return d


def of(text, lines=False):
    """a product's SAM text (None: no output) as the record it is compared with"""
    return digest(0, text, lines) if text is not None else None


def line_crcs(d, key="line_crc"):
    return np.frombuffer(d[key], dtype="<u4")


def _load():
    """{name: record} from the .npz (one array per record field: <name>:<field>)"""
    store = {}
    if os.path.exists(STORE):
        with np.load(STORE) as z:
            for k in z.files:
                name, field = k.rsplit(":", 1)
                a = z[k]
                store.setdefault(name, {})[field] = (a.tobytes() if field in CRC_KEYS else bytes(a).hex() if field == "sha256" else int(a))
    return store


def _save(store):
    arrays = {}
    for name, d in store.items():
        for field, v in d.items():
            arrays[name + ":" + field] = (np.frombuffer(v, dtype="<u4") if field in CRC_KEYS else
                                          np.frombuffer(bytes.fromhex(v), dtype=np.uint8) if field == "sha256" else np.array(v, dtype=np.int64))
    np.savez_compressed(STORE, **arrays)


def reference(name, args, env=None, lines=False):
    """the record of `kart <args> -o <file>` under `name` (unique in the suite): live where the reference was built, else the stored one"""
    store = _load()
    if not os.path.exists(KART_REF):
        assert name in store, "no record of the reference's run %r in tests/golden/ref_runs.npz and no oracle/_ref/kart to make one" % name
        return store[name]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ref.sam")
        r = subprocess.run([KART_REF] + list(args) + ["-o", out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           env=dict(os.environ, **(env or {})), timeout=600)
        got = digest(r.returncode, open(out, "rb").read() if os.path.exists(out) else None, lines)
    if os.environ.get("KART_RECORD_REF_RUNS") == "1":
        store[name] = got
        _save(store)
    else:
        assert store.get(name) == got, "the reference's run %r differs from its record in tests/golden/ref_runs.npz (KART_RECORD_REF_RUNS=1 writes it again)" % name
    return got
