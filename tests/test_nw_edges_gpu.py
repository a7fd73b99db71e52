"""The gap-closing kernels (nw_kernels.hip) at the edges of their five shape-dependent paths and in both input modes, against the
plain NW of tests/nw_plain.py (both sides <= 80) and the CPU oracle (above; tests/test_nw_plain_cpu.py ties the two together and
to the goldens pinned to the reference's object code).  Every comparison is exact equality of the op bytes: the operation has no
tolerance.  No case is skipped or filtered, and no descriptor-mode request may be handed back (status 0 everywhere).

Offset mode: kg_nw_batch / kg_nw_batch_device with off1/off2 and characters on both sides.  Descriptor mode -- the only one the
product runs: kg_fragments_batch with one side <= 30, which is not partitioned (src/tools.cpp:146) and becomes exactly one NW job
that reads its genome side from the packed 2-bit text.

The small fixture's text (oracle.ref_sequence(), 2 x 103000 characters, forward strand + reverse complement) holds A/C/G/T only --
asserted below -- so no window, the fixed ones at the text's start, end and seam included, meets a character the 2-bit text cannot
hold, and none has to be kept clear of one."""
from collections import namedtuple

import numpy as np
import pytest
import torch

import nw_plain as P
from kart_amd import api

pytestmark = pytest.mark.gpu

Req = namedtuple("Req", "label read gpos glen")


def _expected_ops(oracle, s1: bytes, s2: bytes) -> bytes:
    if len(s1) <= P.PLAIN_MAX and len(s2) <= P.PLAIN_MAX:
        return P.nw_plain(s1, s2)[0]
    return P.ops_of(*oracle.nw(s1, s2))


# ---- offset mode ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def offset_cases(oracle_small):
    """every generated case with its expected op string, built once"""
    cases = P.all_cases()
    return cases, [_expected_ops(oracle_small, c.s1, c.s2) for c in cases]


def test_offset_mode_all_cases_in_one_call(gpu_index, offset_cases):
    cases, want = offset_cases
    # interleaved, so that the three size classes mix in every block of the classify pass
    order = sorted(range(len(cases)), key=lambda i: (i % 97, i))
    got = gpu_index.nw_ops([(cases[i].s1, cases[i].s2) for i in order])
    assert len(got) == len(cases)
    for i, g in zip(order, got):
        assert len(g) == len(want[i]), (cases[i].label, len(g), len(want[i]))              # aln_len
        assert g.tobytes() == want[i], cases[i].label
    assert any(len(c.s1) == 0 for c in cases) and any(len(c.s2) == 0 for c in cases)


def test_position_independence(gpu_index, offset_cases, oracle_small):
    """the same pair gives the same ops at the front of a batch, at its very end and beside a pair that makes the wave-per-pair kernel and
    its scratch part of the call (the plain orderings end in pairs with an empty side or of 9 and 10 bases: what pins nw_small8_kernel's
    byte loads is test_batch_tail_byte_loads below)"""
    cases, want_all = offset_cases
    k = len(P.exhaustive_small())
    small, want = cases[:k], want_all[:k]
    assert all(c.label.startswith("small_") for c in small)
    pairs = [(c.s1, c.s2) for c in small]
    big = P.related_pair(300, 5)
    fwd = gpu_index.nw_ops(pairs)
    rev = gpu_index.nw_ops(pairs[::-1])[::-1]
    plus = gpu_index.nw_ops(pairs + [big])
    assert plus[-1].tobytes() == _expected_ops(oracle_small, *big)
    for c, w, a, b, d in zip(small, want, fwd, rev, plus):
        assert a.tobytes() == w, c.label
        assert b.tobytes() == w, c.label + " (reversed batch)"
        assert d.tobytes() == w, c.label + " (with a 300 x 300 pair behind)"


def test_batch_tail_byte_loads(gpu_index, offset_cases):
    """nw_small8_kernel loads a pair's characters as two 8-byte words, and byte by byte only where those words would leave the batch's
    characters: the last few pairs of a batch.  The orderings of P.tail_orderings() end in pairs of 2 x 2 .. 7 x 6 with N, R, Y and lower case on
    both sides (tests/test_nw_plain_cpu.py holds them to that), and every small pair that is a batch of its own is byte-loaded as well (8 x 8,
    which fits its words exactly, aside): all must give the ops of nw_plain, the same as anywhere else in a batch"""
    cases, want_all = offset_cases
    want = {c.label: w for c, w in zip(cases, want_all)}
    checked = 0
    for name, order in P.tail_orderings().items():
        pairs = [(c.s1, c.s2) for c in order]
        tail = P.byte_path_pairs(pairs)
        assert any(min(len(pairs[k][0]), len(pairs[k][1])) >= 2 and P.is_ambiguous(pairs[k][0]) and P.is_ambiguous(pairs[k][1]) for k in tail), name
        got = gpu_index.nw_ops(pairs)
        for k, (c, g) in enumerate(zip(order, got)):
            assert g.tobytes() == want[c.label], (name, c.label, "byte-loaded" if k in tail else "word-loaded")
        checked += len(tail)
    alone = [c for c in cases if c.label.startswith("small_") and c.label.split("_")[-1] in ("mixed", "rand", "tr3") and 1 <= min(len(c.s1), len(c.s2)) and max(len(c.s1), len(c.s2)) <= 8]
    assert len(alone) == 3 * 64
    for c in alone:
        assert P.byte_path_pairs([(c.s1, c.s2)]) == ([] if (len(c.s1), len(c.s2)) == (8, 8) else [0]), c.label
        (g,) = gpu_index.nw_ops([(c.s1, c.s2)])
        assert g.tobytes() == want[c.label], c.label + " (a batch of its own)"
    assert checked >= 8                       # (nine as the lists stand: 3 + 2 + 2 + 1 + 1, held on the CPU in test_nw_plain_cpu.py)


def test_device_entry_with_max_len_above_the_true_maximum(gpu_index, offset_cases):
    """the caller supplies max_len and the product passes upper bounds: the true maximum, 1000 and 7001 (the HBM-slab path, although every
    pair is small) must give the same ops"""
    cases, want = offset_cases
    sel = [i for i, c in enumerate(cases) if c.label.startswith("edge_")]
    assert len(sel) == 276 * 3
    s1 = [cases[i].s1 for i in sel]; s2 = [cases[i].s2 for i in sel]
    n = len(sel)
    off1 = np.zeros(n + 1, np.int64); off2 = np.zeros(n + 1, np.int64)
    np.cumsum([len(x) for x in s1], out=off1[1:]); np.cumsum([len(x) for x in s2], out=off2[1:])
    true_max = max(max(len(x) for x in s1), max(len(x) for x in s2))
    assert true_max == 513
    dev = torch.device("cuda", 0)
    f1 = torch.from_numpy(np.frombuffer(b"".join(s1) + b"\0" * 16, np.uint8).copy()).to(dev)
    f2 = torch.from_numpy(np.frombuffer(b"".join(s2) + b"\0" * 16, np.uint8).copy()).to(dev)
    d1 = torch.from_numpy(off1).to(dev); d2 = torch.from_numpy(off2).to(dev)
    total = int(off1[n] + off2[n])
    oo = off1 + off2
    stream = torch.cuda.current_stream(dev).cuda_stream
    runs = {}
    for max_len in (true_max, 1000, 7001):
        ops = torch.full((total + 16,), 0xEE, dtype=torch.uint8, device=dev)
        ln = torch.full((n,), -1, dtype=torch.int32, device=dev)
        api._check(gpu_index.lib.kg_nw_batch_device(gpu_index.h, f1.data_ptr(), d1.data_ptr(), f2.data_ptr(), d2.data_ptr(), n, max_len,
                                                    ops.data_ptr(), ln.data_ptr(), stream), "kg_nw_batch_device")
        torch.cuda.synchronize()
        h_ops, h_len = ops.cpu().numpy(), ln.cpu().numpy()
        assert (h_ops[total:] == 0xEE).all(), max_len                                      # nothing written behind the last pair's columns
        runs[max_len] = [h_ops[oo[k]:oo[k] + h_len[k]].tobytes() for k in range(n)]
        for k, i in enumerate(sel):
            assert int(h_len[k]) == len(want[i]), (max_len, cases[i].label)
            assert runs[max_len][k] == want[i], (max_len, cases[i].label)
    assert runs[true_max] == runs[1000] == runs[7001]


# ---- descriptor mode ------------------------------------------------------------------------------------------------------------
DESC_N = (1, 4, 7, 8, 9, 30, 31, 32, 33, 64, 65, 128, 129, 256, 257, 513)
DESC_M = (1, 8, 9, 30)
DESC_LONG_M = (33, 129, 257, 600)
DESC_SHORT_N = (1, 8, 30)


def _read_for(rng, window: bytes, m: int) -> bytes:
    """a read fragment of exactly m bases cut from the text window (with random flanks where the window is shorter) and mutated:
    substitutions and indels"""
    src = window
    if len(src) < m + 2:
        pad = m + 2 - len(src)
        src = P.rand_seq(rng, pad // 2) + src + P.rand_seq(rng, pad - pad // 2)
    at = int(rng.integers(0, len(src) - m + 1))
    return P.mutate_to(rng, src[at:at + m + 1], m)


def _ambiguous(rng, read: bytes) -> bytes:
    """the same fragment with an N and lower case in it (allowed while a side is <= 30)"""
    b = bytearray(read.lower() if len(read) < 3 else read[:len(read) // 2] + read[len(read) // 2:].lower())
    b[int(rng.integers(0, len(b)))] = ord("N")
    if len(b) > 4:
        b[int(rng.integers(0, len(b)))] = ord("n")
    return bytes(b)


def _descriptor_requests(text: np.ndarray):
    rng = np.random.default_rng(20243)
    two_l = len(text)
    L = two_l // 2
    shapes = [(m, n) for n in DESC_N for m in DESC_M] + [(m, n) for m in DESC_LONG_M for n in DESC_SHORT_N]
    reqs = []

    def add(label, m, gpos, n, ambiguous=False):
        assert 0 <= gpos and gpos + n <= two_l and min(m, n) <= 30
        read = _read_for(rng, text[gpos:gpos + n].tobytes(), m)
        if ambiguous:
            read = _ambiguous(rng, read)
        reqs.append(Req(label, read, gpos, n))

    # every shape at the four phases of the packed 2-bit text, plain reads and reads with N / lower case
    for m, n in shapes:
        base = 4 * int(rng.integers(1000, (two_l - 2000) // 4))
        if base <= L < base + n + 3:                                      # (the seam has windows of its own below)
            base += 4 * 200
        for ph in range(4):
            add("desc_%dx%d_phase%d" % (m, n, ph), m, base + ph, n)
        ph = int(rng.integers(0, 4))
        add("desc_%dx%d_phase%d_ambiguous" % (m, n, ph), m, base + 1000 + ph, n, ambiguous=True)
    # the very first and the very last bases of the indexed text, and windows across the forward / reverse-complement seam
    for m, n in shapes:
        add("desc_%dx%d_text_start" % (m, n), m, 0, n)
        add("desc_%dx%d_text_end" % (m, n), m, two_l - n, n)
        if n >= 2:
            for left in sorted({1, n // 2, n - 1}):
                add("desc_%dx%d_seam_left%d" % (m, n, left), m, L - left, n)
    return reqs


@pytest.fixture(scope="module")
def descriptor_set(oracle_small):
    text = oracle_small.ref_sequence()
    assert len(text) == 2 * oracle_small.genome_size
    assert np.isin(text, np.frombuffer(b"ACGT", np.uint8)).all()              # see the module docstring
    reqs = _descriptor_requests(text)
    want = [_expected_ops(oracle_small, r.read, text[r.gpos:r.gpos + r.glen].tobytes()) for r in reqs]
    return reqs, want


def _run_fragments(ix, reqs, pacbio):
    ops, status = ix.fragments_ops([r.read for r in reqs], [r.gpos for r in reqs], [r.glen for r in reqs], pacbio=pacbio, max_gaps=5)
    assert len(ops) == len(reqs) == len(status)
    return ops, status


def test_descriptor_requests_are_what_they_should_be(descriptor_set, oracle_small):
    reqs, _ = descriptor_set
    two_l = 2 * oracle_small.genome_size
    L = two_l // 2
    labels = [r.label for r in reqs]
    assert len(set(labels)) == len(labels)
    want_shapes = {(m, n) for n in DESC_N for m in DESC_M} | {(m, n) for m in DESC_LONG_M for n in DESC_SHORT_N}
    for ph in range(4):
        assert {(len(r.read), r.glen) for r in reqs if r.label.endswith("_phase%d" % ph) and r.gpos % 4 == ph} == want_shapes
    assert {(len(r.read), r.glen) for r in reqs if r.gpos == 0} == want_shapes
    assert {(len(r.read), r.glen) for r in reqs if r.gpos + r.glen == two_l} == want_shapes
    assert {(len(r.read), r.glen) for r in reqs if r.gpos < L < r.gpos + r.glen} == {s for s in want_shapes if s[1] >= 2}
    assert {(len(r.read), r.glen) for r in reqs if r.label.endswith("_ambiguous")} == want_shapes
    assert all(set(r.read) - set(b"ACGT") for r in reqs if r.label.endswith("_ambiguous"))
    assert all(min(len(r.read), r.glen) <= 30 and len(r.read) >= 1 and r.glen >= 1 for r in reqs)


@pytest.mark.parametrize("mode", ["pacbio", "illumina"])
def test_descriptor_mode_direct_jobs(gpu_index_full, descriptor_set, mode):
    reqs, want = descriptor_set
    ops, status = _run_fragments(gpu_index_full, reqs, pacbio=(mode == "pacbio"))
    assert not np.asarray(status).any(), [r.label for r, s in zip(reqs, status) if s]       # zero handed back
    for r, w, g in zip(reqs, want, ops):
        assert len(g) == len(w), (mode, r.label, len(g), len(w))
        assert g.tobytes() == w, (mode, r.label)


def test_tier_boundary(gpu_index_full, descriptor_set):
    """kg_fragments_batch hands kgi_nw_launch the longest side of the call's requests as max_len (abi_frag.hip: max_len = max over m and
    glen), and the two-tier launch needs a.desc and 512 < max_len <= 7000 (abi.hip, kgi_nw_launch): one direct job with a 600-base read makes the
    first call a two-tier one -- its jobs of 33..256 columns run in the tier-1 launch, the 257-column ones and the 600 in the other -- and
    without it the same requests (max_len = 257) run in one launch.  Same ops either way."""
    reqs, want = descriptor_set
    sel = [i for i, r in enumerate(reqs) if 33 <= r.glen <= 257 and len(r.read) <= 30]
    long_one = [i for i, r in enumerate(reqs) if len(r.read) == 600 and r.glen == 30][:1]
    assert len(sel) > 100 and len(long_one) == 1 and {reqs[i].glen for i in sel} == {33, 64, 65, 128, 129, 256, 257}
    with_long = sel[:len(sel) // 2] + long_one + sel[len(sel) // 2:]
    assert max(max(len(reqs[i].read), reqs[i].glen) for i in with_long) == 600 and max(max(len(reqs[i].read), reqs[i].glen) for i in sel) == 257
    ops_a, st_a = _run_fragments(gpu_index_full, [reqs[i] for i in with_long], pacbio=True)
    ops_b, st_b = _run_fragments(gpu_index_full, [reqs[i] for i in sel], pacbio=True)
    assert not np.asarray(st_a).any() and not np.asarray(st_b).any()
    a = {i: g.tobytes() for i, g in zip(with_long, ops_a)}
    b = {i: g.tobytes() for i, g in zip(sel, ops_b)}
    assert a[long_one[0]] == want[long_one[0]], reqs[long_one[0]].label
    for i in sel:
        assert a[i] == want[i], reqs[i].label + " (two tiers)"
        assert b[i] == want[i], reqs[i].label + " (one launch)"
        assert a[i] == b[i], reqs[i].label
