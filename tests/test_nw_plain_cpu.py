"""The plain NW of tests/nw_plain.py against the CPU oracle and the goldens pinned to the reference's object code, and the case
lists of the NW edge tests: what tests/test_nw_edges_gpu.py compares the kernels with is checked here, without a GPU."""
import pytest

import nw_plain as P
from kart_amd import api


@pytest.fixture(scope="module")
def cases():
    return {"small": P.exhaustive_small(), "edge": P.boundary_shapes(), "runs": P.long_runs()}


def test_op_codes_are_the_abi_s():
    assert (P.OP_DIAG, P.OP_GAP1, P.OP_GAP2) == (api.KG_OP_DIAG, api.KG_OP_GAP1, api.KG_OP_GAP2)


def test_plain_equals_oracle_on_every_small_enough_case(cases, oracle_small):
    compared = 0
    for c in cases["small"] + cases["edge"] + cases["runs"]:
        if not P.is_plain_size(c):
            continue
        ops, a1, a2 = P.nw_plain(c.s1, c.s2)
        assert (a1, a2) == oracle_small.nw(c.s1, c.s2), c.label
        assert P.ops_of(a1, a2) == ops and P.gapped(c.s1, c.s2, ops) == (a1, a2), c.label
        compared += 1
    # the whole small grid and every boundary shape with both sides <= 80
    small_edge = sum(1 for m, n in P.boundary_shape_list() if m <= P.PLAIN_MAX and n <= P.PLAIN_MAX)
    assert compared == len(cases["small"]) + small_edge * len(P.BOUNDARY_FLAVOURS)
    assert small_edge == 96                      # 10 x 8 shapes with n <= 65, their transposes, the 8 x 8 common ones counted once


def test_plain_equals_pinned_goldens(golden):
    compared = 0
    for s1, s2, g1, g2 in zip(golden["nw_s1"], golden["nw_s2"], golden["nw_a1"], golden["nw_a2"]):
        s1, s2 = bytes(s1), bytes(s2)
        if len(s1) > P.PLAIN_MAX or len(s2) > P.PLAIN_MAX:
            continue
        ops, a1, a2 = P.nw_plain(s1, s2)
        assert (a1, a2) == (bytes(g1), bytes(g2)), (s1, s2)
        compared += 1
    assert compared > 1000


def test_oracle_round_trips_on_the_larger_cases(cases, oracle_small):
    checked = 0
    for c in cases["edge"] + cases["runs"]:
        if P.is_plain_size(c):
            continue
        a1, a2 = oracle_small.nw(c.s1, c.s2)
        assert len(a1) == len(a2), c.label
        assert a1.replace(b"-", b"") == c.s1 and a2.replace(b"-", b"") == c.s2, c.label
        assert not any(x == 0x2D and y == 0x2D for x, y in zip(a1, a2)), c.label
        checked += 1
    assert checked == sum(1 for c in cases["edge"] + cases["runs"] if not P.is_plain_size(c)) > 500


def test_case_lists(cases):
    small, edge, runs = cases["small"], cases["edge"], cases["runs"]
    every = small + edge + runs
    labels = [c.label for c in every]
    assert len(set(labels)) == len(labels)
    assert all(len(c.s1) + len(c.s2) > 0 for c in every)
    assert all(b"-" not in c.s1 and b"-" not in c.s2 for c in every)
    # the small grid: every (m, n) of 0..10 x 0..10 but (0, 0), every flavour
    grid = {(m, n) for m in range(11) for n in range(11)} - {(0, 0)}
    for f in P.SMALL_FLAVOURS:
        assert {(len(c.s1), len(c.s2)) for c in small if c.label.endswith("_" + f)} == grid, f
    assert len(small) == 120 * 7 and len(P.SMALL_FLAVOURS) == 7
    by = {c.label: c for c in small}
    assert by["small_7x7_ident"].s1 == by["small_7x7_ident"].s2
    c = by["small_9x4_homo_same"]
    assert len(set(c.s1 + c.s2)) == 1
    c = by["small_9x4_homo_diff"]
    assert len(set(c.s1)) == 1 and len(set(c.s2)) == 1 and c.s1[0] != c.s2[0]
    c = by["small_10x10_tr2"]
    assert c.s1[:2] * 5 == c.s1 and c.s2 == c.s1[1:] + c.s1[:1]
    c = by["small_10x10_tr3"]
    assert c.s1 == (c.s1[:3] * 4)[:10] and c.s2 != c.s1 and c.s2 in c.s1[:3] * 6
    assert any(set(c.s1 + c.s2) & set(b"NnRY") and set(c.s1 + c.s2) & set(b"acgt") for c in small if c.label.endswith("_mixed"))
    # the boundary shapes: the listed cross product and its transpose, every flavour
    M = (1, 2, 8, 9, 31, 32, 33, 63, 64, 65)
    N = (1, 8, 9, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
    want = {(m, n) for m in M for n in N} | {(n, m) for m in M for n in N}
    assert len(want) == 276
    for f in P.BOUNDARY_FLAVOURS:
        assert {(len(c.s1), len(c.s2)) for c in edge if c.label.endswith("_" + f)} == want, f
    assert len(edge) == 276 * 3
    for c in edge:
        if c.label.endswith("_homo"):
            assert len(set(c.s1 + c.s2)) == 1, c.label
        if c.label.endswith("_unrelated"):
            assert not (set(c.s1) & set(c.s2)), c.label
    # the long runs: the listed shapes, in both directions
    shapes = {(len(c.s1), len(c.s2)) for c in runs}
    assert {(600, 3), (3, 600), (600, 33), (33, 600), (300, 500), (500, 300), (700, 400), (400, 700)} <= shapes


def test_long_runs_do_force_long_pure_runs(cases, oracle_small):
    """the point of long_runs(): a vertical and a horizontal run of more than 256 columns, and runs of more than 64"""
    def longest(a):
        best = cur = 0
        for x in a:
            cur = cur + 1 if x == 0x2D else 0
            best = max(best, cur)
        return best
    v = h = 0
    for c in cases["runs"]:
        a1, a2 = oracle_small.nw(c.s1, c.s2)
        assert max(longest(a1), longest(a2)) > 64, c.label
        h, v = max(h, longest(a1)), max(v, longest(a2))
    assert h > 256 and v > 256


def test_tail_orderings_put_pairs_that_matter_on_the_byte_loaded_tail():
    """nw_small8_kernel loads the last few small pairs of an offset-mode batch byte by byte (P.byte_path_pairs restates its condition).  The
    plain orderings of the small grid end in pairs with an empty side or in 9- and 10-base pairs, for which those loads cannot change a result:
    the orderings of P.tail_orderings() must end in pairs with both sides >= 2 and characters outside upper-case A/C/G/T, among them pairs of
    5 x 5 and more -- test_nw_edges_gpu.py compares exactly these with nw_plain"""
    small = P.exhaustive_small()
    for name, pairs in (("forward", small), ("reversed", small[::-1])):
        assert all(min(len(pairs[k].s1), len(pairs[k].s2)) == 0 for k in P.byte_path_pairs([(c.s1, c.s2) for c in pairs])), name
    seen = {}
    for name, order in P.tail_orderings().items():
        assert sorted(c.label for c in order) == sorted(c.label for c in small), name
        on_tail = [order[k] for k in P.byte_path_pairs([(c.s1, c.s2) for c in order])]
        good = [c for c in on_tail if min(len(c.s1), len(c.s2)) >= 2 and P.is_ambiguous(c.s1) and P.is_ambiguous(c.s2)]
        assert good, name
        if name.startswith("mixed_"):
            assert len(good) >= 2, (name, [c.label for c in on_tail])
        else:
            assert any(min(len(c.s1), len(c.s2)) >= 5 for c in good), (name, [c.label for c in on_tail])
        seen.update((c.label, c) for c in good)
    assert len(seen) >= 8, sorted(seen)
    assert any(any(ch in b"acgt" for ch in c.s1 + c.s2) for c in seen.values()) and any(any(ch in b"NnRY" for ch in c.s1 + c.s2) for c in seen.values())
