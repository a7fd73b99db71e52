"""A plain Needleman-Wunsch for tests, and the case lists the NW tests share (imported by name, like bgzf_util and ref_runs).

nw_plain states the operation of the reference's nw_alignment (src/nw_alignment.cpp:18-80) in the simplest form: three full
(m+1) x (n+1) float matrices -- every value is a multiple of 0.5, so float64 is exact -- the reference's boundary rows and columns,
characters compared through a 256-entry table (ACGTacgt -> 0..3, everything else 4), and a walk back from the corner that prefers a
gap in sequence 1, then a gap in sequence 2, then a pair of bases.  It shares no code with oracle/ or with the kernels, and is meant
for sides of up to 80 bases (PLAIN_MAX): it is slow on purpose.

The generators are seeded and deterministic; every case carries a label that names its shape and flavour."""
from collections import namedtuple

import numpy as np

OP_DIAG, OP_GAP1, OP_GAP2 = 0, 1, 2         # = KG_OP_DIAG, KG_OP_GAP1 (gap in sequence 1), KG_OP_GAP2 (checked in test_nw_plain_cpu.py)
PLAIN_MAX = 80

# scores, as floats (all multiples of 0.5): equal bases +1.5, different bases -1.5, the first base of a gap -1.5, every further one -0.5;
# the edge of the matrix after k bases costs 1 + k / 2; "cannot be" is -65536
SAME, DIFFERENT = 1.5, -1.5
GAP_FIRST, GAP_NEXT = -1.5, -0.5
NEVER = -65536.0

CODE = [4] * 256
for _k, _c in enumerate(b"ACGT"):
    CODE[_c] = _k
    CODE[_c + 32] = _k                        # lower case

Case = namedtuple("Case", "label s1 s2")


def _edge(k):
    return -1.0 - 0.5 * k


def nw_plain(s1: bytes, s2: bytes):
    """-> (ops as bytes of OP_*, gapped s1, gapped s2).
    best[i][j]: the best alignment of s1[:i] with s2[:j]; in1[i][j]: the best one that ends in a gap in sequence 1 (s2[j-1] against '-');
    in2[i][j]: the best one that ends in a gap in sequence 2."""
    m, n = len(s1), len(s2)
    best = [[0.0] * (n + 1) for _ in range(m + 1)]
    in1 = [[0.0] * (n + 1) for _ in range(m + 1)]
    in2 = [[0.0] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):                 # column 0: only gaps in sequence 2
        best[i][0] = in2[i][0] = _edge(i)
        in1[i][0] = NEVER
    for j in range(1, n + 1):                 # row 0: only gaps in sequence 1
        best[0][j] = in1[0][j] = _edge(j)
        in2[0][j] = NEVER
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            longer1, new1 = in1[i][j - 1] + GAP_NEXT, best[i][j - 1] + GAP_FIRST
            longer2, new2 = in2[i - 1][j] + GAP_NEXT, best[i - 1][j] + GAP_FIRST
            in1[i][j] = max(longer1, new1)
            in2[i][j] = max(longer2, new2)
            pair = best[i - 1][j - 1] + (SAME if CODE[s1[i - 1]] == CODE[s2[j - 1]] else DIFFERENT)
            best[i][j] = max(pair, in1[i][j], in2[i][j])
    # back from the corner; where scores tie, a gap in sequence 1 wins over a gap in sequence 2, and that over a pair of bases
    ops = []
    i, j = m, n
    while i > 0 or j > 0:
        if best[i][j] == in1[i][j]:
            ops.append(OP_GAP1)
            j -= 1
        elif best[i][j] == in2[i][j]:
            ops.append(OP_GAP2)
            i -= 1
        else:
            ops.append(OP_DIAG)
            i -= 1
            j -= 1
    ops.reverse()
    a1, a2 = gapped(s1, s2, ops)
    return bytes(ops), a1, a2


def gapped(s1: bytes, s2: bytes, ops):
    """the two gapped strings an op string describes"""
    a1, a2 = bytearray(), bytearray()
    i = j = 0
    for op in ops:
        if op == OP_GAP1:
            a1.append(0x2D); a2.append(s2[j]); j += 1
        elif op == OP_GAP2:
            a1.append(s1[i]); a2.append(0x2D); i += 1
        else:
            a1.append(s1[i]); a2.append(s2[j]); i += 1; j += 1
    assert i == len(s1) and j == len(s2)
    return bytes(a1), bytes(a2)


def ops_of(a1: bytes, a2: bytes) -> bytes:
    """the op string of two gapped strings (no test sequence contains '-')"""
    assert len(a1) == len(a2)
    return bytes(OP_GAP1 if x == 0x2D else OP_GAP2 if y == 0x2D else OP_DIAG for x, y in zip(a1, a2))


# ---- case generators ------------------------------------------------------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_MIXED = np.frombuffer(b"NnRYacgtACGT", np.uint8)

SMALL_FLAVOURS = ("rand", "ident", "homo_same", "homo_diff", "tr2", "tr3", "mixed")
BOUNDARY_M = (1, 2, 8, 9, 31, 32, 33, 63, 64, 65)
BOUNDARY_N = (1, 8, 9, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
BOUNDARY_FLAVOURS = ("related", "homo", "unrelated")


def rand_seq(rng, k, alphabet=_ACGT):
    return alphabet[rng.integers(0, len(alphabet), size=k)].tobytes()


def _repeat(unit: bytes, shift: int, k: int) -> bytes:
    return (unit * (k // len(unit) + 2))[shift:shift + k]


def mutate_to(rng, src: bytes, k: int) -> bytes:
    """a copy of `src` with substitutions and indels (about one edit per 12 bases, at least one of each kind where there is room),
    cut or filled with random bases to exactly k"""
    b = list(src)
    edits = max(3, len(b) // 12)
    for e in range(edits):
        kind = e % 3
        if kind == 0 and len(b) > 1:
            del b[int(rng.integers(0, len(b)))]
        elif kind == 1:
            b.insert(int(rng.integers(0, len(b) + 1)), int(_ACGT[rng.integers(0, 4)]))
        elif b:
            b[int(rng.integers(0, len(b)))] = int(_ACGT[rng.integers(0, 4)])
    b = b[:k]
    while len(b) < k:
        b.append(int(_ACGT[rng.integers(0, 4)]))
    return bytes(b)


def boundary_shape_list():
    shapes = []
    for m in BOUNDARY_M:
        for n in BOUNDARY_N:
            for sh in ((m, n), (n, m)):
                if sh not in shapes:
                    shapes.append(sh)
    return shapes


def exhaustive_small():
    """every (m, n) in 0..10 x 0..10 but (0, 0), seven flavours each"""
    rng = np.random.default_rng(20240)
    cases = []
    for m in range(11):
        for n in range(11):
            if m == 0 and n == 0:
                continue
            base = "ACGT"[(m + n) % 4].encode()
            other = "ACGT"[(m + n + 1 + m % 3) % 4].encode()
            common = rand_seq(rng, max(m, n))
            flav = {
                "rand": (rand_seq(rng, m), rand_seq(rng, n)),
                "ident": (common[:m], common[:n]),                     # identical where both exist (m == n: identical sequences)
                "homo_same": (base * m, base * n),
                "homo_diff": (base * m, other * n),
                "tr2": (_repeat(b"AC", 0, m), _repeat(b"AC", 1, n)),
                "tr3": (_repeat(b"ACG", 0, m), _repeat(b"ACG", 1 + (m + n) % 2, n)),
                "mixed": (rand_seq(rng, m, _MIXED), rand_seq(rng, n, _MIXED)),
            }
            for f in SMALL_FLAVOURS:
                cases.append(Case("small_%dx%d_%s" % (m, n, f), flav[f][0], flav[f][1]))
    return cases


def boundary_shapes():
    """BOUNDARY_M x BOUNDARY_N and its transpose, three flavours each"""
    rng = np.random.default_rng(20241)
    cases = []
    for m, n in boundary_shape_list():
        common = rand_seq(rng, max(m, n) + 8)
        hb = "ACGT"[(m + n) % 4].encode()
        flav = {
            "related": (common[:m], mutate_to(rng, common[:n], n)),
            "homo": (hb * m, hb * n),
            "unrelated": (rand_seq(rng, m, np.frombuffer(b"AG", np.uint8)), rand_seq(rng, n, np.frombuffer(b"CT", np.uint8))),
        }
        for f in BOUNDARY_FLAVOURS:
            cases.append(Case("edge_%dx%d_%s" % (m, n, f), flav[f][0], flav[f][1]))
    return cases


def long_runs():
    """pure vertical and horizontal runs longer than 64 and longer than 256, inside one stripe and across stripes"""
    rng = np.random.default_rng(20242)
    cases = []
    for m, n in ((600, 3), (3, 600), (600, 33), (33, 600)):
        long_side = rand_seq(rng, max(m, n))
        piece = long_side[300:300 + min(m, n)]                             # the short side lies in the middle of the long one
        cases.append(Case("run_%dx%d_sub" % (m, n), *((long_side, piece) if m > n else (piece, long_side))))
        cases.append(Case("run_%dx%d_homo" % (m, n), b"A" * m, b"A" * n))
        cases.append(Case("run_%dx%d_unrelated" % (m, n), b"G" * m, b"T" * n))
    cases.append(Case("run_300A_vs_300A200C", b"A" * 300, b"A" * 300 + b"C" * 200))
    cases.append(Case("run_300A200C_vs_300A", b"A" * 300 + b"C" * 200, b"A" * 300))
    cases.append(Case("run_200C300A_vs_300A", b"C" * 200 + b"A" * 300, b"A" * 300))
    cases.append(Case("run_300A_vs_200C300A", b"A" * 300, b"C" * 200 + b"A" * 300))
    full = rand_seq(rng, 700)
    cut = full[:200] + full[500:]                                          # a 300-base block deleted from the middle
    cases.append(Case("run_700_vs_block_deleted", full, cut))
    cases.append(Case("run_block_deleted_vs_700", cut, full))
    tr = _repeat(b"ACG", 0, 700)
    cases.append(Case("run_tr3_700_vs_400", tr, tr[:400]))
    cases.append(Case("run_tr3_400_vs_700", tr[:400], tr))
    return cases


def related_pair(k: int, seed: int):
    """a k x k pair of related sequences with indels (what makes the wave-per-pair kernel part of a batch of small pairs)"""
    rng = np.random.default_rng(seed)
    a = rand_seq(rng, k)
    return a, mutate_to(rng, a, k)


def is_ambiguous(seq: bytes) -> bool:
    return any(c not in b"ACGT" for c in seq)


def byte_path_pairs(pairs):
    """which pairs of an offset-mode batch nw_small8_kernel loads byte by byte: those of up to 8 x 8 whose eight bytes from their first
    character on would leave the batch's characters on either side -- the last few of the batch, and only where they are small"""
    t1 = sum(len(a) for a, _ in pairs)
    t2 = sum(len(b) for _, b in pairs)
    out, o1, o2 = [], 0, 0
    for k, (a, b) in enumerate(pairs):
        if max(len(a), len(b)) <= 8 and (o1 + 8 > t1 or o2 + 8 > t2):
            out.append(k)
        o1 += len(a)
        o2 += len(b)
    return out


def tail_orderings():
    """orderings of exhaustive_small() that end in pairs of up to 8 x 8 with both sides non-empty and characters that matter, so that these
    are what the batch's byte-loaded tail consists of: name -> list of cases"""
    small = exhaustive_small()

    def ends_with(pick, key):
        tail = sorted((c for c in small if pick(c)), key=key)
        return [c for c in small if not pick(c)] + tail

    def shape(c):
        return len(c.s1), len(c.s2)

    def is_mixed(c, lo, hi):
        return c.label.endswith("_mixed") and lo <= min(shape(c)) and max(shape(c)) <= hi

    return {
        # the smallest mixed pairs last: 3x2, 2x3, 2x2 all lie within the last eight characters of both sides
        "mixed_2to8_smallest_last": ends_with(lambda c: is_mixed(c, 2, 8), lambda c: (-sum(shape(c)), c.label)),
        # ... and 3x3, 2x3, 3x2 / 4x4, 3x4: other shapes and other positions of the last eight
        "mixed_3to8_smallest_last": ends_with(lambda c: is_mixed(c, 3, 8), lambda c: (-sum(shape(c)), c.label)),
        "mixed_2to4_largest_last": ends_with(lambda c: is_mixed(c, 2, 4), lambda c: (sum(shape(c)), c.label)),
        # random, tandem-repeat and mixed pairs of 5..8 x 5..8, a 5 x 5 .. 7 x 7 mixed pair last: most of the register matrix in use
        "mid_5to8_mixed_5x5_last": ends_with(lambda c: 5 <= min(shape(c)) and max(shape(c)) <= 8 and c.label.split("_")[-1] in ("rand", "tr2", "tr3", "mixed"),
                                             lambda c: (c.label.endswith("_mixed"), -sum(shape(c)), c.label)),
        "mid_5to8_mixed_7x6_last": ends_with(lambda c: 5 <= min(shape(c)) and max(shape(c)) <= 8 and c.label.split("_")[-1] in ("rand", "tr2", "tr3", "mixed"),
                                             lambda c: (c.label == "small_7x6_mixed", c.label == "small_6x7_mixed", c.label.endswith("_mixed"), c.label)),
    }


def all_cases():
    return exhaustive_small() + boundary_shapes() + long_runs()


def is_plain_size(c) -> bool:
    return len(c.s1) <= PLAIN_MAX and len(c.s2) <= PLAIN_MAX
