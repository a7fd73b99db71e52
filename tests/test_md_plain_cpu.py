"""CPU: tests/md_plain.py -- the plain-Python MD:Z every other MD test measures the product with -- against known answers written by hand."""
import random

from md_plain import md_of, ref_from_md, reference_at


def test_the_specifications_own_example():
    # SAMv1 1.5: "10A5^AC6" -- ten matches, a reference A against another base, five matches, AC deleted from the read, six matches
    ref = "CCCCCCCCCC" + "A" + "GGGGG" + "AC" + "TTTTTT"
    seq = "CCCCCCCCCC" + "T" + "GGGGG" + "TTTTTT"
    assert md_of(seq, "16M2D6M", reference_at(ref, 1)) == "10A5^AC6"
    assert ref_from_md(seq, "16M2D6M", "10A5^AC6") == ref


def test_hand_written_answers():
    ref = "ACGTACGTACGTACGTACGT"
    at = reference_at(ref, 1)
    assert md_of("ACGTACGT", "8M", at) == "8"
    assert md_of("TCGTACGA", "8M", at) == "0A6T0"                       # first and last column: the string starts and ends with a number
    assert md_of("ACTAACGT", "8M", at) == "2G0T4"                       # two adjacent mismatches: a 0 between them
    assert md_of("ACTACCGT", "8M", at) == "2G0T0A3"                     # three
    assert md_of("ACGTTTACGT", "4M2I4M", at) == "8"                     # an insertion leaves no trace
    assert md_of("ACGTGT", "4M2D2M", at) == "4^AC2"                     # a deletion
    assert md_of("ACGTTT", "4M2D2M", at) == "4^AC0G1"                   # ... directly followed by a mismatch: a 0 between them
    assert md_of("GGACGTACGG", "2S6M2S", at) == "6"                     # soft clips consume read only
    assert md_of("acgtacgt", "8M", at) == "8"                           # lower case matches
    assert md_of("ACNTACGT", "8M", at) == "2G5" and md_of("ACnTACGT", "8M", at) == "2G5"
    assert md_of("ACRTACGT", "8M", at) == "2G5"                         # IUPAC in the read: a mismatch, whatever it stands for
    assert md_of("AC=TACGT", "8M", at) == "8"                           # '=' matches
    assert md_of("ACGT", "2M4N2M", at) == "4"                           # N skips reference: columns 3, 4 face ref[6], ref[7] = G, T
    assert md_of("ACTT", "2M4N2M", at) == "2G1"
    assert md_of("CGTA", "4M", reference_at(ref, 2)) == "4"             # POS
    assert md_of("ACGT", "4M", reference_at(ref, 19)) == "0G0T0N0N0"    # past the contig's end: N, never a match


def test_a_long_string_built_by_hand_from_a_toy_reference():
    # 6G4C20G1A5C5A1^C3A15G1G15 -- the shape of a real record: nine mismatches and one deleted base
    pieces = [(6, "G"), (4, "C"), (20, "G"), (1, "A"), (5, "C"), (5, "A"), (1, "^C"), (3, "A"), (15, "G"), (1, "G"), (15, None)]
    rng = random.Random(5)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    ref, seq, m_cols, cigar = [], [], 0, []
    for n, what in pieces:
        # n matching columns whose bases differ from their neighbours' mismatch letters only by chance: any base will do
        run = [rng.choice("ACGT") for _ in range(n)]
        ref += run
        seq += run
        m_cols += n
        if what is None:
            continue
        if what[0] == "^":
            cigar.append("%dM%dD" % (m_cols, len(what) - 1))
            m_cols = 0
            ref += list(what[1:])
        else:
            ref.append(what)
            seq.append(other[what])
            m_cols += 1
    cigar.append("%dM" % m_cols)
    ref, seq, cigar = "".join(ref), "".join(seq), "".join(cigar)
    want = "6G4C20G1A5C5A1^C3A15G1G15"
    assert md_of(seq, cigar, reference_at(ref, 1)) == want
    assert ref_from_md(seq, cigar, want) == ref


def test_holes_show_their_own_character_and_never_match():
    stored = "ACGTACGTACGT"                       # what the index holds: random bases where the FASTA had N / R
    holes = [(2, 1, "N"), (5, 3, "n"), (10, 1, "R")]
    at = reference_at(stored, 1, holes)
    assert md_of(stored, "12M", at) == "2N2N0N0N2R1"          # the read equals the stored bases: still a mismatch at every hole
    assert md_of("ACNTACGTACRT", "12M", at) == "2N2N0N0N2R1"  # N against N, R against R: no match either
    assert md_of("AC=TA===AC=T", "12M", at) == "12"           # '=' matches whatever the reference shows
    assert md_of("ACTT", "2M8D2M", at) == "2^NTANNNAC0R1"


def test_round_trip_on_random_alignments():
    rng = random.Random(11)
    for _ in range(300):
        ref = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 120)))
        seq, cigar, g = [], [], 0
        if rng.random() < 0.3:
            n = rng.randint(1, 9)
            seq += [rng.choice("ACGTN") for _ in range(n)]
            cigar.append("%dS" % n)
        last = None
        while g < len(ref):
            op = rng.choice("MMMID") if last == "M" else "M"
            n = min(rng.randint(1, 40), len(ref) - g) if op != "I" else rng.randint(1, 5)
            if op == "M":
                seq += [c if rng.random() < 0.85 else rng.choice("ACGTNacgtR") for c in ref[g:g + n]]
                g += n
            elif op == "I":
                seq += [rng.choice("ACGT") for _ in range(n)]
            else:
                if g + n >= len(ref):
                    op, n = "M", len(ref) - g
                    seq += list(ref[g:])
                g += n
            if cigar and cigar[-1].endswith(op):
                cigar[-1] = "%d%s" % (int(cigar[-1][:-1]) + n, op)
            else:
                cigar.append("%d%s" % (n, op))
            last = op
        seq, cigar = "".join(seq), "".join(cigar)
        md = md_of(seq, cigar, reference_at(ref, 1))
        assert ref_from_md(seq, cigar, md) == ref, (seq, cigar, md, ref)
