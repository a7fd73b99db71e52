"""CPU: the plain specification of -un / -un2 (tests/un_plain.py) on hand-written inputs, expected bytes written out."""
import un_plain

H = "@PG\tID:kart\n@SQ\tSN:chrA\tLN:100\n"


def sam(*records):
    """(name, flag) -> a SAM text with the columns the specification reads"""
    return (H + "".join("%s\t%d\t%s\t0\t0\t*\t*\t0\t0\tACGT\tIIII\tAS:i:0\tXS:i:0\n" % (n, f, "*" if f & 4 else "chrA") for n, f in records)).encode()


def test_wrapped_fasta_record():
    text = b">r1 first\nACGT\nacgt\nAC\n>r2\nGG\n>r3\nTTTT\nTT\n"
    assert un_plain.spans(text, True) == [(0, 23), (23, 30), (30, 42)]          # (10 + 5 + 5 + 3 bytes, 4 + 3, 4 + 5 + 3)
    assert un_plain.records(text, True) == [b">r1 first\nACGT\nacgt\nAC\n", b">r2\nGG\n", b">r3\nTTTT\nTT\n"]
    got = un_plain.expected([text], sam(("r1", 4), ("r2", 0), ("r3", 4)), False, False, fasta=True)
    assert got == (b">r1 first\nACGT\nacgt\nAC\n>r3\nTTTT\nTT\n", b"")


def test_file_without_a_final_line_feed():
    fq = b"@a\nAC\n+\nII\n@b\nGT\n+\nJJ"
    assert un_plain.records(fq, False) == [b"@a\nAC\n+\nII\n", b"@b\nGT\n+\nJJ\n"]
    assert un_plain.expected([fq], sam(("a", 0), ("b", 4)), False, False) == (b"@b\nGT\n+\nJJ\n", b"")
    fa = b">a\nAC\n>b\nGT\nG"
    assert un_plain.expected([fa], sam(("a", 4), ("b", 4)), False, False, fasta=True) == (b">a\nAC\n>b\nGT\nG\n", b"")


def test_plus_name_line_comment_lower_case_and_cr_stay():
    fq = b"@r1 1:N:0\tx\nacgt\r\n+r1 1:N:0\nIIII\r\n@r2/1\nAC\n+\n@@\n"
    assert [un_plain.name_of(r) for r in un_plain.records(fq, False)] == [b"r1", b"r2"]
    assert un_plain.expected([fq], sam(("r1", 4), ("r2", 4)), False, False) == (fq, b"")
    assert un_plain.expected([fq], sam(("r1", 4), ("r2", 16)), False, False) == (b"@r1 1:N:0\tx\nacgt\r\n+r1 1:N:0\nIIII\r\n", b"")


def test_pair_with_one_mapped_mate_is_not_written():
    f1 = b"@p1/1\nAA\n+\nII\n@p2/1\nCC\n+\nII\n@p3/1\nGG\n+\nII\n"
    f2 = b"@p1/2\nTT\n+\nJJ\n@p2/2\nGG\n+\nJJ\n@p3/2\nCC\n+\nJJ\n"
    text = sam(("p1", 77), ("p1", 141), ("p2", 73), ("p2", 133), ("p3", 99), ("p3", 147))
    assert un_plain.unmapped_reads([b"p1", b"p1", b"p2", b"p2", b"p3", b"p3"], text, True) == [True, True, False, True, False, False]
    assert un_plain.expected([f1, f2], text, True, True) == (b"@p1/1\nAA\n+\nII\n", b"@p1/2\nTT\n+\nJJ\n")
    # interleaved: the two records of a pair follow each other in the one file
    inter = b"".join(a + b for a, b in zip(un_plain.records(f1, False), un_plain.records(f2, False)))
    assert un_plain.expected([inter], text, True, False) == (b"@p1/1\nAA\n+\nII\n@p1/2\nTT\n+\nJJ\n", b"")


def test_multi_hit_read_with_any_mapped_record_is_mapped():
    fq = b"@m\nAC\n+\nII\n@u\nGT\n+\nII\n"
    assert un_plain.expected([fq], sam(("m", 0), ("m", 16), ("m", 0), ("u", 4)), False, False) == (b"@u\nGT\n+\nII\n", b"")
