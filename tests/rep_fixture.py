"""The repeat-family fixture (tests/golden/rep.fa.gz, tests/golden/sam/rep_*; written by oracle/make_golden_rep.py) as the tests and its
generator read it: the index built from the committed genome, the reads as the mapper holds them (mate 2 reverse-complemented), their
seeds and candidates from the CPU oracle, the pairing test of the reference restated on (score, PosDiff) lists, and the columns of the
reference's SAM lines per read."""
import gzip
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")          # (as conftest.GOLDEN; the generator imports this module without pytest)
SAM = os.path.join(GOLDEN, "sam")
REP_FA = os.path.join(GOLDEN, "rep.fa.gz")
EST_DISTANCE = 1500          # MaxInsertSize: what a run's first chunk is paired under (src/Mapping.cpp:534-539)


def gunzip_to(src, dst):
    with gzip.open(src) as fi, open(dst, "wb") as fo:
        fo.write(fi.read())
    return dst


def build_rep_index(tmp, device="cpu"):
    """<tmp>/rep.{bwt,sa,pac,ann,amb} from the committed genome (kart_amd.index_build is held to the reference's bwt_index byte for
    byte by tests/test_index_build.py); returns the prefix"""
    from kart_amd import index_build
    fa = gunzip_to(REP_FA, os.path.join(tmp, "rep.fa"))
    prefix = os.path.join(tmp, "rep")
    index_build.build_index(fa, prefix, device=device)
    return prefix


def read_fastq_gz(path):
    lines = gzip.open(path).read().split(b"\n")
    n = len(lines) // 4
    return [lines[4 * i][1:].split(b"\t")[0] for i in range(n)], [lines[4 * i + 1] for i in range(n)]


def held_reads(seqs1, seqs2):
    """the chunk as ReadMapping() holds it: read 2q = mate 1, read 2q + 1 = mate 2 reverse-complemented (src/GetData.cpp:125-135); ASCII arrays"""
    from kart_amd import synth
    out = []
    for a, b in zip(seqs1, seqs2):
        out.append(np.frombuffer(a, np.uint8))
        out.append(synth.revcomp(np.frombuffer(b, np.uint8)))
    return out


def load_reads():
    names, s1 = read_fastq_gz(os.path.join(SAM, "rep_1.fq.gz"))
    _, s2 = read_fastq_gz(os.path.join(SAM, "rep_2.fq.gz"))
    return names, held_reads(s1, s2)


def oracle_chain(orc, reads, max_gaps=5):
    """(seed_offsets, seeds, [candidates per read]) of the held reads from the CPU oracle: IdentifySeedPairs_FastMode + GenerateAlignmentCandidateForIlluminaSeq"""
    from kart_amd import api, synth
    enc, off = api.concat_reads([synth.encode(r) for r in reads])
    so, seeds = orc.seed_batch(enc, off, 0)
    cands = [orc.candidates(len(reads[i]), seeds[so[i]:so[i + 1]], False, max_gaps) for i in range(len(reads))]
    return so, seeds, cands


def _remove_redundant(scores):
    """RemoveRedundantCandidates, src/Mapping.cpp:317-346 (not -pacbio)"""
    if len(scores) <= 1:
        return scores
    s1 = s2 = 0
    for s in scores:
        if s > s2:
            if s >= s1:
                s2, s1 = s1, s
            else:
                s2 = s
    thr = s1 if (s1 == s2 or s1 - s2 > 20) else s2
    return [0 if s < thr else s for s in scores]


def chained_lists_pair(c1, c2, est=EST_DISTANCE):
    """bPairing of CheckPairedAlignmentCandidates (src/Mapping.cpp:348-400) on two candidate lists of (score, PosDiff, ...): does any
    candidate of mate 1 find a single best candidate of mate 2 within `est` behind it"""
    sc1, sc2 = [c[0] for c in c1], [c[0] for c in c2]
    if len(c1) * len(c2) > 1000:
        sc1, sc2 = _remove_redundant(sc1), _remove_redundant(sc2)
    for i, a in enumerate(c1):
        if sc1[i] == 0:
            continue
        best, s = -1, 0
        for j, b in enumerate(c2):
            if sc2[j] == 0 or b[1] < a[1]:
                continue
            if b[1] - a[1] < est:
                if sc2[j] > s:
                    best, s = j, sc2[j]
                elif sc2[j] == s:
                    best = -1
        if s > 0 and best != -1:
            return True
    return False


def sam_records(text, never=()):
    """the records of a SAM text by read: {(name, mate 0 / 1): [(line number, fields)] in print order} (mate: the FLAG's 0x40 / 0x80).  A line
    in `never` (its FLAG is heap contents) is never a read's first record -- the print loop starts at iBestAlnCanIdx, whose FLAG is assigned
    (src/Mapping.cpp:177-270) -- and belongs to the read of the line before it"""
    out, last = {}, None
    for ln, line in enumerate(text.split(b"\n")):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        key = last if ln in never else (f[0], 1 if int(f[1]) & 0x80 else 0)
        out.setdefault(key, []).append((ln, f))
        last = key
    return out


def load_sam(name):
    return gzip.open(os.path.join(SAM, name + ".sam.gz")).read()


def never_assigned_lines():
    """the lines of rep_m.sam.gz whose FLAG the reference never assigns (they differ between its two MALLOC_PERTURB_ runs)"""
    return {int(x) for x in open(os.path.join(SAM, "rep_m.never_assigned_flags.txt")).read().split()}
