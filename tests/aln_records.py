"""What a kg_aln_record shows against what the reference's SAM line shows, shared by the GPU tests that hold kg_align_batch to the reference record by
record (tests/test_rep_gpu.py, tests/test_shapes_gpu.py).  `rep` is the fixture dict of the calling module: "ix" (the api.Index), "reads" (as the mapper
holds them: mate 2 reverse-complemented), "names", "never" (lines of an -m SAM whose FLAG the reference never assigns)."""


def record_columns(rep, rec, rlen):
    """what the SAM line of a record shows, as the columns of the reference's line are compared"""
    from kart_amd import api
    if rec["kind"] == api.KG_ALN_UNMAPPED:
        return (int(rec["flag"]), b"*", 0, 0, b"*", b"*", 0, 0, 0, 0, None)
    cigar = bytes(rec["cigar"])[:int(rec["cigar_len"])]
    mate = (b"=", int(rec["mate_pos"]), int(rec["tlen"])) if rec["has_mate"] else (b"*", 0, 0)
    return (int(rec["flag"]), rep["ix"].contigs[int(rec["chr"])][0].encode(), int(rec["pos"]), int(rec["mapq"]), cigar) + mate + \
           (int(rec["score"]), int(rec["sub_score"]), rlen - int(rec["score"]))


def line_columns(f):
    tags = dict(t.split(b":i:") for t in f[11:])
    return (int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[6], int(f[7]), int(f[8]), int(tags[b"AS"]), int(tags[b"XS"]), int(tags[b"NM"]) if b"NM" in tags else None)


def chain_of(recs, k):
    """the records of read k in print order"""
    from kart_amd import api
    if recs[k]["kind"] == api.KG_ALN_NONE:
        return []
    out, at = [], k
    while at >= 0:
        out.append(recs[at])
        at = int(recs[at]["next"])
    return out


def compare_pairs_with_reference(rep, sam, pairs, recs, multi_hit):
    """every read decided on the device against its lines of the reference's SAM (`sam`: rep_fixture.sam_records of it); returns the pairs handed back"""
    from kart_amd import api, synth
    host = []
    for k, q in enumerate(pairs):
        kinds = [int(recs[2 * k + m]["kind"]) for m in (0, 1)]
        assert (kinds[0] == api.KG_ALN_HOST) == (kinds[1] == api.KG_ALN_HOST), q
        if kinds[0] == api.KG_ALN_HOST:
            host.append(q)
            continue
        for m in (0, 1):
            read = rep["reads"][2 * q + m]
            lines = sam.get((rep["names"][q], m), [])
            chain = chain_of(recs, 2 * k + m)
            assert len(chain) == len(lines), (q, m, len(chain), len(lines))
            for rec, (ln, f) in zip(chain, lines):
                got, want = record_columns(rep, rec, len(read)), line_columns(f)
                if multi_hit and ln in rep["never"]:
                    got, want = got[1:], want[1:]
                assert got == want, (q, m, ln, got, want)
                if rec["kind"] == api.KG_ALN_MAPPED:
                    assert f[9] == (synth.revcomp(read) if rec["flip"] else read).tobytes(), (q, m, ln)
    return host
