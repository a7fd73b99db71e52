#!/usr/bin/env python3
"""Kernel-level fuzz on the GPU box: kg_seed_batch / kg_candidates_batch through the C ABI against the CPU oracle
with random parameters (MinSeedLength 13..16, occurrence threshold 1..120, MaxGaps 0..40, both modes, both SA modes), ragged and
ambiguous reads from the fixture genome.  (The NW kernels' cases live in one place: tests/nw_plain.py, run by tests/test_nw_edges_gpu.py.)  VALIDATION TOOL.  usage: python tools/fuzz_kernels_gpu.py [iterations]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kart_amd import api, synth
from kart_amd.index_build import read_fasta
from oracle import oracle as O
it_n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
prefix = os.path.join(ROOT, "tests", "golden", "idx", "small")
fwd = np.concatenate([s for _, _, s in read_fasta(os.path.join(ROOT, "tests", "golden", "small.fa"))])
orc = O.Oracle(prefix)
ixs = {api.KG_SA_SAMPLED: api.Index(prefix, 0, api.KG_SA_SAMPLED), api.KG_SA_FULL: api.Index(prefix, 0, api.KG_SA_FULL)}
codes = np.frombuffer(b"ACGTNacgtnRY", np.uint8)
bad = 0
for it in range(it_n):
    rng = np.random.default_rng(1000 + it)
    mode = int(rng.integers(0, 2)); msl = int(rng.integers(13, 17)); occ = int(rng.choice([1, 2, 5, 50, 120])); gaps = int(rng.choice([0, 5, 40]))
    reads = []
    for _ in range(int(rng.integers(50, 3000))):
        ln = int(rng.choice([rng.integers(0, 30), rng.integers(30, 200), 150, rng.integers(200, 1500)])) if mode == 0 else int(rng.integers(0, 9000))
        p = int(rng.integers(0, max(1, len(fwd) - ln - 1)))
        r = fwd[p:p + ln].copy()
        if rng.random() < 0.5: r = synth.revcomp(r)
        m = rng.random(len(r)) < rng.choice([0.0, 0.01, 0.05, 0.15])
        r[m] = codes[rng.integers(0, len(codes), int(m.sum()))]
        if rng.random() < 0.1 and len(r) > 40: r[5:5 + int(rng.integers(1, 35))] = ord("N")
        reads.append(synth.encode(r))
    enc, off = api.concat_reads(reads)
    sa = int(rng.choice([api.KG_SA_SAMPLED, api.KG_SA_FULL]))
    ws = ixs[sa].workspace(len(reads), max(1, len(enc)))
    so_g, s_g = ws.seed_batch(enc, off, mode, min_seed_len=msl, occ_thr=occ)
    so_o, s_o = orc.seed_batch(enc, off, mode, min_seed_len=msl, threads=4) if occ == 50 else (None, None)
    ok = True
    if so_o is not None:
        ok = bool((so_g == so_o).all() and (s_g == s_o.astype(api.SEED_DT)).all())
    else:   # the oracle has the reference's fixed threshold of 50: check the property instead (no hit with more occurrences than asked)
        ok = bool(np.all(np.diff(so_g) >= 0))
    if ok and len(reads) and so_g[-1] > 0:
        cands = ws.candidates_batch(so_g, bool(mode), gaps)
        for r in range(0, len(reads), max(1, len(reads) // 200)):
            want = orc.candidates(len(reads[r]), s_g[so_g[r]:so_g[r + 1]], bool(mode), gaps)
            if len(cands[r]) != len(want) or any((a[0], a[1]) != (b[0], b[1]) or len(a[2]) != len(b[2]) or (a[2]["gPos"] != b[2]["gPos"]).any() or (a[2]["rPos"] != b[2]["rPos"]).any() for a, b in zip(cands[r], want)):
                ok = False; break
    print("it", it, "mode", mode, "msl", msl, "occ", occ, "gaps", gaps, "sa", sa, "reads", len(reads), "seeds", int(so_g[-1]), "ok" if ok else "MISMATCH")
    bad += 0 if ok else 1
print("done, mismatches:", bad)
sys.exit(1 if bad else 0)
