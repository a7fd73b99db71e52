// host/detail/chunk_stages.inc -- the two host stages of a chunk around its gap-closing call: stage A (chaining results in, pairing, rescue, filters, report pass 1:
// src/Mapping.cpp:542-563, src/AlignmentCandidates.cpp:624-745), run_nw (the chunk's nw_alignment jobs as one batched call), stage C (report pass 2, final pair check,
// flags, MAPQ, SAM text: src/Mapping.cpp:564-600) -- for the reads the device handed back, or for every read when the backend has no report stage.
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
int est_distance(const Ctx &cx, int64_t iPaired, int64_t iDistance)  // src/Mapping.cpp:534-539
{
	if (iPaired < 1000) return cx.opt.max_insert;
	int est = (int)(iDistance / (iPaired >> 2));
	return est + (est >> 1);
}

// KART_AMD_VERBOSE: thread-seconds per section of the two chunk stages (summed over all workers)
std::atomic<int64_t> g_sec_ns[6];
const char *const g_sec_name[6] = {"unpack candidates", "pair+rescue+filters", "report plan", "report finish", "pair check+flags+mapq", "sam text"};
bool g_sections = false;
struct Section {
	int id;
	timespec t0;
	explicit Section(int i) : id(i) { if (g_sections) clock_gettime(CLOCK_MONOTONIC, &t0); }
	~Section()
	{
		if (!g_sections) return;
		timespec t1;
		clock_gettime(CLOCK_MONOTONIC, &t1);
		g_sec_ns[id] += (int64_t)(t1.tv_sec - t0.tv_sec) * 1000000000 + (t1.tv_nsec - t0.tv_nsec);
	}
};

// stage A: chaining, pairing, rescue, filters, report pass 1 (collects the chunk's NW jobs) -- for the reads in ck.hq
void chunk_stage_a(const Ctx &cx, std::vector<Read> &reads, const int64_t *cand_off, const kg_candidate *dev_cands, const kg_seed *cand_seeds, ChunkState &ck, int est)
{
	ck.est_used = est;
	ck.ps = PairStats();
	ck.st = Stats();
	const size_t nh = ck.hq.size();
	ck.n_host = (int)nh;
	if (ck.recs && !g_check_align) {
		// the share of the reads decided on the device: what Output{Paired,Singled}Alignments would have counted for them, and
		// the interval of estimates for which their pairing holds (their records were made under the same `est`)
		if (ck.force.empty()) {
			ck.st.unmapped = ck.dev.unmapped; ck.st.unique = ck.dev.unique;
			ck.ps.paired = ck.dev.paired; ck.ps.distance = ck.dev.distance;
			ck.ps.lo = ck.dev.lo; ck.ps.hi = ck.dev.hi;
			ck.ps.rescue_used = ck.dev.rescue_wanted != 0;
		} else {
			// some pairs of the chunk are being mapped again: the chunk's statistics are those of the records that stand
			for (int q = 0; q < ck.count; ++q) {
				if (ck.host_read(q)) continue;
				const kg_aln_record &rec = ck.recs[ck.begin + q];
				if (rec.score == 0) ck.st.unmapped++;
				else if (rec.mapq == 60) ck.st.unique++;
				if (!ck.paired || (q & 1)) continue;
				if (rec.est_lo > ck.ps.lo) ck.ps.lo = rec.est_lo;
				if (rec.est_hi != INT32_MAX && rec.est_hi < ck.ps.hi) ck.ps.hi = rec.est_hi;
				if (rec.rescue) ck.ps.rescue_used = true;
				if (rec.kind == KG_ALN_MAPPED && rec.has_mate && rec.primary) {    // src/Mapping.cpp:209-213 (i == iBestAlnCanIdx)
					ck.ps.paired += 2;
					int ad = rec.tlen < 0 ? -rec.tlen : rec.tlen;
					if (ad < 10000) ck.ps.distance += ad;
				}
			}
		}
	}
	if (ck.paired) {
		ck.pair_lo.assign((size_t)ck.count / 2, -1); ck.pair_hi.assign((size_t)ck.count / 2, INT32_MAX); ck.pair_rescue.assign((size_t)ck.count / 2, 0);
	}
	ck.cands.assign(nh, std::vector<Candidate>());
	ck.work.assign(nh, std::vector<CandWork>());
	ck.jobs.clear();
	ck.frags.clear();
	{ Section sec(0);
	for (size_t k = 0; k < nh; ++k) {
		size_t ri = (size_t)(ck.begin + ck.hq[k]);
		// the candidates were chained on the device (kg_candidates_batch); unpack them into the per-read vectors
		std::vector<Candidate> &out = ck.cands[k];
		const int nc = (int)(cand_off[ri + 1] - cand_off[ri]);
		out.resize((size_t)nc);
		for (int c = 0; c < nc; ++c) {
			const kg_candidate &d = dev_cands[(size_t)cand_off[ri] + (size_t)c];
			Candidate &o = out[(size_t)c];
			o.score = d.score;
			o.posDiff = d.posDiff;
			o.pairs.reserve((size_t)d.count * 2 + 3);     // room for the gap pairs identify_normal_pairs adds later
			o.pairs.resize((size_t)d.count);
			for (int j = 0; j < d.count; ++j) o.pairs[(size_t)j] = from_seed(cand_seeds[(size_t)d.first + (size_t)j]);
		}
	}
	}
	{ Section sec(1);
	if (ck.paired) {
		for (size_t k = 0; k + 1 < nh; k += 2) {
			const int q = ck.hq[k];
			std::vector<Candidate> &v1 = ck.cands[k], &v2 = ck.cands[k + 1];
			Read &r1 = ck.read_at(reads, k), &r2 = ck.read_at(reads, k + 1);
			PairStats pp;
			bool pairing = pair_candidates(cx, est, v1, v2, pp);
			if (!pairing) pp.rescue_used = true;
			ck.pair_lo[(size_t)q >> 1] = (int32_t)pp.lo; ck.pair_hi[(size_t)q >> 1] = pp.hi > INT32_MAX ? INT32_MAX : (int32_t)pp.hi; ck.pair_rescue[(size_t)q >> 1] = pp.rescue_used;
			if (pp.lo > ck.ps.lo) ck.ps.lo = pp.lo;
			if (pp.hi < ck.ps.hi) ck.ps.hi = pp.hi;
			if (!pairing) {
				ck.ps.rescue_used = true;
				pairing = rescue_unpaired(cx, est, r1, r2, v1, v2);
			}
			if (pairing) remove_unmated(v1, v2);
			remove_redundant(cx, v1);
			remove_redundant(cx, v2);
		}
	} else {
		for (size_t k = 0; k < nh; ++k) remove_redundant(cx, ck.cands[k]);
	}
	}
	Section sec(2);
	// the plan compares read fragments with the reference at the candidates' positions -- random addresses in 6.2 GB for
	// hg38: ask for the lines of the reads a few places ahead while this one is being planned
	auto prefetch_ref = [&](size_t k) {
		if (k >= nh) return;
		for (const Candidate &c : ck.cands[k])
			for (const Pair &p : c.pairs) {
				__builtin_prefetch(cx.refseq() + p.gPos);
				__builtin_prefetch(cx.refseq() + p.gPos + p.gLen + 64);
			}
	};
	for (size_t k = 0; k < 6 && k < nh; ++k) prefetch_ref(k);
	for (size_t k = 0; k < nh; ++k) {
		prefetch_ref(k + 6);
		report_plan(cx, ck.read_at(reads, k), ck.cands[k], ck.work[k], ck.jobs, cx.frag_service ? &ck.frags : nullptr);
	}
}

// -un / -un2: the input text of the chunk's unmapped units (a read; with -p / -f2 a pair, both mates unmapped), per input file, from the flags stage C has
// just set.  A read the host mapped is unmapped when it printed the unmapped record (score 0: FLAG & 4, set_single_flag / set_one_mate_flags); one the
// device decided when its record is that one.  A chunk of the device stream holds the units in hq alone: the device hands the others' bytes back itself
void chunk_unmapped(const Ctx &cx, std::vector<Read> &reads, ChunkState &ck)
{
	for (int f = 0; f < 2; ++f) { ck.un_text[f].clear(); ck.un_host_len[f].clear(); }
	// (pairs wherever the run is paired and the chunk holds whole pairs -- also where -pacbio maps the mates one by one, chunk_stage_c)
	const bool pairs = cx.opt.paired && ck.count % 2 == 0;
	const int step = pairs ? 2 : 1;
	const bool two_files = cx.un_out[1] != nullptr;
	size_t k = 0;
	for (int q = 0; q + step <= ck.count; q += step) {
		const bool host = k < ck.hq.size() && ck.hq[k] == q;
		if (!host && ck.stream) continue;
		bool take = true;
		const Read *rd[2] = {nullptr, nullptr};
		for (int t = 0; t < step; ++t) {
			if (host) {
				rd[t] = &ck.read_at(reads, k + (size_t)t);
				take = take && rd[t]->score == 0;
			} else {
				rd[t] = &reads[(size_t)(ck.begin + q + t)];
				const kg_aln_record &rec = ck.recs[ck.begin + q + t];
				take = take && rec.kind == KG_ALN_UNMAPPED && (rec.flag & 4) != 0;
			}
		}
		if (host) k += (size_t)step;
		size_t added[2] = {0, 0};
		for (int t = 0; take && t < step; ++t) {
			const int f = two_files ? (q + t) & 1 : 0;             // (GetNextChunk: a chunk's even reads come from the first file, its odd ones from the second)
			std::string &out = ck.un_text[f];
			const size_t before = out.size();
			out += rd[t]->raw;
			if (out.size() > before && out.back() != '\n') out += '\n';       // (the file's last line came without its line feed)
			added[f] += out.size() - before;
		}
		if (ck.stream)
			for (int f = 0; f < (two_files ? 2 : 1); ++f) ck.un_host_len[f].push_back((uint32_t)added[f]);
	}
}

// -stats: the device's share of a stream chunk's tally (the host's own reads, ck.hq, are counted where they are printed).  The rule of stage A's first lines:
// nothing of the chunk is mapped again -- the device's row as it is (it leaves out the reads handed back); otherwise a recount of the records that stand,
// each with the records chained behind it (-m), so that a chunk mapped again counts once, under its final records
void chunk_device_tally(ChunkState &ck)
{
	if (!ck.tally || !ck.stream || !ck.recs) return;
	if (ck.force.empty()) {
		if (ck.dev_tally) ck.tally->add_row(ck.dev_tally);
		return;
	}
	const int64_t n_reads = ck.n_records_reads;
	for (int q = 0; q < ck.count; ++q) {
		if (!ck.dev_read(q)) continue;
		int64_t at = ck.begin + q;
		for (int64_t step = 0; step <= ck.n_records - n_reads; ++step) {
			ck.tally->add(ck.recs[at]);
			const int64_t next = ck.recs[at].next;
			if (next < n_reads || next >= ck.n_records) break;
			at = next;
		}
	}
}

// stage C: report pass 2, final pair check, flags, MAPQ, SAM text
void chunk_stage_c(const Ctx &cx, std::vector<Read> &reads, ChunkState &ck)
{
	const size_t nh = ck.hq.size();
	if (cx.stats) {
		if (!ck.tally) ck.tally = std::make_shared<Tally>();
		ck.tally->clear();
	}
	TallyInto tally_into(cx.stats ? ck.tally.get() : nullptr);
	{ Section sec(3);
	// pass 2 reads the text at the fragment pairs' positions again (random addresses in 6.2 GB for hg38, long after the plan touched
	// them): ask for the first lines of the pairs of the read two places ahead
	auto prefetch_frags = [&](size_t k) {
		if (k >= nh || ck.frags.size() == 0) return;
		for (const CandWork &cw : ck.work[k])
			for (const PairWork &w : cw.pairs)
				if (w.frag >= 0) {
					__builtin_prefetch(cx.refseq() + ck.frags.g[(size_t)w.frag]);
					__builtin_prefetch(cx.refseq() + ck.frags.g[(size_t)w.frag] + 64);
				}
	};
	prefetch_frags(0); prefetch_frags(1);
	for (size_t k = 0; k < nh; ++k) {
		prefetch_frags(k + 2);
		bool first = ck.paired ? (ck.hq[k] % 2 == 0) : true;
		report_finish(cx, first, ck.read_at(reads, k), ck.cands[k], ck.work[k], ck.jobs, ck.frags);
	}
	}
	ck.text.clear();
	ck.host_len.clear();
	if (!ck.stream) {
		// room for the chunk's records up front: name, bases, qualities and the fixed columns of every read (+ half the bases again
		// for a long read's CIGAR) -- a 4000-read chunk of 7 kb reads is 59 MB of text; growing to that by doubling copied it all once more
		size_t need = 0;
		for (int q = 0; q < ck.count; ++q) {
			const Read &r = reads[(size_t)(ck.begin + q)];
			need += r.name.size() + r.seq.size() + r.qual.size() + 160 + (cx.opt.pacbio ? r.seq.size() / 2 : 0);
		}
		ck.text.reserve(std::max(need, (size_t)ck.count * 400));
	}
	if (ck.paired) {
		{ Section sec(4);
		for (size_t k = 0; k + 1 < nh; k += 2) {
			Read &r1 = ck.read_at(reads, k), &r2 = ck.read_at(reads, k + 1);
			check_final_pair(cx, r1, r2);
			set_paired_flags(r1, r2);
			evaluate_mapq(cx, r1);
			evaluate_mapq(cx, r2);
		}
		}
		Section sec(5);
		size_t k = 0;
		for (int q = 0; q < ck.count; q += 2) {
			if (k < nh && ck.hq[k] == q) {
				size_t from = ck.text.size();
				output_pair(cx, ck.read_at(reads, k), ck.read_at(reads, k + 1), ck.st, ck.ps, ck.text);
				if (g_check_align && ck.dev_read(q)) check_record_text(cx, ck, reads, q, 2, from);
				if (ck.stream) ck.host_len.push_back((uint32_t)(ck.text.size() - from));
				k += 2;
				if (ck.stream && k >= nh) break;            // (the device printed the rest)
			} else if (!ck.stream) {
				sam_from_record(cx, reads[(size_t)(ck.begin + q)], ck.recs, ck.begin + q, ck.text);
				sam_from_record(cx, reads[(size_t)(ck.begin + q + 1)], ck.recs, ck.begin + q + 1, ck.text);
			} else if (nh == 0) break;
		}
	} else {
		for (size_t k = 0; k < nh; ++k) {
			Read &rd = ck.read_at(reads, k);
			set_single_flag(rd);
			evaluate_mapq(cx, rd);
		}
		Section sec(5);
		size_t k = 0;
		if (cx.opt.paired && ck.count % 2 == 0 && cx.opt.pacbio && nh == (size_t)ck.count && !ck.stream) {
			// -pacbio with mate files: the reads are mapped one by one (src/Mapping.cpp:514-529 comes first) but printed by
			// OutputPairedAlignments (:598 asks only for bPairEnd and an even count) -- mate 2, held reverse-complemented, is shown
			// flipped back by a forward report, and no report has a mate
			for (; k + 1 < nh; k += 2) output_pair(cx, ck.read_at(reads, k), ck.read_at(reads, k + 1), ck.st, ck.ps, ck.text);
		}
		for (int q = (int)k; q < ck.count; ++q) {
			if (k < nh && ck.hq[k] == q) {
				size_t from = ck.text.size();
				output_single(cx, ck.read_at(reads, k), ck.st, ck.text);
				if (g_check_align && ck.dev_read(q)) check_record_text(cx, ck, reads, q, 1, from);
				if (ck.stream) ck.host_len.push_back((uint32_t)(ck.text.size() - from));
				k++;
				if (ck.stream && k >= nh) break;
			} else if (!ck.stream) sam_from_record(cx, reads[(size_t)(ck.begin + q)], ck.recs, ck.begin + q, ck.text, ck.cigar_pool);
			else if (nh == 0) break;
		}
	}
	// -bo: the chunk's text becomes its compressed BAM records here; a chunk of the device stream holds only the host's own lines, which become
	// raw records -- the device's records around them are joined and compressed once the chunk is committed (stream.inc, BamPacker)
	if (cx.opt.bam && ck.stream) bam_raw_pieces(cx, ck.text, ck.host_len);
	else if (cx.opt.bam) bam_encode_chunk(cx, ck.text);
	ck.text_size = ck.text.size();
	ck.st.total_reads = ck.count;
	if (cx.un()) chunk_unmapped(cx, reads, ck);
	if (cx.stats) chunk_device_tally(ck);
	ck.cands.clear(); ck.work.clear();
	// the reports are spent once the text exists: release them here, on the worker that allocated them, instead of in the
	// batch destructor on the main thread (400 k small frees per batch, serial)
	for (size_t k = 0; k < nh; ++k) std::vector<Report>().swap(ck.read_at(reads, k).rep);
}

// one NW kernel call for the jobs of many chunks
std::atomic<int64_t> g_frag_total{0}, g_frag_back{0};     // KART_AMD_VERBOSE: fragment pairs sent to the device / planned here after all
void run_nw(const Ctx &cx, std::vector<ChunkState> &chunks, size_t from, size_t to)
{
	// first the fragment pairs the device plans itself (-pacbio: partition, recursion, alignment of the pieces in one call); a pair
	// outside the kernels' envelope is planned here after all, its alignments joining the chunk's other NW jobs below
	{
		std::vector<FragJobs *> fparts;
		for (size_t c = from; c < to; ++c)
			if (chunks[c].frags.size() > 0) fparts.push_back(&chunks[c].frags);
		if (!fparts.empty()) {
			const bool served = cx.kern.fragments_batch(fparts, cx.opt.pacbio, cx.opt.max_gaps);
			for (size_t c = from; c < to; ++c) {
				ChunkState &ck = chunks[c];
				for (size_t j = 0; j < ck.frags.size(); ++j) {
					g_frag_total++;
					if (served && !ck.frags.status[j]) continue;
					g_frag_back++;
					PairWork &w = *static_cast<PairWork *>(ck.frags.owner[j]);
					w.frag = -1;
					plan_alignment(cx, (int)(ck.frags.o1[j + 1] - ck.frags.o1[j]), ck.frags.f1.data() + ck.frags.o1[j], ck.frags.gl[j], cx.refseq() + ck.frags.g[j], w.plan, ck.jobs);
				}
			}
		}
	}
	std::vector<NwJobs *> parts;
	for (size_t c = from; c < to; ++c)
		if (chunks[c].jobs.size() > 0) parts.push_back(&chunks[c].jobs);
	if (!parts.empty()) cx.kern.nw_batch(parts);
}
