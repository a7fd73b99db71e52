// host/detail/chunk_state.inc -- a chunk's state through the pipeline (ChunkState), the check mode's comparison, the worker Pool; and why chunks are mapped under a speculated EstDistance.
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
// ----------------------------------------------------------------------------------------------
// one library: batches of chunks (ReadMapping, src/Mapping.cpp:488-637)
// ----------------------------------------------------------------------------------------------
// The reference is only deterministic at -t 1, where chunk k sees EstDistance computed from the final
// alignments of chunks < k (:533-540).  To run chunks concurrently and still write exactly that output,
// every chunk is mapped with a SPECULATED EstDistance (the latest committed value) and records the
// interval of values for which its decisions hold; a commit step walks the chunks in input order,
// derives the true value from the committed totals and re-runs the (rare) chunk that falls outside.
bool g_check_align = false;

struct ChunkState {
	int begin = 0, count = 0;
	bool paired = false;
	int est_used = 0;
	PairStats ps;
	Stats st;
	std::vector<std::vector<Candidate>> cands;
	std::vector<std::vector<CandWork>> work;
	NwJobs jobs;
	FragJobs frags;                                  // -pacbio: the fragment pairs whose alignment the device plans and computes (kg_fragments_batch)
	std::string text;
	// the device's per-read records for this chunk's reads (indexed like `reads`), or null: every read is mapped here.  A read
	// whose record is not KG_ALN_HOST only needs its SAM text; dev = the chunk's statistics from the device
	const kg_aln_record *recs = nullptr;
	const char *cigar_pool = nullptr;                // long reads: the CIGAR strings of the batch's records (kg_longread_batch)
	kg_chunk_stats dev{};
	// per pair (index q / 2): the EstDistance interval for which the pair's own decisions hold, and whether rescue was due --
	// so that a chunk whose speculated estimate did not hold re-maps only the pairs it matters for (force[q] set)
	std::vector<int32_t> pair_lo, pair_hi;
	std::vector<uint8_t> pair_rescue, force;
	int n_host = 0;                                  // reads of the chunk mapped by the host stages
	// The reads (index in the chunk, ascending; the two reads of a pair stay together) that the host stages map: everything when
	// there is no device report, else the pairs handed back (KG_ALN_HOST) and the ones forced by a failed speculation.  The
	// per-read vectors below (cands, work) and own_reads are indexed by the position in this list.
	std::vector<int> hq;
	// stream path (stream.inc): the device printed the text of the reads it decided; `text` holds only the lines of the reads in
	// hq (host_len: bytes per pair / read, in hq order), and those reads are materialised here from the input text
	bool stream = false;
	std::vector<uint32_t> host_len;
	std::vector<Read> own_reads;
	std::string own_chars;                           // storage behind own_reads' reverse-complemented mates
	size_t text_size = 0;                            // bytes of the whole chunk's text
	// -un / -un2 (chunk_unmapped): the unmapped units' input text per input file -- of the whole chunk, or (stream) of the units in hq alone, un_host_len
	// bytes per such unit in hq order (0: the unit is not selected)
	std::string un_text[2];
	std::vector<uint32_t> un_host_len[2];
	// -stats (null otherwise): the tally of the records the chunk prints -- what the host printed (the printer's record sites, sam.inc) plus, for a chunk of
	// the device stream, the device's share (chunk_device_tally): its row dev_tally when every record of it stands, else a recount of those that do
	std::shared_ptr<Tally> tally;
	const uint32_t *dev_tally = nullptr;             // the chunk's row of kg_stream_result::chunk_tally
	int64_t n_records_reads = 0, n_records = 0;      // ... and the reads and records of its batch (the -m chains lie in [reads, records))
	bool host_read(int q) const { return g_check_align || !recs || recs[begin + q].kind == KG_ALN_HOST || (!force.empty() && force[(size_t)q]); }
	bool dev_read(int q) const { return recs && recs[begin + q].kind != KG_ALN_HOST && (force.empty() || !force[(size_t)q]); }   // its record stands
	void list_host_reads()
	{
		hq.clear();
		for (int q = 0; q < count; ++q)
			if (host_read(q)) hq.push_back(q);
	}
	Read &read_at(std::vector<Read> &reads, size_t k) const { return own_reads.empty() ? reads[(size_t)(begin + hq[k])] : const_cast<Read &>(own_reads[k]); }
	// the pairs of a device-aligned chunk that must be mapped again because `est_true` falls outside their own interval
	void force_invalid_pairs(int est_true, int max_insert)
	{
		if (!recs || !paired) return;
		force.resize((size_t)count, 0);
		for (int q = 0; q + 1 < count; q += 2) {
			int64_t lo, hi;
			bool resc;
			if (host_read(q)) { lo = pair_lo[(size_t)q >> 1]; hi = pair_hi[(size_t)q >> 1]; resc = pair_rescue[(size_t)q >> 1] != 0; }
			else { const kg_aln_record &a = recs[begin + q]; lo = a.est_lo; hi = a.est_hi; resc = a.rescue != 0; }
			bool ok = lo < est_true && (hi == INT32_MAX || est_true <= hi) && (!resc || std::min(est_true, max_insert) == std::min(est_used, max_insert));
			if (!ok) force[(size_t)q] = force[(size_t)q + 1] = 1;
		}
	}
};

// KART_AMD_CHECK_ALIGN: every read is mapped on the host as well, and the text of the device's record is compared with it
std::atomic<int64_t> g_check_bad{0}, g_check_n{0};
void check_record_text(const Ctx &cx, const ChunkState &ck, const std::vector<Read> &reads, int q, int n, size_t text_from)
{
	std::string want;
	TallyInto nowhere(nullptr);                      // (a text made for comparison: not a record of the output)
	for (int t = 0; t < n; ++t) sam_from_record(cx, reads[(size_t)(ck.begin + q + t)], ck.recs, ck.begin + q + t, want, ck.cigar_pool);
	g_check_n += n;
	if (want.size() == ck.text.size() - text_from && memcmp(want.data(), ck.text.data() + text_from, want.size()) == 0) return;
	if (g_check_bad++ < 30) fprintf(stderr, "CHECK_ALIGN mismatch (est %d):\n  host  : %s  device: %s", ck.est_used, ck.text.substr(text_from).c_str(), want.c_str());
}

// persistent worker pool: stage after stage reuses the same threads (and their malloc arenas)
class Pool {
public:
	// nice_level > 0: the pool's own threads run at that niceness (the bulk workers yield the cores to the stages on the
	// critical path -- reader, device thread, writers -- when the thread budget exceeds the CPU quota)
	explicit Pool(int n, int nice_level = 0) : n_(std::max(1, n))
	{
		for (int t = 1; t < n_; ++t) workers_.emplace_back([this, t, nice_level]() {
			if (nice_level > 0) setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), nice_level);
			loop(t);
		});
	}
	~Pool()
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			stop_ = true;
		}
		cv_.notify_all();
		for (std::thread &th : workers_) th.join();
	}
	int size() const { return n_; }
	// two item sets in one parallel phase, both with the item -> worker (i mod n) mapping
	void run2(int n_a, const std::function<void(int)> &fa, int n_b, const std::function<void(int)> &fb)
	{
		int n = std::max(n_a, n_b);
		run(n, [&](int i) {
			if (i < n_a) fa(i);
			if (i < n_b) fb(i);
		});
	}
	// the same two sets, but every worker first does ALL its items of the first set, then calls `between` (which may
	// block), then does its items of the second set
	void run_ordered(int n_first, const std::function<void(int)> &f_first, const std::function<void()> &between, int n_second,
	                 const std::function<void(int)> &f_second)
	{
		if (n_first <= 0 && n_second <= 0) return;
		run(n_, [&](int w) {
			for (int i = w; i < n_first; i += n_) f_first(i);
			between();
			for (int i = w; i < n_second; i += n_) f_second(i);
		});
	}
	void run(int n_items, const std::function<void(int)> &fn)
	{
		if (n_items <= 0) return;
		if (n_ == 1 || n_items == 1) {
			for (int i = 0; i < n_items; ++i) fn(i);
			return;
		}
		{
			std::lock_guard<std::mutex> lk(mu_);
			fn_ = &fn; items_ = n_items; pending_ = n_ - 1; gen_++;
		}
		cv_.notify_all();
		// static assignment (item i -> worker i mod n): the chunk a worker built in one stage is the chunk it
		// finishes and frees in the next, so allocations never cross threads
		for (int i = 0; i < n_items; i += n_) fn(i);
		std::unique_lock<std::mutex> lk(mu_);
		done_cv_.wait(lk, [this]() { return pending_ == 0; });
		fn_ = nullptr;
	}

private:
	void loop(int me)
	{
		uint64_t seen = 0;
		for (;;) {
			const std::function<void(int)> *fn;
			int items;
			{
				std::unique_lock<std::mutex> lk(mu_);
				cv_.wait(lk, [&]() { return stop_ || gen_ != seen; });
				if (stop_) return;
				seen = gen_;
				fn = fn_; items = items_;
			}
			for (int i = me; i < items; i += n_) (*fn)(i);
			{
				std::lock_guard<std::mutex> lk(mu_);
				if (--pending_ == 0) done_cv_.notify_one();
			}
		}
	}
	int n_;
	std::vector<std::thread> workers_;
	std::mutex mu_;
	std::condition_variable cv_, done_cv_;
	const std::function<void(int)> *fn_ = nullptr;
	int items_ = 0, pending_ = 0;
	uint64_t gen_ = 0;
	bool stop_ = false;
};
