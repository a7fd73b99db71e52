// host/detail/stream.inc -- one library through the device's FASTQ-in / SAM-out (-bo: BAM-out) stream: the host only moves bytes (and deflates them).
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
// ----------------------------------------------------------------------------------------------
// The reference's worker reads a chunk with getline() (GetNextChunk, src/GetData.cpp:109-143), maps it and prints its records with
// fprintf (src/Mapping.cpp:601-622).  With the whole per-read path on the device (kg_stream_*: line index, records, mate-2 reverse
// complement, seeding .. report, SAM text) the host is left with one StreamRun per library:
//   lane threads   StreamRun::lane_batch, batch s in lane s % K, one step after the other:
//                    1 wait_lane_free     the lane's buffers are free (the batch before it in the lane is committed and written)
//                    2 claim_block        the next raw block of each input file, assigned in batch order (StreamFeed::dispatched)
//                    3 read_and_upload    pread() the block into the page-locked staging buffer, upload it
//                    4 place_window       once the batch before is parsed (StreamFeed::parsed): the unconsumed tail of the text goes in front
//                    5 parse_and_publish  the device finds the records; where they end is where the next batch's window begins
//                    6 map_or_sit_out     the device maps; the few reads it hands back (KG_ALN_HOST) go through the host stages of pipeline.inc
//                    7 hand_over          to the commit
//   commit (main)  StreamRun::commit, the in-order EstDistance commit (src/Mapping.cpp:533-540) on the chunks' device statistics: take batch s,
//                  settle_estimates (re-map the pairs of a chunk whose speculated estimate did not hold), emit_chunks, publish_commit
//   writer threads copy the text into the mapped output file (-bo: BamPacker's threads deflate it first)
// Input blocks are cut by bytes, not by records: a batch's window is the unconsumed tail of the text before it (known once the
// batch before has been parsed) followed by its own block, which was read and uploaded ahead of that.  Who waits for whom is StreamFeed's
// business alone: one mutex, one condition variable, the ordering rules written at its members.

// a pool that several threads may hand work to at once (the lane threads' host reads, the commit's re-maps)
class TaskPool {
public:
	explicit TaskPool(int n, int nice_level = 0)
	{
		for (int t = 0; t < std::max(1, n); ++t) th_.emplace_back([this, nice_level]() {
			if (nice_level > 0) setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), nice_level);
			loop();
		});
	}
	~TaskPool()
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			stop_ = true;
		}
		cv_.notify_all();
		for (std::thread &t : th_) t.join();
	}
	int size() const { return (int)th_.size(); }
	// fn(i) for every i in [0, n); the caller works along and returns when all are done
	void run(int n, const std::function<void(int)> &fn)
	{
		if (n <= 0) return;
		if (n == 1) { fn(0); return; }
		Group g;
		g.fn = &fn; g.n = n;
		std::unique_lock<std::mutex> lk(mu_);
		groups_.push_back(&g);
		cv_.notify_all();
		// (a group lives on its caller's stack: it is only touched under the lock, and not after its last item was counted)
		while (g.next < g.n) {
			int i = g.next++;
			lk.unlock();
			fn(i);
			lk.lock();
			g.done++;
		}
		g.cv.wait(lk, [&]() { return g.done == g.n; });
		groups_.erase(std::find(groups_.begin(), groups_.end(), &g));
	}

private:
	struct Group {
		const std::function<void(int)> *fn = nullptr;
		int n = 0, next = 0, done = 0;
		std::condition_variable cv;
	};
	void loop()
	{
		std::unique_lock<std::mutex> lk(mu_);
		for (;;) {
			Group *g = nullptr;
			cv_.wait(lk, [&]() {
				if (stop_) return true;
				for (Group *x : groups_)
					if (x->next < x->n) { g = x; return true; }
				return false;
			});
			if (!g) return;
			while (g->next < g->n) {
				int i = g->next++;
				const std::function<void(int)> *fn = g->fn;
				lk.unlock();
				(*fn)(i);
				lk.lock();
				if (++g->done == g->n) { g->cv.notify_all(); break; }     // (the group may be gone from here on)
			}
		}
	}
	std::mutex mu_;
	std::condition_variable cv_;
	std::vector<Group *> groups_;
	std::vector<std::thread> th_;
	bool stop_ = false;
};

// The BGZF blocks the device made of a batch's records (kg_stream_result::block_src, n_blocks + 1 ascending offsets into the records) that hold exactly
// the bytes [from, to) of them: blocks [first, last), `whole` where both ends are block boundaries.  The device cuts at every chunk's first byte and at
// the place of every read it handed back, so a piece of a chunk between two such places is whole; a piece next to a pair the commit mapped again
// under another EstDistance ends inside a block and is not.
struct BlockRange {
	int64_t first = 0, last = 0;
	bool whole = false;
};
inline BlockRange stream_piece_blocks(const int64_t *block_src, int64_t n_blocks, int64_t from, int64_t to)
{
	BlockRange r;
	if (!block_src || n_blocks <= 0 || to <= from) return r;
	const int64_t *end = block_src + n_blocks + 1;
	const int64_t *a = std::lower_bound(block_src, end, from), *b = std::lower_bound(a, end, to);
	r.first = a - block_src; r.last = b - block_src;
	r.whole = a != end && b != end && *a == from && *b == to;
	return r;
}

// -bo: the committed chunks of a run whose records the device makes as BAM (kg_stream_set_format).  A chunk's raw BAM is its pieces joined -- the
// device's records out of the lane's buffer, the host's own records (bam_raw_pieces) between them -- and is compressed as one series of BGZF blocks
// per chunk: what bam_encode_chunk makes of the same chunk's text on the host's path, so the file is the same byte for byte.  Deflate is the run's
// largest cost on the host, so it runs on threads of its own beside the commit.  The file's order is the chunks' order, and a chunk's place in the
// file is known only once every chunk before it has been compressed: whoever finishes the next chunk in line hands it -- and the finished ones
// behind it -- to the writer.
// -bz device (KG_STREAM_FORMAT_BAM_BGZF): the batch comes with the BGZF blocks the device made of its records.  A device piece whose two ends are
// block boundaries (stream_piece_blocks) goes into the file as those blocks, unchanged; everything else -- the host's own records, a device piece
// next to a pair that was mapped again -- is compressed here as before, neighbouring such pieces together.  The inflated stream is the same.
class BamPacker {
public:
	BamPacker(Writer *writer, int n_threads, std::mutex *done_mu, std::condition_variable *done_cv) : writer_(writer), done_mu_(done_mu), done_cv_(done_cv)
	{
		for (int t = 0; t < std::max(1, n_threads); ++t) th_.emplace_back([this]() { loop(); });
	}
	~BamPacker() { finish(); }
	// the pieces stay where they are until *pending has been decremented (under *done_mu): the lane's buffers are free again once the chunk is joined
	// res: the batch's result where it carries the device's BGZF blocks (else null); it is the lane's, as the pieces are
	void push(std::vector<TextPiece> &&pieces, size_t total, std::string &&hold, std::atomic<int> *pending, const kg_stream_result *res = nullptr)
	{
		std::lock_guard<std::mutex> lk(mu_);
		q_.emplace_back();
		Job &j = q_.back();
		j.seq = pushed_++; j.pieces = std::move(pieces); j.total = total; j.hold = std::move(hold); j.pending = pending;
		j.res = res && res->n_blocks > 0 ? res : nullptr;
		cv_.notify_one();
	}
	// every chunk pushed so far is with the writer when this returns
	void finish()
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			stop_ = true;
		}
		cv_.notify_all();
		for (std::thread &t : th_) t.join();
		th_.clear();
	}
	int64_t bytes() const { return bytes_; }
	int64_t device_bytes() const { return device_bytes_; }     // file bytes the device compressed / the host did (after finish())
	int64_t host_bytes() const { return bytes_ - device_bytes_; }

private:
	struct Job {
		int64_t seq = 0;
		std::vector<TextPiece> pieces;
		size_t total = 0;
		std::string hold;
		std::atomic<int> *pending = nullptr;
		const kg_stream_result *res = nullptr;
	};
	// a run of the chunk: BGZF blocks of the device's, or raw records the host compresses
	struct Seg {
		bool packed = false;
		std::string bytes;
	};
	void loop()
	{
		for (;;) {
			Job j;
			{
				std::unique_lock<std::mutex> lk(mu_);
				cv_.wait(lk, [this]() { return stop_ || !q_.empty(); });
				if (q_.empty()) return;
				j = std::move(q_.front());
				q_.pop_front();
			}
			std::string out;
			std::vector<Seg> segs;
			size_t hold_at = 0, raw_bytes = 0;
			for (const TextPiece &tp : j.pieces) {
				BlockRange br;
				if (tp.p && j.res) br = stream_piece_blocks(j.res->block_src, j.res->n_blocks, tp.p - j.res->sam, tp.p - j.res->sam + (int64_t)tp.n);
				if (br.whole) {
					const int64_t *off = j.res->block_off;
					segs.emplace_back();
					segs.back().packed = true;
					segs.back().bytes.assign((const char *)j.res->bgzf + off[br.first], (size_t)(off[br.last] - off[br.first]));
					continue;
				}
				if (segs.empty() || segs.back().packed) {
					segs.emplace_back();
					if (!j.res) segs.back().bytes.reserve(j.total);
				}
				if (tp.p) segs.back().bytes.append(tp.p, tp.n);
				else { segs.back().bytes.append(j.hold.data() + hold_at, tp.n); hold_at += tp.n; }
				raw_bytes += tp.n;
			}
			{
				std::lock_guard<std::mutex> lk(*done_mu_);
				j.pending->fetch_sub(1);
				done_cv_->notify_all();
			}
			size_t packed_bytes = 0;
			for (const Seg &sg : segs) packed_bytes += sg.packed ? sg.bytes.size() : 0;
			out.reserve(packed_bytes + raw_bytes / 3 + 64);
			for (const Seg &sg : segs) {
				if (sg.packed) out.append(sg.bytes);
				else bgzf_append(sg.bytes, out);
			}
			std::lock_guard<std::mutex> lk(mu_);
			device_bytes_ += (int64_t)packed_bytes;
			ready_[j.seq] = std::move(out);
			for (std::map<int64_t, std::string>::iterator it = ready_.begin(); it != ready_.end() && it->first == next_; it = ready_.erase(it), ++next_) {
				bytes_ += (int64_t)it->second.size();
				writer_->push(std::move(it->second));
			}
		}
	}
	Writer *writer_;
	std::mutex *done_mu_;
	std::condition_variable *done_cv_;
	std::mutex mu_;
	std::condition_variable cv_;
	std::deque<Job> q_;
	std::map<int64_t, std::string> ready_;      // compressed chunks that wait for one before them
	int64_t pushed_ = 0, next_ = 0, bytes_ = 0, device_bytes_ = 0;
	bool stop_ = false;
	std::vector<std::thread> th_;
};

// one batch in a lane
struct StreamBatch {
	int lane = 0;
	int64_t seq = 0;
	kg_stream_window win{};
	kg_stream_parsed parsed{};
	kg_stream_result res{};
	size_t abs0[2] = {0, 0};              // file offset of staging byte 0 of either window
	int est_dev = 0;
	bool fetched_all = false;             // the result holds every record and candidate (else: those of the chunks fetched, StreamBackend::fetch)
	std::vector<ChunkState> chunks;
	std::vector<Read> no_reads;           // (the host stages take a chunk's reads from ChunkState::own_reads)
	// chunks of this batch the writer has not copied out yet: the lane's result buffers are theirs.  Set before the batch's first chunk is pushed (the
	// commit, StreamRun::emit_chunks), decremented under StreamFeed::mu by whoever copied a chunk out (writer, packer), so that a waiter on
	// StreamFeed::cv sees it fall to zero
	std::atomic<int> writes_pending{0};
	bool last = false;                    // no batch follows
	size_t text_begin[2] = {0, 0}, text_end[2] = {0, 0};   // the file bytes of the batch's windows (a growing text: nothing in front of text_begin is read once the batch is committed)
};

inline MappedFile &file_of(Source &src, int f) { return f ? src.m2 : src.m1; }
inline const MappedFile &file_of(const Source &src, int f) { return f ? src.m2 : src.m1; }

// a cursor over the mapped input at read `r` of the batch, where the device found its record (never unmaps: mapped stays false)
void stream_record_cursor(const Source &src, const StreamBatch &b, int64_t r, MappedFile &one)
{
	const int f = src.sep ? (int)(r & 1) : 0;
	const int64_t j = src.sep ? r >> 1 : r;
	const MappedFile &mf = file_of(src, f);
	one.data = mf.data; one.size = mf.grow ? b.text_end[f] : mf.map_size; one.pos = b.abs0[f] + (size_t)b.res.rec_start[f][j];
	one.gz_lines = mf.gz_lines;
}

// FASTA: GetNextEntry from the record's header on (fasta_view_next).  A sequence of several lines, and a mate held reverse-complemented,
// need storage of their own: Read::seq is one piece of memory
void stream_own_reads_fasta(const Ctx &cx, const Source &src, const StreamBatch &b, ChunkState &ck)
{
	const size_t nh = ck.hq.size();
	std::vector<FastaView> views(nh);
	std::vector<size_t> size_of(nh);
	size_t own = 0;
	for (size_t k = 0; k < nh; ++k) {
		const int64_t r = ck.begin + ck.hq[k];
		MappedFile one;
		stream_record_cursor(src, b, r, one);
		size_of[k] = one.size;
		if (!fasta_view_next(one, views[k])) { fprintf(stderr, "Error! a record the device parsed cannot be read back\n"); exit(1); }
		if (views[k].joined || (cx.opt.paired && (r & 1))) own += (size_t)views[k].rlen;
	}
	ck.own_chars.assign(own, '\0');
	std::string joined;
	size_t at = 0;
	for (size_t k = 0; k < nh; ++k) {
		const FastaView &v = views[k];
		const int64_t r = ck.begin + ck.hq[k];
		const bool flip = cx.opt.paired && (r & 1);
		Read &rd = ck.own_reads[k];
		rd.name = header_view(v.hdr, v.hdr_len);
		rd.raw = std::string_view(v.hdr, v.raw_len);
		rd.rlen = v.rlen;
		if (!v.joined && !flip) { rd.seq = std::string_view(v.seq ? v.seq : "", (size_t)v.rlen); continue; }
		char *dst = &ck.own_chars[at];
		const char *seq = v.seq;
		if (v.joined) {
			char *to = dst;
			if (flip) { joined.assign((size_t)v.rlen, '\0'); to = &joined[0]; }
			fasta_join(file_of(src, src.sep ? (int)(r & 1) : 0).data, size_of[k], v, to);
			seq = to;
		}
		if (flip) revcomp_into(dst, seq, (size_t)v.rlen);
		rd.seq = std::string_view(dst, (size_t)v.rlen);
		at += (size_t)v.rlen;
	}
}

void stream_own_reads_fastq(const Ctx &cx, const Source &src, const StreamBatch &b, ChunkState &ck)
{
	const size_t nh = ck.hq.size();
	size_t flipped = 0;
	std::vector<RecView> views(nh);
	for (size_t k = 0; k < nh; ++k) {
		const int64_t r = ck.begin + ck.hq[k];
		MappedFile one;
		stream_record_cursor(src, b, r, one);
		RecView &v = views[k];
		if (!view_next(one, v)) { fprintf(stderr, "Error! a record the device parsed cannot be read back\n"); exit(1); }
		v.flip = cx.opt.paired && (r & 1);
		if (v.flip) flipped += (size_t)v.rlen;
	}
	ck.own_chars.assign(flipped, '\0');
	size_t at = 0;
	for (size_t k = 0; k < nh; ++k) {
		const RecView &v = views[k];
		Read &rd = ck.own_reads[k];
		rd.name = header_view(v.hdr, v.hdr_len);
		rd.raw = std::string_view(v.hdr, (size_t)v.raw_len);
		rd.rlen = v.rlen;
		int ql = std::min(v.qual_len, v.rlen);
		const char *z = ql > 0 ? (const char *)memchr(v.qual, '\0', (size_t)ql) : nullptr;
		if (z) ql = (int)(z - v.qual);
		rd.qual = std::string_view(v.qual ? v.qual : "", (size_t)ql);
		if (!v.flip) { rd.seq = std::string_view(v.seq, (size_t)v.rlen); continue; }
		revcomp_into(&ck.own_chars[at], v.seq, (size_t)v.rlen);
		rd.seq = std::string_view(&ck.own_chars[at], (size_t)v.rlen);
		rd.qual_rev = true;
		at += (size_t)v.rlen;
	}
}

// the reads of chunk `ck` listed in ck.hq, parsed from the mapped input exactly as view_next() / materialise() do
void stream_own_reads(const Ctx &cx, const Source &src, const StreamBatch &b, ChunkState &ck)
{
	ck.own_reads.assign(ck.hq.size(), Read());
	if (cx.fastq) stream_own_reads_fastq(cx, src, b, ck);
	else stream_own_reads_fasta(cx, src, b, ck);
}

// the chunk's text as pieces: the device's lines between the reads the host mapped, and the host's own lines for those
// (pieces without address: consecutive parts of ck.text)
void stream_chunk_pieces(const StreamBatch &b, const ChunkState &ck, std::vector<TextPiece> &out, size_t &total)
{
	const int64_t *off = b.res.sam_off;
	const char *sam = b.res.sam;
	const int step = ck.paired ? 2 : 1;
	int64_t from = ck.begin;
	size_t piece = 0;
	total = 0;
	for (size_t k = 0; k < ck.hq.size(); k += (size_t)step) {
		const int64_t r = ck.begin + ck.hq[k];
		if (off[r] > off[from]) { out.push_back(TextPiece{sam + off[from], (size_t)(off[r] - off[from])}); total += out.back().n; }
		const uint32_t n = ck.host_len[piece++];
		if (n) { out.push_back(TextPiece{nullptr, n}); total += n; }
		from = r + step;
		// (a forced pair's device lines, sam[off[r], off[r + step]), are skipped: the host mapped it again)
	}
	const int64_t end = ck.begin + ck.count;
	if (off[end] > off[from]) { out.push_back(TextPiece{sam + off[from], (size_t)(off[end] - off[from])}); total += out.back().n; }
}

// -un / -un2: the chunk's unmapped reads of input file f as pieces, the same way: the device's bytes (kg_stream_result::un, per unit) between the units
// the host mapped, and the host's own bytes for those (consecutive parts of ck.un_text[f], ck.un_host_len[f] per unit in hq order)
void stream_chunk_un_pieces(const StreamBatch &b, const ChunkState &ck, int f, std::vector<TextPiece> &out, size_t &total)
{
	const int64_t *off = b.res.un_off[f];
	const char *un = (const char *)b.res.un[f];
	const int step = ck.paired ? 2 : 1;
	int64_t from = ck.begin / step;
	size_t piece = 0;
	total = 0;
	for (size_t k = 0; k < ck.hq.size(); k += (size_t)step) {
		const int64_t u = (ck.begin + ck.hq[k]) / step;
		if (off[u] > off[from]) { out.push_back(TextPiece{un + off[from], (size_t)(off[u] - off[from])}); total += out.back().n; }
		const uint32_t n = ck.un_host_len[f][piece++];
		if (n) { out.push_back(TextPiece{nullptr, n}); total += n; }
		from = u + 1;
		// (a forced pair's device bytes are skipped: the host decided it again)
	}
	const int64_t end = (ck.begin + ck.count) / step;
	if (off[end] > off[from]) { out.push_back(TextPiece{un + off[from], (size_t)(off[end] - off[from])}); total += out.back().n; }
}

// the reads of a chunk the host stages map: the device's list restricted to the chunk, plus the forced pairs
void stream_list_host_reads(const StreamBatch &b, ChunkState &ck)
{
	ck.hq.clear();
	const int32_t *hl = b.res.host_reads, *he = hl + b.res.n_host_reads;
	const int32_t *lo = std::lower_bound(hl, he, (int32_t)ck.begin), *hi = std::lower_bound(lo, he, (int32_t)(ck.begin + ck.count));
	if (ck.force.empty()) {
		for (const int32_t *p = lo; p < hi; ++p) ck.hq.push_back((int)(*p - ck.begin));
		return;
	}
	for (int q = 0; q < ck.count; ++q)
		if (ck.recs[ck.begin + q].kind == KG_ALN_HOST || ck.force[(size_t)q]) ck.hq.push_back(q);
}

// (a growing text -- the inflated gz file a thread of its own writes, GzProducer -- has no end yet: it is learnt when a block reaches it)
constexpr size_t kNoEnd = ~(size_t)0;

// bytes of one file to hand out as the next batch's raw block.  The window should hold about `want` reads over `nf` files of `bpr` bytes per
// record: what is outstanding of the file -- handed out (`raw`) and not consumed (`pos`), beyond what the `batches_between` blocks handed
// out and not yet parsed will consume themselves -- counts
inline int64_t stream_block_bytes(int64_t want, int nf, int64_t batches_between, size_t raw, size_t pos, double bpr, int64_t bulk_cap)
{
	const double recs = (double)want / (double)nf;
	double outstanding = (double)(raw - pos) - (double)batches_between * recs * bpr;
	if (outstanding < 0) outstanding = 0;
	const double w = recs * bpr * 1.02 + 65536 - outstanding;
	return (int64_t)std::max(0.0, std::min(w, (double)bulk_cap));
}

// Where a batch's window of one file lies in the lane's staging buffer.  The raw block [blk0, blk1) of the file sits at staging byte
// `carry_cap`; the unconsumed tail in front of it, file bytes [pos, blk0), goes right before it.
struct WindowPlace {
	int64_t begin = 0, end = 0;           // the window in the staging buffer
	bool eof = false;                     // the block ends where the file does
	size_t abs0 = 0;                      // file offset of staging byte 0 (modular: staging byte carry_cap is file byte blk0)
	size_t text_begin = 0, text_end = 0;  // the file bytes the window holds
	bool fits = false;                    // false: the tail is longer than the room in front of the block
};
inline WindowPlace stream_place_window(size_t blk0, size_t blk1, size_t pos, size_t file_end, int64_t carry_cap)
{
	const int64_t carry = (int64_t)(blk0 - pos);
	WindowPlace p;
	p.fits = carry <= carry_cap;
	p.begin = carry_cap - carry;
	p.end = carry_cap + (int64_t)(blk1 - blk0);
	p.eof = blk1 == file_end;
	p.abs0 = blk0 - (size_t)carry_cap;
	p.text_begin = blk0 - (size_t)std::max<int64_t>(0, carry);
	p.text_end = blk1;
	return p;
}

// the raw block of either file a batch was given, and the reads the batch aims at
struct StreamBlock {
	size_t blk0[2] = {0, 0}, blk1[2] = {0, 0};
	int64_t want = 0;
};

// What the lanes and the commit agree on: batch s = lane s % K.  Three counters walk the batches in order -- dispatched (raw blocks), parsed
// (windows), committed (output) -- and every wait of the run is a wait for one of them (or for a lane's writes_pending) on the one condition
// variable.  A method that returns false tells a lane's thread to end: the stream is over (or failed) in front of its batch.
struct StreamFeed {
	std::mutex mu;
	std::condition_variable cv;
	int nf = 1, K = 1;
	MappedFile *file[2] = {nullptr, nullptr};
	// batches whose raw block has been assigned.  Only batch s moves raw[], target, end[] and the files' sizes while dispatched == s: that is
	// why its wait for a growing text may drop the lock (claim_block)
	int64_t dispatched = 0;
	// batches parsed.  Only batch s writes pos[] / bpr[] while parsed == s: batch s reads them without the lock between place_in_staging and publish_parse
	int64_t parsed = 0;
	size_t pos[2] = {0, 0};               // first unconsumed byte of either file (exact after every parse)
	size_t raw[2] = {0, 0};               // bytes of either file handed out as raw blocks
	size_t end[2] = {0, 0};               // where this process's part of either file ends (kNoEnd: not known yet)
	double bpr[2] = {0, 0};               // bytes per record, measured
	int64_t target = 4000;                // reads the next batch aims at
	bool finished = false;                // no further batch: the files ended (done), or the host's reader takes over at pos[] (fallback)
	bool fallback = false;
	// in-order hand-over to the commit: every batch up to the one marked last arrives here, in whatever order the lanes finish
	std::map<int64_t, StreamBatch *> ready;
	// batches committed.  A lane may start batch s only when committed + K > s (its previous batch, s - K, is committed: nobody reads its
	// chunk states any more) and its writes_pending is zero (nobody reads its result buffers any more)
	int64_t committed = 0;
	bool failed = false;

	// ---- the lanes ----
	bool lane_may_start(int64_t s, const StreamBatch &b)
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&]() { return failed || (b.writes_pending.load() == 0 && committed + K > s); });
		return !failed;
	}
	// this batch's raw block of either file, assigned in batch order; batches grow towards `full_target` reads
	bool claim_block(int64_t s, int64_t bulk_cap, int64_t full_target, StreamBlock &blk)
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&]() { return failed || finished || dispatched == s; });
		if (failed || finished) return false;            // (the batch that finished the stream lies before this one)
		blk.want = target;
		int64_t bytes_of[2] = {0, 0};
		bool grows = false;
		for (int f = 0; f < nf; ++f) {
			bytes_of[f] = stream_block_bytes(blk.want, nf, s - parsed, raw[f], pos[f], bpr[f], bulk_cap);
			grows = grows || (file[f]->grow && end[f] == kNoEnd);
		}
		if (grows) {
			// the block of a growing text must exist before it is handed out (or the text must have ended in front of its end): waited for without the lock
			size_t upto[2] = {raw[0] + (size_t)bytes_of[0], raw[1] + (size_t)bytes_of[1]};
			lk.unlock();
			size_t have[2] = {0, 0};
			bool ended[2] = {false, false};
			for (int f = 0; f < nf; ++f)
				if (file[f]->grow) have[f] = file[f]->grow->wait_for(upto[f], ended[f]);
			lk.lock();
			if (failed || finished) return false;
			for (int f = 0; f < nf; ++f)
				if (file[f]->grow) {
					if (have[f] > file[f]->size) file[f]->size = file[f]->map_size = have[f];
					if (ended[f]) end[f] = have[f];
				}
		}
		for (int f = 0; f < nf; ++f) {
			blk.blk0[f] = raw[f];
			blk.blk1[f] = std::min(end[f], raw[f] + (size_t)bytes_of[f]);
			raw[f] = blk.blk1[f];
		}
		dispatched = s + 1;
		// batches grow towards the full size: the estimate moves fastest while the totals are small
		target = std::min<int64_t>(full_target, target * 4);
		cv.notify_all();
		return true;
	}
	// the unconsumed tail in front of the block is known once the batch before has been parsed
	bool wait_parsed_before(int64_t s)
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&]() { return failed || finished || parsed == s; });
		return !(failed || finished);
	}
	// (parsed == s) the batch's windows in its lane's staging buffer.  false: the batch has no window -- the tail does not fit in front of the block
	// (the windows drifted apart further than the staging buffer allows: the host's reader continues at pos[]), or nothing is left to read -- and
	// was handed over as the stream's last
	bool place_in_staging(int64_t s, StreamBatch &b, const StreamBlock &blk, int64_t carry_cap, kg_stream_window &w)
	{
		std::lock_guard<std::mutex> lk(mu);
		bool give_up = false, nothing = true;
		for (int f = 0; f < nf; ++f) {
			const WindowPlace p = stream_place_window(blk.blk0[f], blk.blk1[f], pos[f], end[f], carry_cap);
			if (!p.fits) give_up = true;
			w.begin[f] = p.begin; w.end[f] = p.end; w.eof[f] = p.eof;
			b.abs0[f] = p.abs0; b.text_begin[f] = p.text_begin; b.text_end[f] = p.text_end;
			nothing = nothing && p.end == p.begin;
		}
		if (give_up) fallback = true;
		if (give_up || nothing) hand_over_last(b, s);
		return !(give_up || nothing);
	}
	// (parsed == s) what the parse of batch s consumed; `fits` false: the window did not fit the lane
	void publish_parse(int64_t s, StreamBatch &b, bool fits)
	{
		std::lock_guard<std::mutex> lk(mu);
		if (!fits) { finished = true; fallback = true; b.parsed = kg_stream_parsed{}; }
		else {
			for (int f = 0; f < nf; ++f) {
				const size_t before = pos[f];
				pos[f] = b.abs0[f] + (size_t)b.parsed.used[f];
				const int64_t recs = nf == 2 ? b.parsed.n_reads / 2 : b.parsed.n_reads;
				if (recs > 0) bpr[f] = (double)(pos[f] - before) / (double)recs;
			}
			if (b.parsed.done) finished = true;
			else if (b.parsed.stop != KG_STREAM_STOP_NONE) { finished = true; fallback = true; }
			else if (b.parsed.n_reads == 0 && b.win.eof[0] && (nf == 1 || b.win.eof[1])) { finished = true; fallback = true; }   // (cannot happen: a window at the end of both files is done, stopped or non-empty)
		}
		b.last = finished;
		parsed = s + 1;
		cv.notify_all();
	}
	void hand_over(int64_t s, StreamBatch &b)
	{
		std::lock_guard<std::mutex> lk(mu);
		ready[s] = &b;
		cv.notify_all();
	}

	// ---- the commit ----
	StreamBatch &take(int64_t s)
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&]() { return ready.count(s) != 0; });
		std::map<int64_t, StreamBatch *>::iterator it = ready.find(s);
		StreamBatch *b = it->second;
		ready.erase(it);
		return *b;
	}
	void publish_commit(int64_t s)
	{
		std::lock_guard<std::mutex> lk(mu);
		committed = s + 1;
		cv.notify_all();
	}
	// every chunk's pieces point into the lanes' result buffers: they must be in the file before the lanes go away
	void wait_writes_done(const std::vector<std::unique_ptr<StreamBatch>> &batches)
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&]() {
			for (const std::unique_ptr<StreamBatch> &b : batches)
				if (b->writes_pending.load() != 0) return false;
			return true;
		});
	}

private:
	// a batch without reads that ends the stream (the commit walks the batches in order up to the one marked last); mu held
	void hand_over_last(StreamBatch &b, int64_t s)
	{
		b.seq = s; b.last = true;
		b.parsed = kg_stream_parsed{}; b.res = kg_stream_result{}; b.chunks.clear();
		finished = true;
		parsed = s + 1;
		ready[s] = &b;
		cv.notify_all();
	}
};

// what the lanes' host threads waited for / worked on, summed over the lanes (Stats::lane_seconds has the same order)
struct LaneTimers {
	enum Step { kWaitLane, kReadUpload, kWaitParse, kParse, kMap, kHostReads, kSteps };
	std::atomic<int64_t> ns[kSteps];
	LaneTimers() { for (std::atomic<int64_t> &a : ns) a.store(0); }
	void add(Step s, double t0) { ns[s] += (int64_t)((now_s() - t0) * 1e9); }
	double seconds(int s) const { return 1e-9 * (double)ns[s].load(); }
};

void add_timing(kg_stream_timing_t &into, const kg_stream_timing_t &from)
{
	into.batches += from.batches; into.reads += from.reads;
	into.parse_ms += from.parse_ms; into.seed_ms += from.seed_ms; into.chain_ms += from.chain_ms; into.align_ms += from.align_ms; into.format_ms += from.format_ms; into.copy_ms += from.copy_ms;
	into.search_kernel_ms += from.search_kernel_ms; into.search_kernel_launches += from.search_kernel_launches; into.search_useful_bytes += from.search_useful_bytes;
	into.text_in_bytes += from.text_in_bytes; into.text_out_bytes += from.text_out_bytes;
	into.candidates += from.candidates; into.candidate_seeds += from.candidate_seeds;
	for (int i = 0; i < 16; ++i) { into.kernel_ms[i] += from.kernel_ms[i]; into.kernel_launches[i] += from.kernel_launches[i]; }
	for (int i = 0; i < 8; ++i) into.aln_counts[i] += from.aln_counts[i];
	into.text_checksum[0] += from.text_checksum[0]; into.text_checksum[1] += from.text_checksum[1];
	for (int i = 0; i < 2; ++i) { into.un_kernel_ms[i] += from.un_kernel_ms[i]; into.un_kernel_launches[i] += from.un_kernel_launches[i]; }
	into.un_bytes += from.un_bytes;
	into.stats_kernel_ms += from.stats_kernel_ms; into.stats_kernel_launches += from.stats_kernel_launches; into.stats_bytes += from.stats_bytes;
}

// One library's run through the stream: K lane threads (lane_thread) feed the commit (the caller's thread) through `feed`.
struct StreamRun {
	Ctx &cx;
	Source &src;
	StreamBackend &sb;
	Writer *writer;
	std::vector<DeferredChunk> *held;
	Stats &st;
	RunTotals &tot;
	std::atomic<int> &est_latest;
	const Shard *shard;
	int64_t &bytes_out;
	static constexpr int chunk_limit = 4000;
	const int nf, K;
	const int64_t bulk_cap, carry_cap;    // a staging buffer: [0, carry_cap) the tail of the text before the block, [carry_cap, carry_cap + bulk_cap) the block
	const int64_t max_reads, full_target;
	const bool verbose;
	StreamFeed feed;
	std::unique_ptr<TaskPool> pool;       // the few reads the device hands back, the commit's re-maps
	std::unique_ptr<BamPacker> packer;
	std::vector<std::unique_ptr<StreamBatch>> batches;     // one per lane
	LaneTimers timers;

	StreamRun(Ctx &cx_, Source &src_, StreamBackend &sb_, Writer *writer_, Stats &st_, RunTotals &tot_, std::atomic<int> &est_latest_,
	          std::vector<DeferredChunk> *held_, int64_t &bytes_out_, const Shard *shard_)
		: cx(cx_), src(src_), sb(sb_), writer(writer_), held(held_), st(st_), tot(tot_), est_latest(est_latest_), shard(shard_), bytes_out(bytes_out_),
		  nf(src_.sep ? 2 : 1), K(sb_.lanes()), bulk_cap(sb_.max_window() / 4 * 3), carry_cap(sb_.max_window() - bulk_cap),
		  max_reads(sb_.max_reads() / chunk_limit * chunk_limit),
		  full_target(std::max<int64_t>(chunk_limit, std::min<int64_t>(max_reads, cx_.opt.batch_reads / chunk_limit * chunk_limit))),
		  verbose(getenv("KART_AMD_VERBOSE") != nullptr)
	{
		{ kg_stream_timing_t drop{}; sb.timing(drop, true); }      // (the stream is the session's: count this run's batches only)
	}

	// the feed at the files' current positions, the first batch's size, the bytes per record of either file, the size of the output; then the
	// run's own threads (pool, packer) and the lanes' batches
	void prime(int64_t ramp_from)
	{
		feed.nf = nf; feed.K = K;
		for (int f = 0; f < nf; ++f) {
			MappedFile &mf = file_of(src, f);
			feed.file[f] = &mf;
			feed.pos[f] = feed.raw[f] = mf.pos;
			feed.end[f] = mf.size;
			if (mf.grow) {
				bool ended = false;
				const size_t have = mf.grow->wait_for(mf.pos + ((size_t)1 << 18), ended);
				mf.size = mf.map_size = have;
				feed.end[f] = ended ? have : kNoEnd;
			}
		}
		feed.target = std::max<int64_t>(chunk_limit, std::min<int64_t>(full_target, ramp_from));
		for (int f = 0; f < nf; ++f) {
			// bytes per record from the first records of the file (four lines each; FASTA: a header line each)
			const MappedFile &mf = file_of(src, f);
			size_t lo = feed.pos[f], hi = std::min(std::min(feed.end[f], mf.size), lo + ((size_t)1 << 18));
			int64_t lines = 0, blank = 0;
			count_lines(mf.data, lo, hi, lines, blank);
			feed.bpr[f] = !cx.fastq ? fasta_bytes_per_record(mf.data, lo, hi) : lines >= 8 ? 4.0 * (double)(hi - lo) / (double)lines : 400.0;
		}
		// the SAM text of short reads is about 1.2 x the FASTQ text it comes from: its pages are allocated while the first batches map
		if (writer && !held) {
			double text = 0;
			for (int f = 0; f < nf; ++f) text += feed.end[f] != kNoEnd ? (double)(feed.end[f] - feed.pos[f]) : 4.5 * (double)src.gz_packed[f];     // (FASTQ text packs ~4-5 x)
			writer->expect((size_t)(1.2 * text));
		}
		pool.reset(new TaskPool(std::max(1, cx.opt.threads / 2), 5));
		// -bo: the whole thread budget compresses (the lane threads wait for the device, the pool for the few reads handed back, the writers for the packer)
		if (cx.opt.bam && writer && !held) packer.reset(new BamPacker(writer, std::max(1, cx.opt.threads), &feed.mu, &feed.cv));
		for (int l = 0; l < K; ++l) { batches.emplace_back(new StreamBatch()); batches.back()->lane = l; }
	}

	// ---- a lane: its batches s = lane, lane + K, ... one step after the other ----
	void lane_thread(int lane)
	{
		pin_lane_thread();
		StreamBatch &b = *batches[(size_t)lane];
		for (int64_t s = lane; lane_batch(b, s); s += K) {}
		sb.group_absent(lane, -1);          // no further batch in this lane: its group's rounds go on without it
	}
	// false: the lane's thread ends
	bool lane_batch(StreamBatch &b, int64_t s)
	{
		StreamBlock blk;
		kg_stream_window w{};
		if (!wait_lane_free(b, s)) return false;
		if (!feed.claim_block(s, bulk_cap, full_target, blk)) return false;
		read_and_upload(b.lane, blk);
		if (!place_window(b, s, blk, w)) return false;
		parse_and_publish(b, s, blk.want, w);
		map_or_sit_out(b);
		feed.hand_over(s, b);
		return !b.last;
	}
	// 1. the lane's buffers are free again once the writer has copied the previous batch's text out
	bool wait_lane_free(StreamBatch &b, int64_t s)
	{
		double t0 = now_s();
		if (!feed.lane_may_start(s, b)) return false;
		timers.add(LaneTimers::kWaitLane, t0);
		return true;
	}
	// 3. read ahead and upload the block (8 MB pieces: the upload of one runs while the next is read)
	void read_and_upload(int lane, const StreamBlock &blk)
	{
		double t0 = now_s();
		for (int f = 0; f < nf; ++f) {
			const MappedFile &mf = file_of(src, f);
			char *stg = sb.staging(lane, f);
			const size_t piece = (size_t)8 << 20, blk0 = blk.blk0[f], blk1 = blk.blk1[f];
			for (size_t a = blk0; a < blk1; a += piece) {
				size_t e = std::min(blk1, a + piece);
				// (pread: the kernel copies out of the page cache into the page-locked buffer -- reading through the mapping costs a
				//  fault per 64 KB of input and the address space's lock, which the writers' faults want as well; KART_AMD_NO_PREAD=1: memcpy)
				static const bool use_pread = getenv("KART_AMD_NO_PREAD") == nullptr;
				bool done = false;
				if (use_pread && mf.fd >= 0) {
					size_t got = 0;
					while (got < e - a) {
						ssize_t k = ::pread(mf.fd, stg + carry_cap + (a - blk0) + got, e - a - got, (off_t)(a + got));
						if (k <= 0) break;
						got += (size_t)k;
					}
					done = got == e - a;
				}
				if (!done) memcpy(stg + carry_cap + (a - blk0), mf.data + a, e - a);
				sb.upload(lane, f, carry_cap + (int64_t)(a - blk0), carry_cap + (int64_t)(e - blk0));
			}
		}
		timers.add(LaneTimers::kReadUpload, t0);
	}
	// 4. the unconsumed tail in front of the block: known once the batch before has been parsed
	bool place_window(StreamBatch &b, int64_t s, const StreamBlock &blk, kg_stream_window &w)
	{
		double t0 = now_s();
		const bool go_on = feed.wait_parsed_before(s);
		timers.add(LaneTimers::kWaitParse, t0);
		if (!go_on || !feed.place_in_staging(s, b, blk, carry_cap, w)) return false;
		for (int f = 0; f < nf; ++f) {
			const int64_t carry = carry_cap - w.begin[f];
			if (carry > 0) {
				memcpy(sb.staging(b.lane, f) + w.begin[f], file_of(src, f).data + (blk.blk0[f] - (size_t)carry), (size_t)carry);
				sb.upload(b.lane, f, w.begin[f], carry_cap);
			}
		}
		return true;
	}
	// 5. the device finds the window's records; what it consumed is where the next batch's window begins
	void parse_and_publish(StreamBatch &b, int64_t s, int64_t want, kg_stream_window &w)
	{
		w.two_files = src.sep ? 1 : 0;
		w.gz_lines = src.m1.gz_lines ? 1 : 0;
		w.paired = cx.opt.paired ? 1 : 0;
		w.chunk_reads = chunk_limit;
		w.want_reads = std::min<int64_t>(max_reads, std::max<int64_t>(chunk_limit, (want + want / 4) / chunk_limit * chunk_limit));
		b.win = w;
		b.seq = s;
		double tp = now_s();
		const bool fits = sb.parse(b.lane, w, b.parsed);
		timers.add(LaneTimers::kParse, tp);
		feed.publish_parse(s, b, fits);
	}
	// 6. map the batch and the reads the device hands back -- or, without reads, sit this round of the lane's seeding group out
	void map_or_sit_out(StreamBatch &b)
	{
		if (b.parsed.n_reads <= 0) { b.res = kg_stream_result{}; b.chunks.clear(); sb.group_absent(b.lane, 1); return; }
		kg_stream_params prm;
		prm.est_distance = b.est_dev = est_latest.load();
		prm.max_insert = cx.opt.max_insert; prm.max_gaps = cx.opt.max_gaps; prm.multi_hit = cx.opt.multi_hit ? 1 : 0; prm.unset_flag = g_unset_flag;
		// (the check mode compares every record; KART_AMD_FETCH_ALL: A/B aid, everything crosses the link as before round 6)
		static const bool fetch_all_env = getenv("KART_AMD_FETCH_ALL") != nullptr;
		prm.fetch_all = (g_check_align || fetch_all_env) ? 1 : 0;
		b.fetched_all = prm.fetch_all != 0;
		double tm = now_s();
		sb.map(b.lane, prm, b.res);
		timers.add(LaneTimers::kMap, tm);
		double th = now_s();
		host_stage(b);
		timers.add(LaneTimers::kHostReads, th);
	}
	// what the host does for a mapped batch before the commit: chunk states from the device's statistics, the handed-back reads
	void host_stage(StreamBatch &b)
	{
		const kg_stream_result &res = b.res;
		b.chunks.assign((size_t)res.n_chunks, ChunkState());
		std::vector<int> busy;
		for (int c = 0; c < (int)res.n_chunks; ++c) {
			ChunkState &ck = b.chunks[(size_t)c];
			ck.begin = c * chunk_limit;
			ck.count = (int)std::min<int64_t>(chunk_limit, res.n_reads - ck.begin);
			ck.paired = cx.opt.paired;
			ck.recs = res.records;
			ck.dev = res.chunk_stats[c];
			ck.stream = true;
			if (cx.stats) {
				if (!res.chunk_tally) run_fail("the device stream returned no tally for a batch of a -stats run");
				else ck.dev_tally = res.chunk_tally + (size_t)c * KG_STATS_WORDS;
				ck.n_records_reads = res.n_reads; ck.n_records = res.n_records;
			}
			stream_list_host_reads(b, ck);
			if (!ck.hq.empty()) busy.push_back(c);
		}
		// chunks without host reads need no work at all: their statistics are the device's (stage A's first lines)
		for (ChunkState &ck : b.chunks)
			if (ck.hq.empty()) {
				chunk_stage_a(cx, b.no_reads, res.cand_off, res.cands, res.cand_seeds, ck, b.est_dev); ck.text.clear(); ck.host_len.clear(); ck.st.total_reads = ck.count;
				// (-stats: no stage C for such a chunk -- its tally is the device's row)
				if (cx.stats) { ck.tally = std::make_shared<Tally>(); chunk_device_tally(ck); }
			}
		// the others: their records and candidates come over now (the batch's result holds them only for the chunks asked for, kg_stream_fetch),
		// then: plan on the pool, ONE gap-closing call for the batch's handed-back reads (a call per chunk was ~13 small device
		// calls per 1 M-read batch behind one mutex), finish on the pool
		if (!b.fetched_all)
			for (int c : busy) sb.fetch(b.lane, b.chunks[(size_t)c].begin, b.chunks[(size_t)c].count);
		pool->run((int)busy.size(), [&](int i) {
			ChunkState &ck = b.chunks[(size_t)busy[(size_t)i]];
			stream_own_reads(cx, src, b, ck);
			chunk_stage_a(cx, b.no_reads, res.cand_off, res.cands, res.cand_seeds, ck, b.est_dev);
		});
		std::vector<NwJobs *> parts;
		for (int c : busy)
			if (b.chunks[(size_t)c].jobs.size() > 0) parts.push_back(&b.chunks[(size_t)c].jobs);
		if (!parts.empty()) cx.kern.nw_batch(parts);
		pool->run((int)busy.size(), [&](int i) { chunk_stage_c(cx, b.no_reads, b.chunks[(size_t)busy[(size_t)i]]); });
	}

	// ---- the in-order commit (src/Mapping.cpp:533-540), as in map_library() ----
	void commit()
	{
		for (int64_t s = 0;; ++s) {
			StreamBatch &b = feed.take(s);
			double t0 = now_s();
			if (!b.chunks.empty()) {
				settle_estimates(b);
				emit_chunks(b);
				est_latest.store(est_speculated(cx, shard, tot.iPaired, tot.iDistance));
				if (shard && shard->active() && shard->rank == 0) { shard->rdv->hint_paired.store(tot.iPaired); shard->rdv->hint_distance.store(tot.iDistance); }
			}
			tot.t_commit += now_s() - t0;
			// read what the rest of this round needs of the batch BEFORE the commit is published: from then on the lane may place its next batch
			// (s + K) in it and overwrite text_begin, and release() would give back pages that batches s + 1 .. s + K - 1 still read
			const bool last = b.last;
			const size_t text_begin[2] = {b.text_begin[0], b.text_begin[1]};
			feed.publish_commit(s);
			// (a growing text: the pages in front of this batch's windows are read by nobody any more)
			for (int f = 0; f < nf; ++f)
				if (file_of(src, f).grow) file_of(src, f).grow->release(text_begin[f]);
			if (last) break;
		}
	}
	// the chunks whose speculated EstDistance does not hold against the totals in front of them are mapped again, until all hold
	void settle_estimates(StreamBatch &b)
	{
		const kg_stream_result &res = b.res;
		for (;;) {
			std::vector<std::pair<size_t, int>> redo;
			int64_t paired = tot.iPaired, distance = tot.iDistance;
			for (size_t c = 0; c < b.chunks.size(); ++c) {
				ChunkState &ck = b.chunks[c];
				if (ck.paired) {
					int est_true = held ? ck.est_used : est_distance(cx, paired, distance);      // (a deferred shard settles later)
					bool valid = est_true == ck.est_used ||
					             (ck.ps.lo < est_true && est_true <= ck.ps.hi &&
					              (!ck.ps.rescue_used || std::min(est_true, cx.opt.max_insert) == std::min(ck.est_used, cx.opt.max_insert)));
					if (!valid) redo.emplace_back(c, est_true);
				}
				paired += ck.ps.paired;
				distance += ck.ps.distance;
			}
			if (redo.empty()) return;
			st.respeculated += (int64_t)redo.size();
			// (the pairs' validity intervals are in the records: the chunk's come over now -- the lane's batch is still resident, its thread waits for this commit)
			if (!b.fetched_all)
				for (const std::pair<size_t, int> &rd_ : redo) sb.fetch(b.lane, b.chunks[rd_.first].begin, b.chunks[rd_.first].count);
			pool->run((int)redo.size(), [&](int i) {
				ChunkState &ck = b.chunks[redo[(size_t)i].first];
				ck.force_invalid_pairs(redo[(size_t)i].second, cx.opt.max_insert);
				stream_list_host_reads(b, ck);
				stream_own_reads(cx, src, b, ck);
				chunk_stage_a(cx, b.no_reads, res.cand_off, res.cands, res.cand_seeds, ck, redo[(size_t)i].second);
				if (ck.jobs.size() > 0) { std::vector<NwJobs *> parts{&ck.jobs}; cx.kern.nw_batch(parts); }
				chunk_stage_c(cx, b.no_reads, ck);
			});
		}
	}
	// every chunk's text to where it goes: a deferred shard's list, the packer (-bo) or the writer
	void emit_chunks(StreamBatch &b)
	{
		// (-un / -un2: every chunk is pushed to each of those writers as well, and each push counts)
		const int n_un = cx.un_writer[0] ? (cx.un_writer[1] ? 2 : 1) : 0;
		b.writes_pending.store((int)b.chunks.size() * (1 + n_un));
		for (size_t c = 0; c < b.chunks.size(); ++c) {
			ChunkState &ck = b.chunks[c];
			for (int f = 0; f < n_un; ++f) {
				std::vector<TextPiece> un_pieces;
				size_t un_total = 0;
				stream_chunk_un_pieces(b, ck, f, un_pieces, un_total);
				cx.un_writer[f]->push_pieces(std::move(un_pieces), un_total, std::move(ck.un_text[f]), &b.writes_pending, &feed.mu, &feed.cv);
			}
			std::vector<TextPiece> pieces;
			size_t total = 0;
			stream_chunk_pieces(b, ck, pieces, total);
			if (!held) bytes_out += (int64_t)total;           // (a deferred shard's bytes are counted when it settles)
			tot.dev_reads += ck.count - ck.n_host; tot.host_reads += ck.n_host;
			tot.iPaired += ck.ps.paired;
			tot.iDistance += ck.ps.distance;
			st.stream_reads += ck.count;
			if (held) { hold_chunk(b, ck, pieces, total); continue; }
			st.total_reads += ck.count;
			st.unmapped += ck.st.unmapped;
			st.unique += ck.st.unique;
			if (st.tally && ck.tally) *st.tally += *ck.tally;
			if (packer) packer->push(std::move(pieces), total, std::move(ck.text), &b.writes_pending, &b.res);
			else writer->push_pieces(std::move(pieces), total, std::move(ck.text), &b.writes_pending, &feed.mu, &feed.cv);
		}
	}
	// a deferred shard keeps its chunks (text, validity, where they came from) until the totals in front of it are known
	void hold_chunk(StreamBatch &b, ChunkState &ck, const std::vector<TextPiece> &pieces, size_t total)
	{
		DeferredChunk d;
		d.paired = ck.paired; d.est_used = ck.est_used; d.ps = ck.ps; d.st = ck.st;
		d.st.total_reads = ck.count;
		d.text.reserve(total);
		size_t host_at = 0;
		for (const TextPiece &tp : pieces) {
			if (tp.p) d.text.append(tp.p, tp.n);
			else { d.text.append(ck.text.data() + host_at, tp.n); host_at += tp.n; }
		}
		const int64_t r0 = ck.begin;
		d.from_stream = true;
		d.count = ck.count;
		d.fpos[0] = b.abs0[0] + (size_t)b.res.rec_start[0][src.sep ? r0 >> 1 : r0];
		d.fpos[1] = src.sep ? b.abs0[1] + (size_t)b.res.rec_start[1][r0 >> 1] : 0;
		held->push_back(std::move(d));
		if (writer) write_held_chunk(writer, held->back());          // (a -parts shard writes while it maps, map_library())
		b.writes_pending.fetch_sub(1);
	}

	// ---- after the lanes' threads have ended ----
	void finish()
	{
		feed.wait_writes_done(batches);
		if (packer) packer->finish();              // (the caller's own reader and writer may continue behind the stream's last chunk)
		if (packer) { st.bgzf_device_bytes += packer->device_bytes(); st.bgzf_host_bytes += packer->host_bytes(); }
		src.m1.pos = feed.pos[0];
		if (src.sep) src.m2.pos = feed.pos[1];
	}
	void report()
	{
		for (int i = 0; i < LaneTimers::kSteps; ++i) st.lane_seconds[i] += timers.seconds(i);
		st.lanes = K;
		if (verbose)
			fprintf(stdout, "stream: lane-thread seconds (summed over %d lanes): waiting for the lane %.3f | read + upload %.3f | waiting for the parse before %.3f | parse %.3f | map (device) %.3f | host reads %.3f\n", K,
			        timers.seconds(LaneTimers::kWaitLane), timers.seconds(LaneTimers::kReadUpload), timers.seconds(LaneTimers::kWaitParse), timers.seconds(LaneTimers::kParse),
			        timers.seconds(LaneTimers::kMap), timers.seconds(LaneTimers::kHostReads));
		kg_stream_timing_t t{};
		if (!sb.timing(t, true) || t.batches <= 0) return;
		add_timing(st.device, t);
		if (verbose)
			fprintf(stdout, "device stream: %lld batches, %lld reads | stage ms (summed over lanes, stages of different lanes overlap): parse %.1f, seed %.1f (search_kernel %.2f in %lld launches, %.1f useful MB), chain %.1f, align %.1f, format %.1f, copy-out %.1f | text in %.1f MB, out %.1f MB\n",
			        (long long)t.batches, (long long)t.reads, t.parse_ms, t.seed_ms, t.search_kernel_ms, (long long)t.search_kernel_launches, t.search_useful_bytes / 1e6, t.chain_ms, t.align_ms,
			        t.format_ms, t.copy_ms, t.text_in_bytes / 1e6, t.text_out_bytes / 1e6);
	}
};

// Maps the library in `src` from its current positions.  Returns true when the stream mapped everything; false when it stopped
// in front of input the device parser does not take (src.m1.pos / src.m2.pos then name where the caller's own reader continues;
// everything before has been committed and written).
bool map_library_stream(Ctx &cx, Source &src, StreamBackend &sb, Writer *writer, Stats &st, RunTotals &tot, std::atomic<int> &est_latest,
                        std::vector<DeferredChunk> *held, int64_t &bytes_out, int64_t ramp_from, const Shard *shard)
{
	StreamRun run(cx, src, sb, writer, st, tot, est_latest, held, bytes_out, shard);
	run.prime(ramp_from);
	// (seeding groups: every lane of a group takes part in every round -- with a batch, or by saying that it has none)
	for (int l = 0; l < run.K; ++l) sb.group_absent(l, 0);
	std::vector<std::thread> threads;
	for (int l = 0; l < run.K; ++l) threads.emplace_back([&run, l]() { run.lane_thread(l); });
	run.commit();
	for (std::thread &t : threads) t.join();
	run.finish();
	run.report();
	return !run.feed.fallback;
}
