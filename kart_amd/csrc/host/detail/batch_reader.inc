// host/detail/batch_reader.inc -- a batch of chunks from the input files (GetNextChunk, src/GetData.cpp:51-219): the run's totals, the Batch, gz / BGZF text,
// the Source of a library, the parallel materialisation of the reads, read_batch().
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
struct RunTotals {
	int64_t iPaired = 0, iDistance = 0;   // src/Mapping.cpp:13,20
	int64_t dev_reads = 0, host_reads = 0;   // reads whose report came from the device / was made here
	double t_read = 0, t_encode = 0, t_seed = 0, t_a = 0, t_nw = 0, t_c = 0, t_commit = 0, t_drain = 0, t_lib = 0, t_format = 0;   // KART_AMD_VERBOSE stage timers
	double t_long_wait = 0;                           // long reads: the main loop waiting for a batch's device report
	double t_shard_wait = 0, t_shard_settle = 0;     // a deferred shard: waiting for the totals of the shard before it, settling its own chunks against them
	WriterTimes writer;                               // where the writer drain (t_drain) went, and the windows unmapped during the run
};

struct Batch {
	std::vector<Read> reads;
	std::vector<ChunkState> chunks;
	uint8_t *enc = nullptr;                         // the read characters, concatenated (encoded on the device); KernelBackend::host_alloc
	size_t enc_capacity = 0;
	KernelBackend *enc_owner = nullptr;
	~Batch() { if (enc) enc_owner->host_free(enc); }
	void reserve_enc(KernelBackend &k, size_t bytes)
	{
		if (bytes <= enc_capacity) return;
		if (enc) enc_owner->host_free(enc);
		enc_capacity = bytes + bytes / 8 + 4096;
		enc_owner = &k;
		enc = (uint8_t *)k.host_alloc(enc_capacity);
		if (!enc) { fprintf(stderr, "Error! out of memory for a batch of reads\n"); exit(1); }
	}
	std::vector<int64_t> off;
	std::vector<int64_t> cand_off;                  // per-read candidate ranges of this batch (filled by the seeding + chaining stage)
	std::vector<int32_t> n_cands;                   // chaining results of this batch (kg_candidates_batch)
	std::vector<kg_candidate> own_cands;            // storage a backend may use for ...
	std::vector<kg_seed> own_seeds;
	const kg_candidate *cands = nullptr;            // ... the candidates of the batch (else the backend's own rotating arrays)
	const kg_seed *cand_seeds = nullptr;
	std::deque<OwnedRead> owned;                    // storage behind the views (getline()/gzgets() readers)
	std::vector<char> text1, text2;                 // inflated FASTQ text behind the views (gz files)
	std::vector<RecView> views;                     // the records of the batch as views into the input (mapped / inflated text)
	const kg_aln_record *records = nullptr;         // the device's per-read report (KernelBackend::align), null when the host maps everything
	const char *cigar_pool = nullptr;               // ... and, for long reads, the CIGAR strings its records point into (KernelBackend::align_long)
	std::vector<kg_chunk_stats> chunk_dev;
	std::shared_future<void> long_fut;              // long reads: the device report of this batch, running on its own thread (device_stage); get() before the records are read
	int est_dev = 0;                                // the EstDistance the device stage speculated with
	bool eof = false;
	double seconds = 0, seed_seconds = 0;
};
std::atomic<int64_t> g_read_ns{0};   // KART_AMD_VERBOSE: total time of read_batch() ...
std::atomic<int64_t> g_read_part_ns[4];   // ... and of its parts: line index, views, chunk assembly, materialise + characters

// gzipped FASTQ: the text is inflated a batch at a time (both mate files in parallel) into buffers the batch owns and then
// parsed by the same view code as a mapped file; what is left after the last whole chunk is carried into the next batch
//
// A BGZF file (bgzip, SAMv1 4.1: a series of gzip members of at most 64 KB, each carrying its compressed size in a 'BC' extra field)
// is what gzgets() reads as one stream in the reference (src/GetData.cpp:145-219) -- and what can be inflated member by member on
// several threads, which a plain gzip stream cannot: one thread inflates FASTQ text at ~0.3 GB/s (~0.9 M records/s per mate file,
// DESIGN §7e) against 40 M reads/s of mapping.  The members' headers are walked one after the other (18 bytes each), the members of a
// batch inflated side by side straight into the batch's text at the offsets their ISIZE fields add up to, CRC-checked like gzread() does.
// A member that is not BGZF-shaped (a plain gzip member appended to the file) hands the rest of the file to gzread() at that offset.
struct GzText {
	gzFile f = nullptr;
	std::vector<char> carry;
	bool eof = false;
	double bytes_per_record = 0;
	std::string path;          // (for replay())
	uint64_t delivered = 0;    // bytes of text handed out so far
	// BGZF
	gzFile own = nullptr;      // the stream hand_over() / replay() opened (f is the caller's otherwise)
	GzText() = default;
	GzText(const GzText &) = delete;
	GzText &operator=(const GzText &) = delete;
	~GzText() { close_bgzf(); if (own) gzclose(own); }
	int fd = -1;               // >= 0: the file is read member by member from `pos`
	off_t pos = 0;
	int threads = 1;
	std::vector<unsigned char> packed;
	struct Member { size_t in, hdr, csize, isize, out; };

	// the member that starts at h[0..n): total size (BSIZE + 1) and header length, false when it is not a BGZF member
	static bool member_shape(const unsigned char *h, size_t n, size_t &csize, size_t &hdr)
	{
		if (n < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return false;
		if (h[3] & ~4) return false;                                   // name / comment / header CRC: not what bgzip writes
		const size_t xlen = (size_t)h[10] | ((size_t)h[11] << 8);
		if (12 + xlen > n) return false;
		for (size_t at = 12; at + 4 <= 12 + xlen;) {
			const size_t slen = (size_t)h[at + 2] | ((size_t)h[at + 3] << 8);
			if (h[at] == 'B' && h[at + 1] == 'C' && slen == 2 && at + 6 <= 12 + xlen) {
				csize = ((size_t)h[at + 4] | ((size_t)h[at + 5] << 8)) + 1;
				hdr = 12 + xlen;
				return csize >= hdr + 8;
			}
			at += 4 + slen;
		}
		return false;
	}
	// true: `path` starts with a BGZF member and is read that way from now on (f stays open for the hand-over described above)
	bool try_bgzf(const char *path, int n_threads)
	{
		if (getenv("KART_AMD_NO_BGZF")) return false;
		int d = ::open(path, O_RDONLY);
		if (d < 0) return false;
		unsigned char h[64];
		ssize_t n = ::pread(d, h, sizeof(h), 0);
		size_t csize = 0, hdr = 0;
		if (n < 18 || !member_shape(h, (size_t)n, csize, hdr)) { ::close(d); return false; }
		fd = d; pos = 0; threads = std::max(1, n_threads);
		return true;
	}
	void close_bgzf() { if (fd >= 0) ::close(fd); fd = -1; }
	// the rest of the file through gzread(): a gzFile of its own on the descriptor, positioned at the member that did not fit
	void hand_over()
	{
		int d = dup(fd);
		close_bgzf();
		if (d < 0 || lseek(d, pos, SEEK_SET) < 0) { if (d >= 0) ::close(d); eof = true; return; }
		own = gzdopen(d, "rb");
		if (!own) { ::close(d); eof = true; return; }
		gzbuffer(own, 1 << 20);
		f = own;
	}
	// -fz device: the members are inflated by the device (mapper.hpp) instead of the zlib threads; gone again once a run() of it fails
	std::unique_ptr<MemberInflater> inflater;
	bool silent = false;
	int64_t device_bytes = 0, host_bytes = 0;      // text of BGZF members the device / zlib inflated
	double device_ms = 0;
	void drop_inflater(const char *why)
	{
		if (!silent) fprintf(stderr, "Warning! %s: zlib inflates the rest of [%s]\n", why, path.c_str());
		device_ms += inflater->device_ms();
		inflater.reset();
	}
	void fill_bgzf(std::vector<char> &buf, size_t want)
	{
		const size_t at = buf.size();
		// 1. the members that hold the next `want` bytes of text: one read of their span (into the inflater's page-locked buffer where there is one),
		// then a walk over the headers
		std::vector<Member> mem;
		size_t total = 0, span = 0;
		bool foreign = false;
		unsigned char *pk = nullptr;         // the span's bytes: pk[0, have)
		size_t have = 0;
		packed.clear();
		auto room = [&](size_t bytes) {
			if (inflater) {
				if (unsigned char *p = inflater->src(bytes)) { pk = p; return; }
				packed.assign(pk, pk + have);
				drop_inflater("no page-locked memory for the members");
			}
			packed.resize(bytes);
			pk = packed.data();
		};
		while (total < want && !eof && !foreign) {
			const size_t guess = std::max<size_t>((size_t)1 << 20, (want - total) / 3);          // (FASTQ text packs ~3-5x)
			room(have + guess);
			ssize_t n = ::pread(fd, pk + have, guess, pos + (off_t)have);
			have += n > 0 ? (size_t)n : 0;
			const bool end_of_file = n <= 0 || (size_t)n < guess;
			while (total < want) {
				size_t csize = 0, hdr = 0;
				const size_t left = have - span;
				if (left == 0) { if (end_of_file) eof = true; break; }
				if (left < 18 || !member_shape(pk + span, left, csize, hdr)) {
					if (left >= 18 || end_of_file) foreign = true;      // not a BGZF member (or a truncated one): gzread() decides what it is
					break;
				}
				if (csize > left) { if (end_of_file) foreign = true; break; }
				const unsigned char *t = pk + span + csize - 4;
				Member m;
				m.in = span; m.hdr = hdr; m.csize = csize;
				m.isize = (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16) | ((size_t)t[3] << 24);
				m.out = total;
				if (m.isize > 65536) { foreign = true; break; }
				mem.push_back(m);
				total += m.isize; span += csize;
			}
			if (end_of_file) break;
		}
		// 2. inflate them: the device, else the zlib threads side by side
		buf.resize(at + total);
		size_t bad = mem.size();
		bool on_device = false;
		if (inflater && !mem.empty()) {
			std::vector<int64_t> member_off(mem.size() + 1), text_off(mem.size() + 1);
			for (size_t k = 0; k < mem.size(); ++k) { member_off[k] = (int64_t)mem[k].in; text_off[k] = (int64_t)mem[k].out; }
			member_off[mem.size()] = (int64_t)span; text_off[mem.size()] = (int64_t)total;
			const unsigned char *text = nullptr;
			const int32_t *status = nullptr;
			if (inflater->run(span, member_off.data(), text_off.data(), mem.size(), text, status)) {
				on_device = true;
				for (size_t k = 0; k < mem.size(); ++k)
					if (status[k] != KG_INFLATE_OK) { bad = k; break; }
				const size_t sound = bad < mem.size() ? mem[bad].out : total;
				if (sound) memcpy(buf.data() + at, text, sound);
				device_bytes += (int64_t)sound;
			} else {
				packed.assign(pk, pk + have);      // (the members lie in the inflater's buffer, which goes with it)
				pk = packed.data();
				drop_inflater("the device did not inflate a round of members");
			}
		}
		if (!on_device) {
			std::atomic<size_t> next{0}, first_bad{mem.size()};
			auto work = [&]() {
				z_stream z;
				memset(&z, 0, sizeof(z));
				if (inflateInit2(&z, -15) != Z_OK) { first_bad.store(0); return; }
				for (size_t k; (k = next.fetch_add(1)) < mem.size();) {
					const Member &m = mem[k];
					const unsigned char *in = pk + m.in;
					inflateReset(&z);
					z.next_in = const_cast<unsigned char *>(in + m.hdr);
					z.avail_in = (uInt)(m.csize - m.hdr - 8);
					z.next_out = (unsigned char *)buf.data() + at + m.out;
					z.avail_out = (uInt)m.isize;
					int rc = inflate(&z, Z_FINISH);
					const unsigned char *t = in + m.csize - 8;
					const uLong want_crc = (uLong)t[0] | ((uLong)t[1] << 8) | ((uLong)t[2] << 16) | ((uLong)t[3] << 24);
					bool good = rc == Z_STREAM_END && z.avail_out == 0 && z.avail_in == 0 &&
					            crc32(crc32(0L, Z_NULL, 0), (const unsigned char *)buf.data() + at + m.out, (uInt)m.isize) == want_crc;
					if (!good) { size_t cur = first_bad.load(); while (k < cur && !first_bad.compare_exchange_weak(cur, k)) {} }
				}
				inflateEnd(&z);
			};
			const size_t nt = std::min<size_t>((size_t)threads, std::max<size_t>(1, mem.size() / 8));
			std::vector<std::thread> th;
			for (size_t t = 1; t < nt; ++t) th.emplace_back(work);
			work();
			for (std::thread &x : th) x.join();
			bad = first_bad.load();
			host_bytes += (int64_t)(bad < mem.size() ? mem[bad].out : total);
		}
		if (bad < mem.size()) {
			// a damaged member: gzread() takes over AT it and delivers exactly what the reference's gzgets() loop would still see
			// (the bytes before the damage, then the end of the library)
			buf.resize(at + mem[bad].out);
			close_bgzf();
			replay(buf, delivered + mem[bad].out);
			return;
		}
		pos += (off_t)span;
		if (foreign && !eof) {
			hand_over();
			if (!eof && total < want) {
				delivered += total;            // (fill() counts from where the text stands now)
				fill(buf, want - total);
			}
		}
	}
	// The stream is damaged somewhere ahead.  What the reference still sees of it is what gzgets() delivers: everything zlib's own
	// 16 KB output buffer took in whole before the error (src/GetData.cpp:145-219 reads through it line by line) -- which a large
	// gzread() does not tell (it fails as a whole).  So: the file once more from its start, default buffers, small reads; the first
	// `skip` bytes are the ones already handed out, whatever follows them until the error is the rest of the library.
	void replay(std::vector<char> &buf, uint64_t skip)
	{
		eof = true;
		struct stat sb;
		if (stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return;      // (a pipe cannot be read twice: the library ends at the damage)
		// a failing gzread() drops what it had copied before it failed: find the last offset small reads reach, then go there again
		// and finish byte by byte (error path: the file is inflated up to three times)
		uint64_t reach = 0;
		for (int pass = 0; pass < 2; ++pass) {
			gzFile g = gzopen(path.c_str(), "rb");
			if (!g) return;
			char chunk[4096];
			uint64_t seen = 0;
			auto take = [&](int n) {
				if (pass == 1 && seen + (uint64_t)n > skip) {
					const size_t from = seen >= skip ? 0 : (size_t)(skip - seen);
					buf.insert(buf.end(), chunk + from, chunk + n);
				}
				seen += (uint64_t)n;
			};
			for (;;) {
				if (pass == 1 && seen >= reach) break;
				size_t ask = sizeof(chunk);
				if (pass == 1 && reach - seen < ask) ask = (size_t)(reach - seen);
				int n = gzread(g, chunk, (unsigned)ask);
				if (n <= 0) break;
				take(n);
			}
			if (pass == 0) reach = seen;
			else
				for (;;) {
					int n = gzread(g, chunk, 1);
					if (n <= 0) break;
					take(n);
				}
			gzclose(g);
		}
	}
	// an ordinary gzip file on several threads (detail/pgzip.inc); whatever that reader declines, zlib continues at the byte reached
	Pgz pgz;
	bool try_pgz(const char *p, int n_threads) { return fd < 0 && pgz.open(p, n_threads); }
	// the parallel reader has declined the rest: one zlib stream from text byte `offset` on (it inflates up to there once more to get there).
	// false: that stream cannot get there either (the caller replays)
	bool pgz_to_zlib(uint64_t offset)
	{
		pgz.close();
		own = gzopen(path.c_str(), "rb");
		if (!own) { eof = true; return true; }
		gzbuffer(own, 1 << 20);
		f = own;
		return gzseek(own, (z_off_t)offset, SEEK_SET) >= 0;
	}
	void fill_pgz(std::vector<char> &buf, size_t want)
	{
		const size_t at = buf.size();
		buf.resize(at + want);
		const size_t take = pgz.read(buf.data() + at, want);
		buf.resize(at + take);
		if (take == want) return;
		if (pgz.all_done) { eof = true; return; }
		if (!pgz_to_zlib(delivered + take)) { replay(buf, delivered + take); return; }
		if (eof) return;
		delivered += take;
		fill(buf, want - take);
	}
	// Text straight to dst (the growing block of GzProducer): up to `cap` bytes, at least one round of the parallel reader when that one is at
	// work.  0 without eof: the source has changed (the parallel reader declined), ask again.
	size_t fill_direct(char *dst, size_t cap)
	{
		if (fd < 0 && pgz.active) {
			size_t n = 0;
			if (pgz.ready_bytes()) n = pgz.read_ready(dst, cap);
			else if (!pgz.all_done) pgz.round(dst, cap, &n);
			delivered += n;
			if (n) return n;
			if (pgz.ready_bytes()) return fill_direct(dst, cap);          // (the round did not fit dst: it is in the reader's own buffer)
			if (pgz.all_done) { eof = true; return 0; }
			if (!pgz_to_zlib(delivered)) {
				std::vector<char> rest;
				replay(rest, delivered);
				const size_t m = std::min(cap, rest.size());                  // (what a damaged stream still yields: far below any cap)
				memcpy(dst, rest.data(), m);
				delivered += m;
				return m;
			}
			return 0;
		}
		std::vector<char> tmp;
		fill(tmp, std::min(cap, (size_t)64 << 20));
		if (!tmp.empty()) memcpy(dst, tmp.data(), tmp.size());
		return tmp.size();
	}
	void fill(std::vector<char> &buf, size_t want)
	{
		const size_t at = buf.size();
		const uint64_t base = delivered;
		if (fd >= 0) fill_bgzf(buf, want);
		else if (pgz.active) fill_pgz(buf, want);
		else {
			size_t got = 0;
			buf.resize(at + want);
			bool damaged = false;
			while (got < want) {
				int n = gzread(f, buf.data() + at + got, (unsigned)std::min<size_t>(want - got, (size_t)64 << 20));
				if (n < 0) damaged = true;
				if (n <= 0) { eof = true; break; }
				got += (size_t)n;
			}
			buf.resize(at + got);
			if (damaged && !path.empty()) replay(buf, base + got);
		}
		delivered = base + (buf.size() - at);
	}
};

// The inflated text of a gz library as ONE growing block of memory, written by a thread of its own (GzText::fill(): the several-thread
// reader, BGZF members, zlib, and what gzgets() still delivers of a damaged stream -- all as before), so that the device's FASTQ-in / SAM-out
// stream (stream.inc) can take gz input the way it takes a mapped plain file: a block after the other, by offset.  The block is address
// space only (MAP_NORESERVE, the size no deflate stream can exceed where that fits): pages come as the text does and go (release()) once
// every batch that reads them is committed; the writer stays at most `ahead` bytes in front of that.
struct GzProducer : GrowingText {
	GzText *g = nullptr;
	char *base = nullptr;
	size_t reserve = 0;
	std::mutex mu;
	std::condition_variable cv;
	size_t produced = 0, released = 0, demand = 0;      // demand: the furthest byte a reader waits for (the look-ahead never keeps the writer from getting there)
	bool ended = false, stop_flag = false, overflow = false;
	size_t ahead = (size_t)3 << 30;
	size_t freed = 0;                 // pages in front of this byte have been given back (by the janitor thread: release() only says up to where)
	std::thread th, janitor;
	~GzProducer() override { stop(); if (base) munmap(base, reserve); }
	bool start(GzText *gz, size_t packed_bytes)
	{
		g = gz;
		if (const char *e = getenv("KART_AMD_GZ_AHEAD_MB")) ahead = std::max<size_t>(64, (size_t)atoll(e)) << 20;
		// deflate cannot expand beyond 1032 : 1; less address space than that (very large files) still holds any FASTQ text (3-10 : 1)
		size_t want = std::max<size_t>((size_t)2 << 30, std::min<size_t>((size_t)32 << 40, packed_bytes * 1032 + ((size_t)64 << 20)));
		for (; want >= std::max<size_t>((size_t)2 << 30, packed_bytes * 16); want /= 2) {
			void *p = mmap(nullptr, want, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
			if (p != MAP_FAILED) { base = (char *)p; reserve = want; break; }
		}
		if (!base) return false;
		if (!getenv("KART_AMD_GZ_NO_THP")) madvise(base, reserve, MADV_HUGEPAGE);   // (2 MB pages for the text: 40 M reads in 2.04 s against 2.30 s with 4 KB pages, profiles/r06w)
		th = std::thread([this]() { run(); });
		janitor = std::thread([this]() { give_back(); });
		return true;
	}
	// the pages in front of `released` go back to the system on a thread of their own: madvise() of a batch's ~200 MB takes milliseconds, and the
	// caller of release() is the in-order commit
	void give_back()
	{
		const size_t page = 4096;
		std::unique_lock<std::mutex> lk(mu);
		for (;;) {
			cv.wait(lk, [&]() { return stop_flag || released > freed; });
			if (stop_flag) return;
			const size_t to = released, a = (freed + page - 1) / page * page, b = to / page * page;
			lk.unlock();
			if (b > a) madvise(base + a, b - a, MADV_DONTNEED);
			lk.lock();
			freed = to;
		}
	}
	void run()
	{
		for (;;) {
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&]() { return stop_flag || produced - released < ahead || produced < demand; });
				if (stop_flag) return;
			}
			// (a round of the several-thread reader is ~190 MB of text; whatever source: less room than 512 MB ends this way of reading)
			if (g->eof || reserve - produced < ((size_t)512 << 20)) {
				std::lock_guard<std::mutex> lk(mu);
				overflow = !g->eof;
				ended = true;
				cv.notify_all();
				return;
			}
			const size_t n = g->fill_direct(base + produced, reserve - produced);
			std::lock_guard<std::mutex> lk(mu);
			produced += n;
			if (g->eof) ended = true;
			cv.notify_all();
			if (g->eof) return;
		}
	}
	void stop()
	{
		{
			std::lock_guard<std::mutex> lk(mu);
			stop_flag = true;
		}
		cv.notify_all();
		if (th.joinable()) th.join();
		if (janitor.joinable()) janitor.join();
	}
	size_t wait_for(size_t upto, bool &end_seen) override
	{
		std::unique_lock<std::mutex> lk(mu);
		if (upto > demand) { demand = upto; cv.notify_all(); }
		cv.wait(lk, [&]() { return produced >= upto || ended; });
		end_seen = ended;
		return produced;
	}
	void release(size_t below) override
	{
		std::lock_guard<std::mutex> lk(mu);
		if (below > produced) below = produced;
		if (below <= released) return;
		released = below;
		cv.notify_all();
	}
};

struct Source {
	bool gzstream = false;     // a gz library on its way through the device stream: m1 / m2 are the growing texts of p1 / p2
	size_t gz_packed[2] = {0, 0};
	bool sep = false, fast = false, gzfast = false;
	bool fasta_fast = false;   // plain FASTA: m1 / m2 map the files for the device stream; the getline() reader continues wherever that one stops
	double rec_bytes = 400;          // text bytes per record and file, as the batches so far found them (what the parallel line index is sized by)
	Input in1, in2;            // getline()/gzgets() readers (FASTA, gz)
	MappedFile m1, m2;         // mapped plain FASTQ, or the inflated text of the current batch
	GzText g1, g2;
	std::unique_ptr<GzProducer> p1, p2;    // (behind g1 / g2: their threads end before the readers they draw from go away)
	// gz library -> device stream: a thread per file inflates into a growing block, m1 / m2 show it to the stream as they show a mapped plain file
	bool gz_stream_begin()
	{
		const int nf = sep ? 2 : 1;
		for (int f = 0; f < nf; ++f) {
			GzText &g = f ? g2 : g1;
			struct stat sb;
			if (stat(g.path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return false;       // (a pipe: the general reader)
			gz_packed[f] = (size_t)sb.st_size;
		}
		for (int f = 0; f < nf; ++f) {
			std::unique_ptr<GzProducer> &p = f ? p2 : p1;
			p.reset(new GzProducer());
			if (!p->start(f ? &g2 : &g1, gz_packed[f])) { gz_stream_end(); return false; }
			MappedFile &m = f ? m2 : m1;
			m = MappedFile();
			m.grow = p.get(); m.data = p->base; m.size = m.map_size = 0; m.pos = 0; m.gz_lines = true;
		}
		gzstream = true;
		return true;
	}
	// ... and back: whatever the stream has not consumed (all of it behind m1.pos / m2.pos that exists) becomes the text the gz reader starts its
	// next batch with (GzText::carry) -- it goes on inflating behind that, and it is the one that knows what to do with records gzgets() reads differently
	void gz_stream_end()
	{
		for (int f = 0; f < 2; ++f) {
			std::unique_ptr<GzProducer> &p = f ? p2 : p1;
			if (!p) continue;
			p->stop();
			MappedFile &m = f ? m2 : m1;
			GzText &g = f ? g2 : g1;
			if (p->base && p->produced > m.pos) g.carry.assign(p->base + m.pos, p->base + p->produced);
			m = MappedFile();
			p.reset();
		}
		gzstream = false;
	}
};

// the reads of a batch from its views (or from the owned records of the line-by-line readers), and their characters
// concatenated for the seeding call
template <class PoolT>
void materialise_batch(PoolT &pool, Batch &b, bool by_views, KernelBackend &kern)
{
	// The reads of the batch, concatenated, as characters: EnCodeReadSeq (src/Mapping.cpp:482-485) itself runs on the device
	// (KG_INPUT_ASCII).  The reference encodes mate 2 with mate 1's length (:550, App. B-5); with equal-length mates that is the
	// same thing, otherwise it reads or leaves uninitialised bytes -- here every read is taken over its own length.
	std::vector<RecView> &views = b.views;
	std::vector<Read> &reads = b.reads;
	if (by_views) {
		reads.resize(views.size());
		b.off.resize(views.size() + 1);
		b.off[0] = 0;
		for (size_t i = 0; i < views.size(); ++i) b.off[i + 1] = b.off[i] + views[i].rlen;
		b.reserve_enc(kern, (size_t)b.off[views.size()] + 64);
		pool.run((int)((views.size() + 2047) / 2048), [&](int blk) {       // one pass: the Read and its characters
			size_t lo = (size_t)blk * 2048, hi = std::min(views.size(), lo + 2048);
			for (size_t i = lo; i < hi; ++i) materialise(views[i], reads[i], (char *)b.enc + b.off[i]);
		});
		return;
	}
	reads.resize(b.owned.size());
	for (size_t i = 0; i < b.owned.size(); ++i) {
		const OwnedRead &o = b.owned[i];
		Read &rd = reads[i];
		rd = Read();
		rd.name = o.name; rd.seq = o.seq; rd.qual = o.qual; rd.rlen = o.rlen;
		rd.raw = o.raw;
	}
	b.off.assign(reads.size() + 1, 0);
	for (size_t i = 0; i < reads.size(); ++i) b.off[i + 1] = b.off[i] + reads[i].rlen;
	b.reserve_enc(kern, (size_t)b.off[reads.size()] + 64);
	pool.run((int)((reads.size() + 4095) / 4096), [&](int blk) {
		size_t lo = (size_t)blk * 4096, hi = std::min(reads.size(), lo + 4096);
		for (size_t i = lo; i < hi; ++i) memcpy(b.enc + b.off[i], reads[i].seq.data(), (size_t)reads[i].rlen);
	});
}

// reads `batch_chunks` whole chunks (GetNextChunk each); runs on the prefetch thread
// The inflated text of a gz library is parsed through the same line index and views as a mapped file.  That is what the reference's
// gzGetNextEntry (src/GetData.cpp:145-182) reads as long as (a) every line fits its gzgets() buffer -- 1000 bytes, 1000000 with
// -pacbio: a longer line comes back in pieces and the pieces are taken for the record's next lines -- and (b) every record starts
// with '@' or '>' (:162; otherwise the entry ends after that one line).  A window that breaks either rule is left to the line reader
// (next_entry_gz), which restates those calls one by one.
bool gz_text_regular(const MappedFile &f, size_t buf_size)
{
	const size_t limit = buf_size - 1;                      // gzgets() stores at most buf_size - 1 characters
	const std::vector<size_t> &le = f.line_end;
	size_t from = f.pos;
	for (size_t i = 0; i < le.size(); ++i) {
		if (le[i] - from > limit) return false;
		if ((i & 3) == 0) {
			const char c = f.data[from];
			if ((c != '@' && c != '>') || header_view(f.data + from, (int)(le[i] - from)).empty()) return false;
		}
		from = le[i];
	}
	return f.size - from <= limit;                          // (the unfinished line at the end of the window)
}

// the line reader of a gz library from the first byte nobody has taken yet: `unparsed` bytes in front of what the inflater has delivered
// (a fresh stream with zlib's default buffers, as the reference opens it: what gzgets() still delivers of a damaged
//  stream depends on them, and the one in use may have failed under gzread() already)
bool gz_reopen_for_lines(Input &in, GzText &g, size_t unparsed)
{
	gzFile f = gzopen(g.path.c_str(), "rb");
	if (!f) return false;
	if (g.f == in.gz) g.f = nullptr;
	if (in.gz) gzclose(in.gz);
	in.gz = f;
	return gzseek(f, (z_off_t)(g.delivered - unparsed), SEEK_SET) >= 0;
}

void read_batch(const Ctx &cx, Source &src, int64_t batch_chunks, int chunk_limit, Pool &pool, Batch &b)
{
	double t0 = now_s();
	b.reads.clear(); b.chunks.clear(); b.owned.clear(); b.eof = false;
	std::vector<RecView> &views = b.views;
	views.clear();
	int64_t parse_chunks = batch_chunks;
	if (src.gzfast && !cx.fastq) {
		// gz FASTA: the inflater serves the device stream only.  What that one left (GzText::carry, Source::gz_stream_end) is the line reader's --
		// nothing, normally: the library ended with the stream
		const bool all1 = src.g1.eof && src.g1.delivered > 0 && src.g1.carry.empty(), all2 = !src.sep || (src.g2.eof && src.g2.delivered > 0 && src.g2.carry.empty());
		if (all1 && all2) src.in1.ended = src.in2.ended = true;
		else if (!gz_reopen_for_lines(src.in1, src.g1, src.g1.carry.size()) || (src.sep && !gz_reopen_for_lines(src.in2, src.g2, src.g2.carry.size())))
			run_fail("cannot reposition the gz input for its line reader");
		src.gzfast = false;
		src.g1.close_bgzf(); src.g2.close_bgzf();
		src.g1.carry.clear(); src.g2.carry.clear();
	}
	if (src.gzfast) {
		const size_t recs_per_file = (size_t)batch_chunks * (size_t)chunk_limit / (src.sep ? 2 : 1);
		b.text1.swap(src.g1.carry); src.g1.carry.clear();
		b.text2.swap(src.g2.carry); src.g2.carry.clear();
		auto want = [&](const GzText &g, const std::vector<char> &t) {
			size_t est = (size_t)((double)recs_per_file * (g.bytes_per_record > 0 ? g.bytes_per_record * 1.03 : 360.0)) + (1 << 16);
			return est > t.size() ? est - t.size() : (size_t)0;
		};
		size_t need1 = want(src.g1, b.text1), need2 = src.sep ? want(src.g2, b.text2) : 0;
		for (;;) {
			std::future<void> other;
			if (src.sep && !src.g2.eof && need2) other = std::async(std::launch::async, [&]() { src.g2.fill(b.text2, need2); });
			if (!src.g1.eof && need1) src.g1.fill(b.text1, need1);
			if (other.valid()) other.get();
			// the mate files end together or not at all: once one is exhausted the rest of the other is needed
			if (src.sep && src.g1.eof != src.g2.eof) {
				GzText &g = src.g1.eof ? src.g2 : src.g1;
				std::vector<char> &t = src.g1.eof ? b.text2 : b.text1;
				while (!g.eof) g.fill(t, (size_t)64 << 20);
			}
			src.m1.gz_lines = src.m2.gz_lines = true;
			src.m1.attach(b.text1.data(), b.text1.size());
			src.m1.index_ahead(pool, b.text1.size());
			size_t recs1 = src.m1.line_end.size() / 4, recs2 = 0;
			if (src.sep) {
				src.m2.attach(b.text2.data(), b.text2.size());
				src.m2.index_ahead(pool, b.text2.size());
				recs2 = src.m2.line_end.size() / 4;
			}
			const size_t gz_buf = cx.opt.pacbio ? 1000000 : 1000;
			if (!gz_text_regular(src.m1, gz_buf) || (src.sep && !gz_text_regular(src.m2, gz_buf))) {
				// the rest of the library line by line, from the first byte no chunk has taken yet (nothing of this window has been parsed)
				if (!gz_reopen_for_lines(src.in1, src.g1, b.text1.size()) || (src.sep && !gz_reopen_for_lines(src.in2, src.g2, b.text2.size())))
					run_fail("cannot reposition the gz input for its line reader");
				src.gzfast = false;
				src.g1.close_bgzf(); src.g2.close_bgzf();
				b.text1.clear(); b.text2.clear();
				break;
			}
			bool final = src.g1.eof && (!src.sep || src.g2.eof);
			if (final) break;                               // everything is in memory: parse to the end
			size_t reads_avail = src.sep ? 2 * std::min(recs1, recs2) : (recs1 & ~(size_t)1);
			parse_chunks = std::min<int64_t>(batch_chunks, (int64_t)(reads_avail / (size_t)chunk_limit));
			if (parse_chunks >= 1) break;
			need1 = need2 = std::max<size_t>((size_t)1 << 20, recs_per_file * 64);   // not even one whole chunk yet: more text
		}
	}
	if (src.fast) {
		// roughly the bytes this batch will consume(header + 2 x read + "+"), indexed in parallel
		// (sized by the records seen so far: with 400 bytes per record -- short reads -- a batch of 7 kb reads had 3 % of its text indexed in parallel and
		//  the rest walked line by line on this one thread, 2.4 of the 4.4 s of a 2 M-read run, profiles/r05zb_ab_long_2m.log)
		size_t per_file = (size_t)((double)batch_chunks * (double)chunk_limit * src.rec_bytes * 1.05) / (src.sep ? 2 : 1) + (1 << 20);
		src.m1.index_ahead(pool, per_file);
		if (src.sep) src.m2.index_ahead(pool, per_file);
	}
	const size_t pos_before = src.fast ? src.m1.pos : 0;
	double t1 = now_s();
	g_read_part_ns[0] += (int64_t)((t1 - t0) * 1e9);
	const bool by_views = src.fast || src.gzfast;
	if (by_views) {
		// whole chunks straight from the line index (GetNextChunk's loop over precomputed views); whatever the index does
		// not cover -- the tail of a file, a last line without newline -- is left to the line-by-line walk below
		std::vector<RecView> v1, v2;
		views_of_indexed_records(pool, src.m1, v1);
		if (src.sep) views_of_indexed_records(pool, src.m2, v2);
		g_read_part_ns[1] += (int64_t)((now_s() - t1) * 1e9);
		size_t i1 = 0, i2 = 0;
		const size_t per_chunk = src.sep ? (size_t)(chunk_limit + 1) / 2 : (size_t)chunk_limit + 1;   // records a chunk can take from a file
		while ((int64_t)b.chunks.size() < parse_chunks && i1 + per_chunk <= v1.size() && (!src.sep || i2 + per_chunk <= v2.size())) {
			ChunkState ck;
			ck.begin = (int)views.size();
			int count = 0;
			for (;;) {                                        // next_chunk_views() on the precomputed views
				RecView v = v1[i1++];
				if (v.rlen == 0) break;
				v.flip = false;
				views.push_back(v);
				count++;
				v = src.sep ? v2[i2++] : v1[i1++];
				if (v.rlen == 0) break;
				v.flip = cx.opt.paired;
				views.push_back(v);
				count++;
				if (count == chunk_limit) break;
			}
			ck.count = count;
			if (count == 0) { b.eof = true; break; }          // an empty record first ends the library, as in the walk below
			ck.paired = cx.opt.paired && ck.count % 2 == 0 && !cx.opt.pacbio;
			b.chunks.push_back(std::move(ck));
		}
		auto advance = [](MappedFile &f, size_t recs) {
			if (recs == 0) return;
			f.pos = f.line_end[4 * recs - 1];
			f.next_line = 4 * recs;
		};
		advance(src.m1, i1);
		if (src.sep) advance(src.m2, i2);
	}
	while (!b.eof && (int64_t)b.chunks.size() < parse_chunks) {
		ChunkState ck;
		ck.begin = by_views ? (int)views.size() : (int)b.owned.size();
		ck.count = by_views ? next_chunk_views(cx, src.sep, src.m1, src.m2, views, chunk_limit)
		                    : next_chunk(cx, src.sep, src.in1, src.in2, b.owned, chunk_limit);
		if (ck.count == 0) { b.eof = true; break; }
		ck.paired = cx.opt.paired && ck.count % 2 == 0 && !cx.opt.pacbio;
		b.chunks.push_back(std::move(ck));
	}
	if (src.gzfast) {   // what the parser did not reach belongs to the next batch
		size_t n1 = views.size() / (src.sep ? 2 : 1);
		if (n1 > 0) src.g1.bytes_per_record = (double)src.m1.pos / (double)((views.size() + (src.sep ? 1 : 0)) / (src.sep ? 2 : 1));
		if (src.sep && views.size() > 1) src.g2.bytes_per_record = (double)src.m2.pos / (double)(views.size() / 2);
		src.g1.carry.assign(b.text1.begin() + (std::ptrdiff_t)src.m1.pos, b.text1.end());
		if (src.sep) src.g2.carry.assign(b.text2.begin() + (std::ptrdiff_t)src.m2.pos, b.text2.end());
	}
	if (src.fast && !views.empty()) {
		const size_t recs1 = src.sep ? (views.size() + 1) / 2 : views.size();
		src.rec_bytes = std::max(64.0, (double)(src.m1.pos - pos_before) / (double)recs1);
	}
	double t2 = now_s();
	materialise_batch(pool, b, by_views, cx.kern);
	b.seconds = now_s() - t0;
	g_read_part_ns[2] += (int64_t)((t2 - t1) * 1e9);      // (includes the views part)
	g_read_part_ns[3] += (int64_t)((now_s() - t2) * 1e9);
	g_read_ns += (int64_t)(b.seconds * 1e9);
}
