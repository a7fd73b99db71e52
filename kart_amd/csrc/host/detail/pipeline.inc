// host/detail/pipeline.inc -- one library from its first read to its last SAM byte (ReadMapping, src/Mapping.cpp:488-637): map_library() -- the host reader's batches
// or the device stream's lanes, the in-order commit with the EstDistance replay, the long-read overlap, a shard's settling -- and plan_shard().
// The pieces it is made of: chunk_state.inc (ChunkState, Pool), writer.inc, chunk_stages.inc, batch_reader.inc, deferred.inc, stream.inc.
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
// the Writer's last items, the windows still mapped and the exact size; the parts of its time go to the verbose line
void finish_writer(Writer &w, RunTotals &tot)
{
	w.finish();
	const WriterTimes &t = w.times();
	tot.writer.wait += t.wait; tot.writer.unmap += t.unmap; tot.writer.truncate += t.truncate;
	tot.writer.unmap_beside += t.unmap_beside; tot.writer.windows_beside += t.windows_beside; tot.writer.windows_at_end += t.windows_at_end;
}

void map_library(Ctx &cx, Source &src, FILE *out, Stats &st, RunTotals &tot, Shard &shard, FILE *&shard_out)
{
	const int chunk_limit = cx.opt.pacbio ? 10 : 4000;   // ReadChunkSize, src/structure.h:21; src/GetData.cpp:140
	const int mode = cx.opt.pacbio ? KG_MODE_SENSITIVE : KG_MODE_FAST;
	// -t is the thread budget of the run: with the per-read report on the device the workers only format text, and the reader and
	// writer pools need cores of their own -- 3/4 of the budget works, 1/2 reads, up to four write (see below;
	// more threads than cores only adds context switches under a CPU quota)
	// long reads: the report is the device's as well (kg_longread_batch) unless mate files are given -- those are mapped singly but
	// printed by the paired output function (chunk_stage_c), which needs the host's reports
	const bool dev_long = cx.opt.pacbio && !cx.opt.paired;
	const bool dev_report = !cx.opt.pacbio || dev_long;
	const int nthreads = std::max(1, dev_report && cx.opt.threads >= 8 ? cx.opt.threads * 3 / 4 : cx.opt.threads);
	// Three batches in flight:
	//   prefetch thread : read + encode + seed (GPU) of batch k+1
	//   worker pool     : ONE combined phase -- chain/pair/plan the chunks of batch k, then finish/format the chunks of
	//                     batch k-1, chunk c of either batch on worker c mod n, so whatever a worker allocates for a
	//                     chunk it also frees (no cross-thread frees)
	//   helper thread   : NW kernel call of batch k, overlapping the commit of k-1 and the planning of k+1
	//   main thread     : the in-order commit of batch k-1
	// The speculated EstDistance therefore lags the committed totals by up to two batches; the commit's
	// validity check absorbs that.
	// parsing + encoding costs ~0.4x what the mapping stages cost per read: half as many reader threads keep up
	// (the bulk workers at nice 5: in alternation on one box, 20 M reads, the runs took 1.50-1.77 s (six runs, mean 1.64) against
	//  1.40-2.40 s (ten runs, mean 1.98) at equal priority -- reader, device thread and writers are the critical path)
	static const int worker_nice = getenv("KART_AMD_WORKER_NICE") ? atoi(getenv("KART_AMD_WORKER_NICE")) : 5;
	Pool pool(nthreads, worker_nice), read_pool(std::max(1, getenv("KART_AMD_READER_THREADS") ? atoi(getenv("KART_AMD_READER_THREADS")) : (cx.opt.threads + 1) / 2));
	const bool deferred = shard.deferred();
	std::vector<DeferredChunk> held;                 // deferred shard: everything mapped so far, text included
	std::unique_ptr<Writer> writer;
	int64_t bytes_out = 0;
	if (shard.active() && shard.rank == 0) {         // the header is in the stream buffer: everything after it goes through pwrite
		fflush(out);
		shard.rdv->header_bytes.store((int64_t)ftello(out));
		shard.rdv->out_ready.store(1);
	}
	// Writers: every 4 KB page of the output is a write fault on ONE file's mapping, and those contend -- measured per 20 M reads
	// (6.6 GB of SAM on tmpfs): 4 threads 3.4-3.7 s of system time and 1.42-1.50 s of wall, 6 threads 6.5-13.6 s / 1.8-2.9 s,
	// 12 threads 16-26 s / 2.1-3.1 s (allocating the pages ahead with fallocate from one or two extra threads: no gain).  So: four, shared among the processes of a sharded run (they write into the same file).
	const int writer_cap = 7;                       // (4 until the allocator thread went: in product, 20 M reads per step, no allocator: 4 writers 0.85 s, 5 0.79 s, 6 0.75-0.79 s, 8 0.80 s, 12 0.90 s) per process: every shard has its own cores (the page-fault contention is per file, but a shard's writers must keep up with its own device)
	const int writer_threads = getenv("KART_AMD_WRITER_THREADS") ? std::max(1, atoi(getenv("KART_AMD_WRITER_THREADS")))
	                                                            : std::min(writer_cap, std::max(2, cx.opt.threads * 7 / 16));
	// (a sharded run's file is cut to its exact size by rank 0 once every shard has written, run_mapping())
	const bool last_writer = !shard.active() || cx.opt.parts;
	// A deferred shard with a file of its own (-parts) writes while it maps and repairs the file's tail in the rare case that settling
	// changes a chunk: held back until the end, rank r's whole text was ONE burst after the mapping -- with two processes half the output
	// (12.6 M reads/s against 17.9 M for one process, profiles/r03zy; four processes hid it better, 91 %), with eight GPUs an eighth each
	// but behind two writers.  KART_AMD_NO_EAGER_PARTS=1: as before.
	const bool eager = deferred && cx.opt.parts && out && !cx.opt.bam && !getenv("KART_AMD_NO_EAGER_PARTS");
	if (!deferred || eager) writer.reset(new Writer(out, writer_threads, last_writer));
	// -un / -un2: one more writer per file, fed in chunk order beside the main one (two threads each: in an ordinary run next to nothing goes there)
	std::unique_ptr<Writer> un_writer[2];
	for (int f = 0; f < 2; ++f) {
		if (cx.un_out[f]) un_writer[f].reset(new Writer(cx.un_out[f], 2, true));
		cx.un_writer[f] = un_writer[f].get();
	}
	if (writer && shard.active() && !cx.opt.parts && !getenv("KART_AMD_NO_FILE_TURNS")) writer->take_turns(&shard.rdv->file_turn, shard.rank + 1, &shard.rdv->failed);
	// small batches first: the estimate moves fastest while the totals are small
	int64_t batch_chunks = 1;
	// enough chunks per batch to keep every worker busy (static chunk -> worker assignment)
	// ... and a whole number of chunks per worker, so that the last round of a phase is not half empty
	// batches are sized in bases: 400 k short reads, or ~10 k long reads (1024 chunks of 10) -- enough to fill the GPU and the
	// workers, small enough that three batches in flight stay within a few GB and that seeding overlaps the mapping
	// long reads, fragment pairs planned by the workers (round 2): batches of 1024 chunks of 10 reads -- the host is the bottleneck and
	// has to start early.  Fragment pairs on the device: batches of 2048 chunks.  A launch of the SensitiveMode search takes ~41 ms
	// whether it holds 10 k or 160 k reads (a chain of ~400 dependent searches per read, one lane each: tools/probe_sensitive.py), so
	// larger batches seed faster per read -- but the run as a whole does not gain: the search then fills the device and the fragment
	// calls of the slices (below) wait for it.  Measured, 7 kb reads, slices of 2048 chunks: 200 k reads -- batches of 2048 chunks
	// 1.76-1.88 s, doubling 2048 -> 8192 2.71 s, -> 16384 2.24 s; 1 M reads -- 6.00-6.20 s / 6.70 s / 8.17 s (host planning 8.62-9.00 s).
	// KART_AMD_PACBIO_MAX_CHUNKS > KART_AMD_PACBIO_CHUNKS lets the batches double up to it.
	// (not static: a session maps short-read and long-read libraries in turn)
	// With the report on the device as well (round 5) the workers only print: batches of 4096 chunks (41 k reads of 7 kb = 290 MB of characters) --
	// 400 k reads, hg38-sized index: 2048 chunks 2.50 s, 4096 2.40 s, 8192 2.71 s before the report ran beside the next batch's seeding (profiles/r05e_ab_long.log)
	const int64_t pacbio_chunks = getenv("KART_AMD_PACBIO_CHUNKS") ? std::max<int64_t>(1, atoll(getenv("KART_AMD_PACBIO_CHUNKS")))
	                                                              : (dev_long && cx.kern.long_enabled() ? 4096 : cx.frag_service ? 2048 : 1024);
	const int64_t pacbio_max_chunks = getenv("KART_AMD_PACBIO_MAX_CHUNKS") ? std::max<int64_t>(pacbio_chunks, atoll(getenv("KART_AMD_PACBIO_MAX_CHUNKS")))
	                                                                                : pacbio_chunks;
	static const int64_t frag_slice_env = getenv("KART_AMD_FRAG_SLICE") ? std::max<int64_t>(1, atoll(getenv("KART_AMD_FRAG_SLICE"))) : 2048;
	const int64_t frag_slice = (frag_slice_env + nthreads - 1) / nthreads * nthreads;
	int64_t want_chunks = cx.opt.pacbio ? std::max<int64_t>(pacbio_max_chunks, 8 * nthreads)
	                                     : std::max<int64_t>(std::max<int64_t>(1, cx.opt.batch_reads / chunk_limit), 4 * nthreads);
	const int64_t max_batch_chunks = (want_chunks + nthreads - 1) / nthreads * nthreads;
	if (!cx.opt.paired || cx.opt.pacbio) batch_chunks = max_batch_chunks;   // no EstDistance feedback to settle: full batches at once
	if (cx.opt.pacbio) batch_chunks = std::min(max_batch_chunks, (std::max<int64_t>(pacbio_chunks, 8 * nthreads) + nthreads - 1) / nthreads * nthreads);
	std::atomic<int> est_latest{est_speculated(cx, &shard, tot.iPaired, tot.iDistance)};     // EstDistance from the totals committed so far
	std::unique_ptr<Batch> cur(new Batch()), nxt(new Batch()), prev;
	std::shared_future<void> nw_prev;      // the gap-closing kernel call of `prev`, running on its own thread
	struct Pending { Batch *b; size_t from, to; std::shared_future<void> fut; };
	std::deque<Pending> pendq;             // (fragment pairs on the device) the slices whose calls are running, oldest first
	std::deque<std::unique_ptr<Batch>> limbo;   // ... and the batches they belong to, until their last slice is committed
	static const int frag_depth = getenv("KART_AMD_FRAG_DEPTH") ? std::max(1, std::min(3, atoi(getenv("KART_AMD_FRAG_DEPTH")))) : 2;

	// the two stages in front of the worker pool, each on a thread of its own: reading + parsing batch k+2 (the reader pool),
	// and the device stage of batch k+1 (seeding, chaining, the per-read report)
	auto read_stage = [&](Batch *b, int64_t n_chunks) { read_batch(cx, src, n_chunks, chunk_limit, read_pool, *b); };
	auto device_stage = [&](Batch *b) {
		double t = now_s();
		b->records = nullptr;
		if (!b->reads.empty()) {
			cx.kern.seed_and_chain(mode, cx.opt.pacbio, cx.opt.max_gaps, b->enc, b->off, b->n_cands, b->cand_off, b->own_cands, b->own_seeds, b->cands, b->cand_seeds);
			if (!cx.opt.pacbio) {
				// the per-read report of the batch on the device, under the latest committed estimate; what comes back as
				// KG_ALN_HOST (rescue, long gap fragments, ...) is mapped by the worker pool below
				std::vector<int64_t> coff;
				std::vector<uint8_t> cpaired;
				for (const ChunkState &ck : b->chunks) { coff.push_back(ck.begin); cpaired.push_back(ck.paired ? 1 : 0); }
				coff.push_back((int64_t)b->reads.size());
				b->est_dev = est_latest.load();
				if (cx.kern.align(coff, cpaired, b->est_dev, cx.opt.max_insert, cx.opt.max_gaps, cx.opt.multi_hit, g_unset_flag, b->records, b->chunk_dev)) {
					for (size_t c = 0; c < b->chunks.size(); ++c) { b->chunks[c].recs = b->records; b->chunks[c].dev = b->chunk_dev[c]; }
				} else b->records = nullptr;
			} else if (dev_long && cx.kern.long_enabled()) {
				// the per-read report of long reads on the device: what comes back as KG_ALN_HOST (a literal '-' in a read, a fragment
				// outside the kernels' envelope) is mapped by the worker pool below.  It runs on a thread of its own, in the workspace this
				// batch was seeded in, while the next batch is seeded in the other one; whoever needs the records first waits (long_ready)
				const int slot = cx.kern.long_slot();
				// (one workspace only -- KART_AMD_LONG_NO_OVERLAP, an A/B aid --: here and now, the next batch is seeded in the same arrays)
				b->long_fut = std::async(cx.kern.long_overlap() ? std::launch::async : std::launch::deferred, [&cx, b, slot]() {
					std::vector<int64_t> coff;
					for (const ChunkState &ck : b->chunks) coff.push_back(ck.begin);
					coff.push_back((int64_t)b->reads.size());
					if (cx.kern.align_long(slot, coff, b->records, b->cigar_pool, b->chunk_dev)) {
						for (size_t c = 0; c < b->chunks.size(); ++c) { b->chunks[c].recs = b->records; b->chunks[c].cigar_pool = b->cigar_pool; b->chunks[c].dev = b->chunk_dev[c]; }
					} else { b->records = nullptr; b->cigar_pool = nullptr; }
				}).share();
				if (!cx.kern.long_overlap()) b->long_fut.get();
			}
		}
		b->seed_seconds = now_s() - t;
	};
	auto commit = [&](Batch &b, size_t c_from, size_t c_to) {   // chunks [c_from, c_to) of the batch, in order: EstDistance feeds forward (src/Mapping.cpp:533-540)
		double t0 = now_s();
		if (deferred) {
			// the totals in front of this shard are not known yet: keep the chunks (text, validity interval, the views they came
			// from); the running totals of the shard itself only feed the next guesses
			for (size_t c = c_from; c < c_to; ++c) {
				ChunkState &ck = b.chunks[c];
				DeferredChunk d;
				d.views.assign(b.views.begin() + ck.begin, b.views.begin() + ck.begin + ck.count);
				d.paired = ck.paired; d.est_used = ck.est_used; d.ps = ck.ps; d.st = ck.st; d.text = std::move(ck.text);
				tot.iPaired += ck.ps.paired;
				tot.iDistance += ck.ps.distance;
				held.push_back(std::move(d));
				if (eager) write_held_chunk(writer.get(), held.back());
			}
			est_latest.store(est_speculated(cx, &shard, tot.iPaired, tot.iDistance));
			tot.t_commit += now_s() - t0;
			return;
		}
		// A chunk mapped under a speculated EstDistance stands if the true estimate -- a function of the totals of
		// all chunks before it -- would have decided every pair the same way.  Walk the batch with running totals,
		// collect the chunks whose speculation does not hold, re-map those together on the pool, and repeat: a
		// re-mapped chunk can move the estimates after it.  Every round settles at least the first unsettled chunk,
		// so the fixed point is the sequential result.
		for (;;) {
			std::vector<std::pair<size_t, int>> redo;
			int64_t paired = tot.iPaired, distance = tot.iDistance;
			for (size_t c = c_from; c < c_to; ++c) {
				ChunkState &ck = b.chunks[c];
				if (ck.paired) {
					int est_true = est_distance(cx, paired, distance);
					bool valid = est_true == ck.est_used ||
					             (ck.ps.lo < est_true && est_true <= ck.ps.hi &&
					              (!ck.ps.rescue_used || std::min(est_true, cx.opt.max_insert) == std::min(ck.est_used, cx.opt.max_insert)));
					if (!valid) redo.emplace_back(c, est_true);
				}
				paired += ck.ps.paired;
				distance += ck.ps.distance;
			}
			if (redo.empty()) break;
			st.respeculated += (int64_t)redo.size();
			pool.run((int)redo.size(), [&](int i) {
				// the device's records were made under the other estimate: the pairs whose own interval excludes the true one are
				// mapped again here; every other record stands
				b.chunks[redo[(size_t)i].first].force_invalid_pairs(redo[(size_t)i].second, cx.opt.max_insert);
				b.chunks[redo[(size_t)i].first].list_host_reads();
				chunk_stage_a(cx, b.reads, b.cand_off.data(), b.cands, b.cand_seeds, b.chunks[redo[(size_t)i].first], redo[(size_t)i].second);
			});
			std::vector<NwJobs *> parts;
			for (const std::pair<size_t, int> &r : redo)
				if (b.chunks[r.first].jobs.size() > 0) parts.push_back(&b.chunks[r.first].jobs);
			if (!parts.empty()) cx.kern.nw_batch(parts);
			pool.run((int)redo.size(), [&](int i) { chunk_stage_c(cx, b.reads, b.chunks[redo[(size_t)i].first]); });
		}
		for (size_t c = c_from; c < c_to; ++c) {
			ChunkState &ck = b.chunks[c];
			bytes_out += (int64_t)ck.text_size;
			tot.dev_reads += ck.count - ck.n_host; tot.host_reads += ck.n_host;
			writer->push(std::move(ck.text));
			for (int f = 0; f < 2; ++f)
				if (cx.un_writer[f] && !ck.un_text[f].empty()) cx.un_writer[f]->push(std::move(ck.un_text[f]));
			tot.iPaired += ck.ps.paired;
			tot.iDistance += ck.ps.distance;
			st.total_reads += ck.st.total_reads;
			st.unmapped += ck.st.unmapped;
			st.unique += ck.st.unique;
			if (st.tally && ck.tally) *st.tally += *ck.tally;
		}
		est_latest.store(est_distance(cx, tot.iPaired, tot.iDistance));
		if (shard.active() && shard.rank == 0) { shard.rdv->hint_paired.store(tot.iPaired); shard.rdv->hint_distance.store(tot.iDistance); }
		tot.t_commit += now_s() - t0;
	};

	// batches are recycled: their vectors (and the page-locked character buffer) keep their capacity
	std::vector<std::unique_ptr<Batch>> spare;
	auto fresh = [&]() {
		if (spare.empty()) return std::unique_ptr<Batch>(new Batch());
		std::unique_ptr<Batch> b = std::move(spare.back());
		spare.pop_back();
		b->reads.clear(); b->chunks.clear(); b->views.clear(); b->records = nullptr; b->cigar_pool = nullptr; b->cands = nullptr; b->cand_seeds = nullptr; b->eof = false;
		b->long_fut = std::shared_future<void>();
		return b;
	};
	// The device's FASTQ-in / SAM-out stream (stream.inc) takes plain FASTQ of short reads: it maps the library (or this shard's part
	// of it) up to the first thing its parser leaves to the reader below -- normally the end of the file.
	// ... and gz libraries: their text is inflated by threads of their own into a growing block that the stream reads like a mapped file
	// (Source::gz_stream_begin; KART_AMD_NO_GZ_STREAM: the host's gz reader maps them, as until round 5)
	// -bo: the device makes the BAM records (kg_stream_set_format) and the committed chunks are compressed beside the commit (BamPacker); a sharded
	// -bo run keeps the host's reader and encoder (a deferred shard holds text it may have to map again).  -bz device: the device compresses the records
	// as well (KG_STREAM_FORMAT_BAM_BGZF) and the packer takes its blocks where a piece of a chunk is made of whole ones; whatever does not go through
	// the stream -- a sharded run, -pacbio, KART_AMD_NO_STREAM, what the reader below maps after the stream stopped -- is compressed by the host as ever
	const bool bam_by_host = cx.opt.bam && shard.active();
	// FASTA (kg_stream_set_input): plain files mapped for the stream (Source::fasta_fast) and gz alike; a sharded run keeps the general reader
	if (src.gzfast && !src.fast && !cx.opt.pacbio && !g_check_align && cx.kern.has_stream() && !getenv("KART_AMD_NO_GZ_STREAM") && !shard.active()) src.gz_stream_begin();
	if ((src.fast || (src.fasta_fast && !shard.active()) || src.gzstream) && !cx.opt.pacbio && !bam_by_host && !g_check_align) {
		// window per file: the records of a full batch and half as much again (the first quarter of a staging buffer holds the
		// unconsumed tail of the batch before)
		double bpr = 0;
		for (int f = 0; f < (src.sep ? 2 : 1); ++f) {
			MappedFile &mf = f ? src.m2 : src.m1;
			if (mf.grow) { bool ended = false; mf.size = mf.map_size = mf.grow->wait_for((size_t)1 << 18, ended); }
			size_t lo = mf.pos, hi = std::min(mf.size, lo + ((size_t)1 << 18));
			int64_t lines = 0, blank = 0;
			count_lines(mf.data, lo, hi, lines, blank);
			// (FASTA: a record is a header line and what follows it)
			bpr = std::max(bpr, !cx.fastq ? fasta_bytes_per_record(mf.data, lo, hi) : lines >= 8 ? 4.0 * (double)(hi - lo) / (double)lines : 400.0);
		}
		// batches of 1 M reads (KART_AMD_STREAM_READS).  A search launch costs ~0.65 ms + 0.52 ms per M reads (1 M reads 1.21 ms, 2 M 1.75 ms,
		// 4 M 2.94 ms, 20 M 11.0 ms -- alone on the device, the same as inside a run), so larger batches spend less in the search (roofline.frac
		// 0.095 -> 0.128 at 2 M, 0.149 at 4 M) -- but the run as a whole loses: 100 M reads, alternating on one box, 1 M 29.9 / 30.4 M reads/s,
		// 2 M 28.7 / 27.9 M, 4 M 26.1 M (longer fill and drain, larger page-locked windows); 20 M reads: 0.82 s against 0.95 s per step.
		// ... of ordinary records.  Long records (1200-base reads without -pacbio, 1500-character headers: tools/probe_odd_inputs_vs_reference.py)
		// would size eight lanes' windows, character arrays and page-locked buffers for 1 M of THEM -- 3 GB windows, and the stream's
		// allocation failed on the box (profiles/r05b_probe_long_headers.log): a batch holds at most ~400 MB of text per file
		int64_t want_reads = cx.opt.stream_reads;
		{
			const double per_file = 400e6;
			const int64_t fit = (int64_t)(per_file / std::max(64.0, bpr)) * (src.sep ? 2 : 1);
			if (fit < want_reads) want_reads = std::max<int64_t>(chunk_limit, fit);
		}
		const int64_t full_reads = std::max<int64_t>(chunk_limit, want_reads / chunk_limit * chunk_limit);
		const int64_t recs_per_file = src.sep ? full_reads / 2 : full_reads;
		int64_t window = (int64_t)((double)recs_per_file * bpr * 1.5 / 0.75) + ((int64_t)8 << 20);
		window = std::min<int64_t>(window, (int64_t)3 << 30);
		// Seeding groups (round 4): the FM-index search of FOUR lanes' batches is ONE launch (a launch costs ~0.65 ms + 0.52 ms per M reads: at
		// 1 M reads per launch the kernel ran at 0.09 of the HBM peak inside a run against 0.21 in one 20 M-read launch), with two groups =
		// eight lanes, so that one group's batches go through chaining .. text while the other's are uploaded and parsed.
		// KART_AMD_SEED_GROUP=0|1 switches the groups off (four independent lanes, round 3's form); KART_AMD_STREAM_LANES sets the lane count.
		static const int lanes_env = getenv("KART_AMD_STREAM_LANES") ? atoi(getenv("KART_AMD_STREAM_LANES")) : 0;
		static const int group_env = getenv("KART_AMD_SEED_GROUP") ? atoi(getenv("KART_AMD_SEED_GROUP")) : 4;
		int group = group_env > 1 ? std::min(group_env, 8) : 0;
		int lanes = lanes_env > 0 ? std::min(lanes_env, 16) : (group ? 2 * group : 4);      // (independent lanes, six writers: 3 lanes 0.75-0.79 s per 20 M reads, 4 0.73 s, 5 0.72-0.73 s)
		if (group && lanes % group != 0) lanes = (lanes + group - 1) / group * group;
		if (StreamBackend *sb = cx.kern.stream(full_reads + full_reads / 4 + chunk_limit, window, lanes, group)) {
			sb->set_format(cx.opt.bam, cx.opt.bam && cx.opt.bz_device);      // (the stream is the session's: a -o run may follow a -bo run, a -bz host run a -bz device one)
			sb->set_tags(cx.opt.md);                    // (... and a run with -md one without)
			sb->set_read_group(cx.opt.read_group_id(cx.lib));      // (... and a library with a read group one without, or with another)
			sb->set_unmapped(cx.un());                  // (... and a run with -un one without)
			sb->set_stats(cx.stats);                    // (... and a run with -stats one without)
			sb->set_input(!cx.fastq);                   // (... and a FASTQ library a FASTA one)
			Options &o = const_cast<Options &>(cx.opt);
			const int64_t keep = o.batch_reads;
			o.batch_reads = full_reads;
			bool all = map_library_stream(cx, src, *sb, writer.get(), st, tot, est_latest, deferred ? &held : nullptr, bytes_out, cx.opt.paired ? chunk_limit : full_reads, &shard);
			o.batch_reads = keep;
			(void)all;       // (false: the reader below continues at src.m1.pos / src.m2.pos; true: it finds the files exhausted)
		}
		if (src.gzstream) src.gz_stream_end();      // (the gz reader below continues with the text the stream left -- none, normally)
		if (src.fasta_fast) {                       // the getline() reader below continues where the stream stopped -- at the end of the files, normally
			fseeko(src.in1.fp, (off_t)src.m1.pos, SEEK_SET);
			if (src.sep) fseeko(src.in2.fp, (off_t)src.m2.pos, SEEK_SET);
		}
	}
	std::unique_ptr<Batch> nn = fresh();         // cur: device stage done, being mapped; nxt: read, device stage runs now; nn: being read
	read_stage(cur.get(), batch_chunks);
	device_stage(cur.get());
	tot.t_read += cur->seconds;
	tot.t_seed += cur->seed_seconds;
	batch_chunks = std::min(max_batch_chunks, batch_chunks * 2);
	if (!cur->reads.empty() && !cur->eof) { read_stage(nxt.get(), batch_chunks); tot.t_read += nxt->seconds; }
	static const bool inline_fetch = getenv("KART_AMD_NO_PREFETCH") != nullptr;   // profiling aid: everything on the main thread
	const std::launch how = inline_fetch ? std::launch::deferred : std::launch::async;
	while (!cur->reads.empty() || prev || !pendq.empty()) {
		bool have_cur = !cur->reads.empty(), have_nxt = !nxt->reads.empty();
		bool more = have_nxt && !nxt->eof;
		batch_chunks = std::min(max_batch_chunks, batch_chunks * 2);
		std::future<void> f_dev, f_read;
		Batch *np = nxt.get(), *nnp = nn.get();
		if (have_nxt) f_dev = std::async(how, [&, np]() { device_stage(np); });
		if (more) f_read = std::async(how, [&, batch_chunks, nnp]() { read_stage(nnp, batch_chunks); });
		int est_guess = est_distance(cx, tot.iPaired, tot.iDistance);
		Batch *cp = cur.get(), *pp = prev.get();
		std::atomic<int64_t> nw_wait_ns{0};
		auto settle_oldest = [&]() {
			Pending pd = pendq.front();
			pendq.pop_front();
			double tw = now_s();
			pd.fut.wait();
			nw_wait_ns += (int64_t)((now_s() - tw) * 1e9) * nthreads;
			pd.fut.get();
			pool.run((int)(pd.to - pd.from), [&](int c) { chunk_stage_c(cx, pd.b->reads, pd.b->chunks[pd.from + (size_t)c]); });
			commit(*pd.b, pd.from, pd.to);
		};
		double t3 = now_s();
		if (have_cur && cp->long_fut.valid()) {          // (long reads) the device report of this batch: started behind its seeding, due now
			// ... once the text of the batch before is made: its report is in, this batch's is still running (the wait came first until round 5:
			// report and text of a batch then followed each other, 57 + 16 ms per 41 k reads, while the next batch's seeding took 37)
			while (!pendq.empty()) settle_oldest();
			double tw = now_s();
			cp->long_fut.get();
			cp->long_fut = std::shared_future<void>();
			tot.t_long_wait += now_s() - tw;
			t3 += now_s() - tw;
		}
		// one phase on the pool: plan the chunks of batch k, then -- once the gap-closing kernel call of batch k-1, which has
		// been running on its own thread since the last phase, is back -- finish and format the chunks of batch k-1
		if (cx.frag_service) {
			// the device aligns the fragment pairs (one long call per slice of the batch): plan slice j, start its call at once, and finish
			// + commit slice j-1 -- whose call has been running since the step before -- while it runs.  (The batches themselves are
			// larger than a slice: a launch of the SensitiveMode search takes the same ~40 ms for 10 k as for 160 k reads.)
			// Up to frag_depth calls are in flight (two: the device then overlaps one call's copies and kernels with the other's).
			const size_t n_cur = have_cur ? cp->chunks.size() : 0;
			for (size_t from = 0; from < n_cur; from += (size_t)frag_slice) {
				const size_t to = std::min(n_cur, from + (size_t)frag_slice);
				pool.run((int)(to - from), [&](int c) { cp->chunks[from + (size_t)c].list_host_reads(); chunk_stage_a(cx, cp->reads, cp->cand_off.data(), cp->cands, cp->cand_seeds, cp->chunks[from + (size_t)c], est_guess); });
				pendq.push_back(Pending{cp, from, to, std::async(std::launch::async, [&cx, cp, from, to]() { run_nw(cx, cp->chunks, from, to); }).share()});
				while ((int)pendq.size() > frag_depth) settle_oldest();
			}
			if (!have_cur)
				while (!pendq.empty()) settle_oldest();          // the input has ended: everything still in flight
		} else
		pool.run_ordered(have_cur ? (int)cp->chunks.size() : 0,
		                 [&](int c) { cp->chunks[(size_t)c].list_host_reads(); chunk_stage_a(cx, cp->reads, cp->cand_off.data(), cp->cands, cp->cand_seeds, cp->chunks[(size_t)c], !cp->records ? est_guess : cp->est_dev); },
		                 [&]() {
			                 if (!nw_prev.valid()) return;
			                 double tw = now_s();
			                 nw_prev.wait();
			                 nw_wait_ns += (int64_t)((now_s() - tw) * 1e9);
		                 },
		                 pp ? (int)pp->chunks.size() : 0, [&](int c) { chunk_stage_c(cx, pp->reads, pp->chunks[(size_t)c]); });
		if (nw_prev.valid()) nw_prev.get();
		double t4 = now_s();
		tot.t_nw += 1e-9 * (double)nw_wait_ns.load() / (double)nthreads;   // average time a worker stood waiting for the kernel call
		tot.t_a += t4 - t3;
		if (cx.frag_service) nw_prev = std::shared_future<void>();
		else if (have_cur) nw_prev = std::async(std::launch::async, [&cx, cp]() { run_nw(cx, cp->chunks, 0, cp->chunks.size()); }).share();
		else nw_prev = std::shared_future<void>();
		if (pp && !cx.frag_service) commit(*pp, 0, pp->chunks.size());
		if (prev && cx.frag_service) limbo.push_back(std::move(prev));
		else if (prev) spare.push_back(std::move(prev));
		while (!limbo.empty() && std::none_of(pendq.begin(), pendq.end(), [&](const Pending &pd) { return pd.b == limbo.front().get(); })) {
			spare.push_back(std::move(limbo.front()));
			limbo.pop_front();
		}
		prev = have_cur ? std::move(cur) : nullptr;
		double tw = now_s();
		if (f_dev.valid()) f_dev.get();
		if (f_read.valid()) f_read.get();
		tot.t_read += now_s() - tw;       // only the part of reading + the device stage that was not hidden
		if (have_nxt) tot.t_seed += nxt->seed_seconds;
		if (!have_cur && cur) spare.push_back(std::move(cur));
		cur = have_nxt ? std::move(nxt) : fresh();
		if (!have_nxt && nxt) spare.push_back(std::move(nxt));
		nxt = more ? std::move(nn) : fresh();
		if (!nn) nn = fresh();
	}
	if (deferred) {
		// settle: the true totals in front of this shard, then the same fixed-point rounds as the in-process commit
		Rendezvous *rv = shard.rdv;
		const double t_mapped = now_s();
		if (eager) finish_writer(*writer, tot);     // (everything mapped so far is in the file: settling may replace a chunk's text)
		shard.wait([&]() { return rv->done[shard.rank - 1].load() != 0; }, "waiting for the previous shard");
		tot.t_shard_wait = now_s() - t_mapped;
		const double t_settle = now_s();
		const int64_t p0 = rv->paired_end[shard.rank - 1].load(), d0 = rv->distance_end[shard.rank - 1].load();
		int64_t paired = p0, distance = d0;
		for (;;) {
			std::vector<std::pair<size_t, int>> redo;
			paired = p0; distance = d0;
			for (size_t c = 0; c < held.size(); ++c) {
				DeferredChunk &d = held[c];
				if (d.paired) {
					int est_true = est_distance(cx, paired, distance);
					bool valid = est_true == d.est_used ||
					             (d.ps.lo < est_true && est_true <= d.ps.hi &&
					              (!d.ps.rescue_used || std::min(est_true, cx.opt.max_insert) == std::min(d.est_used, cx.opt.max_insert)));
					if (!valid) redo.emplace_back(c, est_true);
				}
				paired += d.ps.paired;
				distance += d.ps.distance;
			}
			if (redo.empty()) break;
			st.respeculated += (int64_t)redo.size();
			remap_chunks(cx, src, held, redo, pool, mode);
		}
		tot.iPaired = paired; tot.iDistance = distance;
		tot.t_shard_settle = now_s() - t_settle;
		for (DeferredChunk &d : held) {
			bytes_out += (int64_t)d.text.size();
			st.total_reads += d.st.total_reads; st.unmapped += d.st.unmapped; st.unique += d.st.unique;
		}
	}
	if (shard.active()) {
		Rendezvous *rv = shard.rdv;
		const int r = shard.rank;
		rv->paired_end[r].store(tot.iPaired); rv->distance_end[r].store(tot.iDistance);
		rv->out_bytes[r].store(bytes_out);
		rv->total_reads[r].store(st.total_reads); rv->unmapped[r].store(st.unmapped); rv->unique[r].store(st.unique); rv->respec[r].store(st.respeculated);
		rv->done[r].store(1);
		if (eager) {
			// the text is in the file already; from the first chunk that settling changed (if any) the tail is written again
			size_t first_changed = held.size();
			off_t keep = 0;                              // (a later shard's part starts with its first chunk: the header is in rank 0's)
			for (size_t c = 0; c < held.size(); ++c) {
				const DeferredChunk &d = held[c];
				if (d.text.size() != d.written_len || text_hash(d.text) != d.written_hash) { first_changed = c; break; }
				keep += (off_t)d.written_len;
			}
			if (first_changed < held.size()) {
				fflush(out);
				if (ftruncate(fileno(out), keep) != 0 || lseek(fileno(out), keep, SEEK_SET) < 0) shard.die("cannot rewrite the tail of this shard's part");
				writer.reset(new Writer(out, writer_threads, true));
				for (size_t c = first_changed; c < held.size(); ++c) writer->push(std::move(held[c].text));
				st.rewritten_chunks += (int64_t)(held.size() - first_changed);
			}
		} else if (deferred && cx.opt.parts) {
			// -parts: this shard's text is a file of its own (opened by the caller)
			writer.reset(new Writer(out, writer_threads, true));
			writer->expect((size_t)bytes_out);
			for (DeferredChunk &d : held) writer->push(std::move(d.text));
		} else if (deferred) {
			// this shard's text follows the header and the text of every earlier shard
			shard.wait([&]() { return rv->out_ready.load() != 0; }, "waiting for the output file");
			int64_t at = rv->header_bytes.load();
			for (int q = 0; q < r; ++q) at += rv->out_bytes[q].load();       // (done[r-1] implies done[q] for every q < r)
			out = fopen(cx.opt.out_name.c_str(), "r+");                       // (created and truncated by shard 0)
			if (!out || lseek(fileno(out), (off_t)at, SEEK_SET) < 0) shard.die("cannot open the output file");
			shard_out = out;
			writer.reset(new Writer(out, writer_threads, last_writer));
			if (!getenv("KART_AMD_NO_FILE_TURNS")) writer->take_turns(&shard.rdv->file_turn, shard.rank + 1, &shard.rdv->failed);
			writer->expect((size_t)bytes_out);
			for (DeferredChunk &d : held) writer->push(std::move(d.text));
		}
	}
	double td = now_s();
	if (writer) finish_writer(*writer, tot);
	for (int f = 0; f < 2; ++f) {
		if (un_writer[f]) un_writer[f]->finish();
		cx.un_writer[f] = nullptr;
	}
	tot.t_drain += now_s() - td;
	if (shard.active()) shard.rdv->written[shard.rank].store(1);
}

// Which part of the library this process maps (shard.inc): the byte range of each mate file that holds the chunks
// [c_r, c_{r+1}), where c_r is the first chunk boundary at or after the start of this process's byte slice of mate file 1.
void plan_shard(const Ctx &cx, Source &src, Shard &shard, bool splittable)
{
	Rendezvous *rv = shard.rdv;
	const int r = shard.rank, n = shard.count;
	int64_t lines[2] = {0, 0}, blank = 0;
	if (splittable) {
		for (int f = 0; f < (src.sep ? 2 : 1); ++f) {
			const MappedFile &m = f ? src.m2 : src.m1;
			int64_t b = 0;
			count_lines(m.data, m.map_size * (size_t)r / (size_t)n, m.map_size * (size_t)(r + 1) / (size_t)n, lines[f], b);
			blank += b;
		}
	} else blank = 1;
	rv->lines[0][r].store(lines[0] + 1); rv->lines[1][r].store(lines[1] + 1);
	rv->blank[r].store(blank + 1);
	shard.wait([&]() {
		for (int q = 0; q < n; ++q)
			if (rv->blank[q].load() == 0 || rv->lines[0][q].load() == 0 || rv->lines[1][q].load() == 0) return false;
		return true;
	}, "waiting for the line counts of the other shards");
	std::vector<int64_t> l1((size_t)n), l2((size_t)n);
	int64_t total1 = 0, total2 = 0, odd = 0;
	for (int q = 0; q < n; ++q) {
		l1[(size_t)q] = rv->lines[0][q].load() - 1; l2[(size_t)q] = rv->lines[1][q].load() - 1;
		total1 += l1[(size_t)q]; total2 += l2[(size_t)q];
		odd += rv->blank[q].load() - 1;
	}
	// four lines per record, no empty lines, a final newline, both mate files alike: anything else is left to one process
	if (odd || total1 % 4 != 0 || (src.sep && total2 != total1) || src.m1.data[src.m1.map_size - 1] != '\n' || (src.sep && src.m2.data[src.m2.map_size - 1] != '\n')) {
		shard.solo = true;
		if (r > 0) { src.m1.pos = src.m1.size; if (src.sep) src.m2.pos = src.m2.size; }   // nothing to do here
		return;
	}
	const int chunk_limit = cx.opt.pacbio ? 10 : 4000;
	const int64_t per_line = 4 * (int64_t)(src.sep ? chunk_limit / 2 : chunk_limit);     // lines of one chunk in one file
	auto boundary = [&](int q) -> int64_t {       // first line of the first chunk that starts at or after slice q of mate file 1
		if (q >= n) return INT64_MAX;
		size_t b = src.m1.map_size * (size_t)q / (size_t)n;
		int64_t before = 0;
		for (int t = 0; t < q; ++t) before += l1[(size_t)t];
		int64_t first = before + ((b > 0 && src.m1.data[b - 1] != '\n') ? 1 : 0);
		return (first + per_line - 1) / per_line * per_line;
	};
	int64_t lo = boundary(r), hi = boundary(r + 1);
	src.m1.pos = offset_of_line(src.m1, l1, lo);
	src.m1.size = hi == INT64_MAX ? src.m1.map_size : offset_of_line(src.m1, l1, hi);
	if (src.sep) {
		src.m2.pos = offset_of_line(src.m2, l2, lo);
		src.m2.size = hi == INT64_MAX ? src.m2.map_size : offset_of_line(src.m2, l2, hi);
	}
}
