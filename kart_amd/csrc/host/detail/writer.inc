// host/detail/writer.inc -- where the run's text goes: the I/O threads' CPU placement, the SIGBUS guard of the output mapping, and the Writer
// (chunks placed into the output file in input order through shared mappings / pwrite threads, page allocation ahead of them, the turn the shard
// processes of one file take; reference: fwrite under OutputLock, src/Mapping.cpp:601-622).
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
struct TextPiece { const char *p; size_t n; };     // p == nullptr: the next n bytes of the item's own text

// The threads that live in the kernel's file paths -- the writers (page faults of the output file), the page allocator, the lane
// threads (copies out of the mapped input) -- are kept on the CPUs of ONE last-level cache.  Those paths serialise on a few locks
// and counters of the file; on the 2 x 64-core box the hand-over of such a cache line between two L3 domains costs more than the
// work done under it: four writers placed anywhere fill a fresh tmpfs file at 4.3 GB/s (3.7 us of system time per 4 KB page),
// four writers on one L3 at 13.2 GB/s (1.1 us) -- tools/ab_output_write_pinned.sh.  KART_AMD_IO_CPUS = a CPU list, or "none".
struct IoCpus {
	cpu_set_t set;
	bool valid = false;
	int count = 0;
};
bool parse_cpu_list(const char *text, cpu_set_t &out)
{
	CPU_ZERO(&out);
	int n = 0;
	for (const char *p = text; *p;) {
		if (*p < '0' || *p > '9') { ++p; continue; }
		long a = strtol(p, const_cast<char **>(&p), 10), b = a;
		if (*p == '-') b = strtol(p + 1, const_cast<char **>(&p), 10);
		for (long c = a; c <= b && c < CPU_SETSIZE; ++c) { CPU_SET((int)c, &out); n++; }
	}
	return n > 0;
}
// shard >= 0: a sharded run -- process r takes domain r mod n of the allowed domains in CPU order (deterministic: two processes
// never pick the same one because of where the scheduler happened to run them); -1: the domain this process runs on; -2: the one after it
IoCpus detect_io_cpus(int shard)
{
	IoCpus io;
	cpu_set_t allowed;
	if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return io;
	const char *env = getenv("KART_AMD_IO_CPUS");
	if (env && !strcmp(env, "none")) return io;
	cpu_set_t want;
	bool have = false;
	if (env) have = parse_cpu_list(env, want);
	else {
		// the L3 domains of the allowed CPUs, in CPU order; this process takes the one it runs on (a sharded run: the shift-th after it)
		std::vector<std::string> domains;
		int mine = -1;
		const int here = sched_getcpu();
		for (int c = 0; c < CPU_SETSIZE; ++c) {
			if (!CPU_ISSET(c, &allowed)) continue;
			char path[128], line[512];
			snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", c);
			FILE *fp = fopen(path, "r");
			if (!fp) continue;
			if (fgets(line, sizeof(line), fp)) {
				std::string d(line);
				size_t at = std::find(domains.begin(), domains.end(), d) - domains.begin();
				if (at == domains.size()) domains.push_back(d);
				if (c == here) mine = (int)at;
			}
			fclose(fp);
		}
		if (!domains.empty()) {
			const size_t pick = shard >= 0 ? (size_t)shard % domains.size() : (size_t)((mine < 0 ? 0 : mine) + (shard == -2 ? 1 : 0)) % domains.size();
			have = parse_cpu_list(domains[pick].c_str(), want);
		}
	}
	if (!have) return io;
	CPU_AND(&io.set, &want, &allowed);
	io.count = CPU_COUNT(&io.set);
	io.valid = io.count >= 8;              // (fewer than writers + lanes can use: not worth squeezing the I/O threads together)
	return io;
}
// L3 domains among the CPUs this process may run on
int count_l3_domains()
{
	cpu_set_t allowed;
	if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return 0;
	std::vector<std::string> domains;
	for (int c = 0; c < CPU_SETSIZE; ++c) {
		if (!CPU_ISSET(c, &allowed)) continue;
		char path[128], line[512];
		snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", c);
		FILE *fp = fopen(path, "r");
		if (!fp) continue;
		if (fgets(line, sizeof(line), fp) && std::find(domains.begin(), domains.end(), std::string(line)) == domains.end()) domains.push_back(line);
		fclose(fp);
	}
	return (int)domains.size();
}
IoCpus g_io_cpus, g_lane_cpus;
void pin_io_thread()
{
	if (g_io_cpus.valid) pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), &g_io_cpus.set);
}
// the stream's lane threads (they read the input into the staging buffers): on the L3 domain NEXT to the writers' (mapper.cpp;
// KART_AMD_LANE_CPUS=same keeps them with the writers, round 3's placement)
void pin_lane_thread()
{
	const IoCpus &io = g_lane_cpus.valid ? g_lane_cpus : g_io_cpus;
	if (io.valid) pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), &io.set);
}

// Asynchronous SAM output.  The chunks arrive in order, so each one's file offset is known when it is pushed.  On a seekable
// file several threads then place their chunks at once: the file is extended (ftruncate), the chunk's page range is mapped
// shared and the text copied in -- write()/pwrite() to ONE file serialise on the inode lock however many threads issue them
// (one thread's 2-4 GB/s was the end of the run: 7.5 GB of SAM per 20 M reads), page faults on a shared mapping do not.
// Where mapping is not possible (pipes, odd file systems) one thread writes sequentially.
// A store into the mapped output raises SIGBUS when the file system cannot provide the page (a full tmpfs, a file truncated by
// someone else): say so instead of dying silently.  (With page pre-allocation the shortage shows up as a failed fallocate first.)
// The handler looks at the faulting address: only a fault inside one of the Writer's output windows is this message; anything
// else (an input file truncated under the run, the host application's own mappings) goes to the handler that was installed
// before, which is also put back when the last Writer has finished.
struct SigbusGuard {
	static constexpr int kSlots = 256;
	static std::atomic<uintptr_t> lo[kSlots], hi[kSlots];
	static std::atomic<int> users;
	static struct sigaction old;
	static void handler(int sig, siginfo_t *si, void *uc)
	{
		const uintptr_t a = (uintptr_t)si->si_addr;
		for (int i = 0; i < kSlots; ++i) {
			const uintptr_t l = lo[i].load(std::memory_order_relaxed);
			if (l && a >= l && a < hi[i].load(std::memory_order_relaxed)) {
				static const char msg[] = "Error! the output file could not be extended (SIGBUS on its mapping): is the file system full?\n";
				ssize_t r = write(2, msg, sizeof(msg) - 1);
				(void)r;
				_exit(1);
			}
		}
		if (old.sa_flags & SA_SIGINFO) { if (old.sa_sigaction) { old.sa_sigaction(sig, si, uc); return; } }
		else if (old.sa_handler != SIG_DFL && old.sa_handler != SIG_IGN) { old.sa_handler(sig); return; }
		sigaction(SIGBUS, &old, nullptr);      // the default action: the faulting instruction runs again and the process dies as it would have
	}
	static void acquire()
	{
		if (users.fetch_add(1) != 0) return;
		struct sigaction sa;
		memset(&sa, 0, sizeof(sa));
		sa.sa_sigaction = handler;
		sa.sa_flags = SA_SIGINFO;
		sigemptyset(&sa.sa_mask);
		sigaction(SIGBUS, &sa, &old);
	}
	static void release()
	{
		if (users.fetch_sub(1) == 1) sigaction(SIGBUS, &old, nullptr);
	}
	static void add(void *base, size_t n)
	{
		for (int i = 0; i < kSlots; ++i) {
			uintptr_t none = 0;
			if (lo[i].compare_exchange_strong(none, (uintptr_t)base)) { hi[i].store((uintptr_t)base + n); return; }
		}
	}
	static void remove(void *base)
	{
		for (int i = 0; i < kSlots; ++i)
			if (lo[i].load() == (uintptr_t)base) { hi[i].store(0); lo[i].store(0); return; }
	}
};
std::atomic<uintptr_t> SigbusGuard::lo[SigbusGuard::kSlots], SigbusGuard::hi[SigbusGuard::kSlots];
std::atomic<int> SigbusGuard::users{0};
struct sigaction SigbusGuard::old;

// What the host can still hold in RAM: min(MemAvailable, cgroup memory.max - memory.current); -1 when neither can be read.  A
// tmpfs file's pages are RAM charged to this cgroup, and the tmpfs's own size limit (fstatvfs) is neither of the two.
int64_t host_memory_available()
{
	int64_t best = -1;
	if (FILE *fp = fopen("/proc/meminfo", "r")) {
		char line[256];
		while (fgets(line, sizeof(line), fp))
			if (!strncmp(line, "MemAvailable:", 13)) { best = atoll(line + 13) * 1024; break; }
		fclose(fp);
	}
	auto read_ll = [](const char *path, int64_t &v) {
		FILE *fp = fopen(path, "r");
		if (!fp) return false;
		char buf[64] = "";
		bool ok = fgets(buf, sizeof(buf), fp) && buf[0] >= '0' && buf[0] <= '9';
		fclose(fp);
		if (ok) v = atoll(buf);
		return ok;
	};
	int64_t mx = 0, cur = 0;
	if ((read_ll("/sys/fs/cgroup/memory.max", mx) && read_ll("/sys/fs/cgroup/memory.current", cur)) ||
	    (read_ll("/sys/fs/cgroup/memory/memory.limit_in_bytes", mx) && read_ll("/sys/fs/cgroup/memory/memory.usage_in_bytes", cur))) {
		if (mx < ((int64_t)1 << 60)) best = best < 0 ? mx - cur : std::min(best, mx - cur);
	}
	return best;
}

// the output window in bytes: KART_AMD_OUT_WINDOW_MB (default 1024), a whole number of pages
size_t out_window_bytes()
{
	const char *env = getenv("KART_AMD_OUT_WINDOW_MB");
	const long long mb = env ? std::max(1LL, atoll(env)) : 1024;
	return (size_t)mb << 20;
}

// where the time of Writer::finish() went (KART_AMD_VERBOSE), and the windows unmapped while the run went on
struct WriterTimes {
	double wait = 0, unmap = 0, truncate = 0;        // finish(): the queue running dry, the windows still mapped, the exact size
	double unmap_beside = 0;                         // the unmapping thread's munmap calls during the run
	int64_t windows_beside = 0, windows_at_end = 0;
};

class Writer {
public:
	// last_writer: this process writes the end of the file (a shard in front of others must neither shrink the file nor set its size)
	explicit Writer(FILE *out, int n_threads = 4, bool last_writer = true) : fd_(fileno(out)), last_writer_(last_writer), win_size_(out_window_bytes())
	{
		fflush(out);
		off_ = lseek(fd_, 0, SEEK_CUR);
		first_off_ = off_;
		seekable_ = off_ >= 0;
		if (seekable_) {
			struct stat sb;
			seekable_ = fstat(fd_, &sb) == 0 && S_ISREG(sb.st_mode);
		}
		use_map_ = seekable_ && !getenv("KART_AMD_NO_MMAP_OUT") && (fcntl(fd_, F_GETFL) & O_ACCMODE) == O_RDWR;
		if (!seekable_) n_threads = 1;
		// The writers' page faults allocate the pages of the output.  Kept on ONE L3 domain they scale with the threads (tools/
		// ab_output_write_threads.sh, 8 GB into a fresh tmpfs file: 4 threads 14 GB/s, 6 19 GB/s, 8 22.8 GB/s), and a thread that
		// allocates the pages AHEAD of them (fallocate, KART_AMD_PREALLOC=1: the default while four writers were the optimum) has
		// become the ceiling instead -- ~15 GB/s however many writers follow it, less with two or three such threads.  A full file
		// system is noticed by the free-space check where the file grows (grow_locked), and as a last resort by the SIGBUS message.
		if (use_map_) { SigbusGuard::acquire(); guarded_ = true; }
		alloc_on_ = use_map_ && getenv("KART_AMD_PREALLOC") && !getenv("KART_AMD_NO_PREALLOC");
		alloc_end_ = alloc_want_ = alloc_from_ = off_;
		if (alloc_on_) alloc_th_ = std::thread([this]() { pin_io_thread(); alloc_loop(); });
		// ... and ONE further thread puts its items into the file with pwrite() (KART_AMD_PWRITE_THREADS=n, default 1 beside four or more
		// mapping threads): no page-table work per page -- 0.67 us per 4 KB page against 1.05-1.45 us through a write fault -- but one
		// such writer at a time (the inode lock), so a second one adds nothing; beside the mapping threads the two paths meet only at the
		// page cache's own lock.  Measured at 100 M reads per step, alternating on one box (profiles/r04za_ab_pwrite.log, r04zb):
		// 6 + 0 threads 30.5 / 32.5 M mapped reads/s, 6 + 1 34.4 / 33.5, 7 + 1 34.1 / 36.7, 8 + 1 35.1 / 35.9, 6 + 2 33.9 / 35.3, 7 + 2 32.6 / 34.7.
		const int n_pwrite = !(seekable_ && use_map_) ? 0 : getenv("KART_AMD_PWRITE_THREADS") ? std::max(0, atoi(getenv("KART_AMD_PWRITE_THREADS"))) : (n_threads >= 4 ? 1 : 0);
		// A window whose bytes are all in the file is unmapped while the run goes on, by a thread of its own: kept until finish(),
		// 39 GB of windows (9.5 M page-table entries of shmem pages) were torn down on one thread after the last byte, inside the run.
		mode_ = getenv("KART_AMD_WRITER_MODE") ? atoi(getenv("KART_AMD_WRITER_MODE")) : 1;
		release_ = use_map_ && (mode_ == 1 || mode_ == 2);
		if (release_) {
			const char *where = getenv("KART_AMD_UNMAP_CPUS");
			const bool on_lanes = where && !strcmp(where, "lanes");
			unmap_th_ = std::thread([this, on_lanes]() { if (on_lanes) pin_lane_thread(); else pin_io_thread(); unmap_loop(); });
		}
		for (int t = 0; t < n_threads; ++t) th_.emplace_back([this]() { pin_io_thread(); loop(false); });
		for (int t = 0; t < n_pwrite; ++t) th_.emplace_back([this]() { pin_io_thread(); loop(true); });
	}
	~Writer() { finish(); }
	// a sharded run: the processes take turns at the file (Rendezvous::file_turn); `id` > 0 names this one
	void take_turns(std::atomic<int32_t> *turn, int id, std::atomic<int32_t> *failed = nullptr) { turn_ = turn; turn_id_ = id; failed_flag_ = failed; }
	bool failed() const { return discard_.load(); }
	// about this much text is going to follow what has been pushed so far: its pages are allocated right away
	void expect(size_t bytes)
	{
		if (!alloc_on_) return;
		std::lock_guard<std::mutex> lk(amu_);
		alloc_want_ = std::max(alloc_want_, off_ + (off_t)bytes);
		acv_.notify_all();
	}
	void push(std::string &&text)
	{
		std::lock_guard<std::mutex> lk(mu_);
		Item it;
		it.off = off_;
		if (seekable_) {
			off_ += (off_t)text.size();
			grow_locked();
			ask_ahead();
		}
		it.map = use_map_;
		it.text = std::move(text);
		q_.push_back(std::move(it));
		cv_.notify_one();
	}
	// a chunk whose text lies in several pieces that stay where they are until the writer has copied them (stream.inc: the device's
	// lines in a lane's page-locked buffer; a piece without address is the next n bytes of `hold`, the host's lines): *pending is
	// decremented, under *mu, once that is done
	void push_pieces(std::vector<TextPiece> &&pieces, size_t total, std::string &&hold, std::atomic<int> *pending, std::mutex *mu, std::condition_variable *cv)
	{
		std::lock_guard<std::mutex> lk(mu_);
		Item it;
		it.off = off_;
		if (seekable_) {
			off_ += (off_t)total;
			grow_locked();
			ask_ahead();
		}
		it.map = use_map_;
		it.text = std::move(hold);
		it.pieces = std::move(pieces);
		it.pending = pending; it.done_mu = mu; it.done_cv = cv;
		q_.push_back(std::move(it));
		cv_.notify_one();
	}
	// Every window is unmapped before this returns: the ones released during the run by the unmapping thread (joined here, after
	// whatever it still had in hand) and the ones still open -- normally the last one or two.
	void finish()
	{
		if (th_.empty()) return;
		const double t0 = now_s();
		{
			std::lock_guard<std::mutex> lk(mu_);
			stop_ = true;
		}
		cv_.notify_all();
		for (std::thread &t : th_) t.join();
		th_.clear();
		if (alloc_th_.joinable()) {
			{
				std::lock_guard<std::mutex> lk(amu_);
				alloc_stop_ = true;
			}
			acv_.notify_all();
			alloc_th_.join();
			extended_ = extended_ || alloc_end_ > alloc_from_;
		}
		if (turn_ && have_turn_) { have_turn_ = false; turn_->store(0); }          // (never keep the turn past the last item)
		const double t1 = now_s();
		if (unmap_th_.joinable()) {
			{
				std::lock_guard<std::mutex> lk(umu_);
				unmap_stop_ = true;
			}
			ucv_.notify_all();
			unmap_th_.join();
		}
		for (const std::pair<const off_t, char *> &w : win_) { SigbusGuard::remove(w.second); munmap(w.second, win_size_); times_.windows_at_end++; }
		win_.clear();
		done_.clear();
		if (guarded_) { SigbusGuard::release(); guarded_ = false; }
		const double t2 = now_s();
		if (seekable_) {
			if ((use_map_ || extended_) && last_writer_ && ftruncate(fd_, off_) != 0) run_fail("ftruncate of the output file: %s", strerror(errno));    // the exact size
			lseek(fd_, off_, SEEK_SET);
		}
		const double t3 = now_s();
		times_.wait += t1 - t0; times_.unmap += t2 - t1; times_.truncate += t3 - t2;
	}
	const WriterTimes &times() const { return times_; }

private:
	// windows of the output file mapped shared, each kept until every byte of it this Writer hands out has been copied: unmapping per
	// chunk costs a TLB shoot-down across all the threads of the process every time
	static constexpr size_t kGrow = (size_t)256 << 20, kAhead = (size_t)768 << 20, kAllocStep = (size_t)64 << 20;
	struct Item {
		std::string text;
		off_t off;
		bool map = false;
		std::vector<TextPiece> pieces;           // empty: the chunk is `text`
		std::atomic<int> *pending = nullptr;
		std::mutex *done_mu = nullptr;
		std::condition_variable *done_cv = nullptr;
	};
	// the mapping needs the pages to exist in the file; the file grows in large steps (the final size is set in finish()).  Several
	// shard processes extend the same file: growth is monotonic under an advisory lock (a bare fstat + ftruncate pair could shrink
	// what another process had extended in between).
	// The turn belongs to the process: all its threads work while it has it; it is given up once nothing is in hand and either
	// nothing is queued or it has been held for a few milliseconds (the others' text is waiting as well).
	void turn_acquire()
	{
		if (!turn_) return;
		std::unique_lock<std::mutex> lk(tmu_);
		for (long spins = 0;;) {
			if (have_turn_ && !yielding_) { turn_active_++; return; }
			if (!have_turn_) {
				int32_t nobody = 0;
				if (turn_->compare_exchange_strong(nobody, turn_id_)) { have_turn_ = true; yielding_ = false; turn_since_ = now_s(); turn_active_++; return; }
			}
			lk.unlock();
			usleep(40);
			// (a process that failed gives the turn up, shard_mark_failed(); the others stop waiting for it here)
			if ((failed_flag_ && failed_flag_->load()) || ++spins > 20000000) {
				run_fail("the output file's turn never came (another shard process failed%s)", failed_flag_ && failed_flag_->load() ? "" : " or died holding it?");
				discard_ = true;
				lk.lock();
				have_turn_ = true; yielding_ = false; turn_active_++;      // (nothing more is written: pass every waiter through)
				return;
			}
			lk.lock();
		}
	}
	void turn_release()
	{
		if (!turn_) return;
		bool more_queued;
		{
			std::lock_guard<std::mutex> lk(mu_);
			more_queued = !q_.empty();             // (looked up now: what was queued when the item was taken may be gone)
		}
		std::lock_guard<std::mutex> lk(tmu_);
		turn_active_--;
		if (have_turn_ && (!more_queued || now_s() - turn_since_ > 0.004)) yielding_ = true;
		if (yielding_ && turn_active_ == 0) { have_turn_ = false; yielding_ = false; turn_->store(0); }
	}
	void ask_ahead()                                  // (mu_ held)
	{
		if (!alloc_on_) return;
		std::lock_guard<std::mutex> lk(amu_);
		if (off_ + (off_t)kAhead > alloc_want_) { alloc_want_ = off_ + (off_t)kAhead; acv_.notify_all(); }
	}
	void alloc_loop()
	{
		std::unique_lock<std::mutex> lk(amu_);
		for (;;) {
			acv_.wait(lk, [this]() { return alloc_stop_ || alloc_want_ > alloc_end_; });
			if (alloc_stop_) return;
			const off_t from = alloc_end_;
			off_t to = std::min<off_t>(alloc_want_, from + (off_t)kAllocStep);
			to = (to + 4095) & ~(off_t)4095;
			lk.unlock();
			turn_acquire();
			int rc = fallocate(fd_, 0, from, to - from);         // (extends the file, never shrinks it: safe beside other shards)
			turn_release();
			lk.lock();
			if (rc != 0) {
				// no such call on this file system, or no room: fall back to a sparse file whose pages the writers' faults allocate
				// (long enough for everything pushed so far: alloc_want_ lies beyond it)
				struct stat sb;
				flock(fd_, LOCK_EX);
				if (fstat(fd_, &sb) == 0 && sb.st_size < alloc_want_ && ftruncate(fd_, alloc_want_) != 0) perror("ftruncate");
				flock(fd_, LOCK_UN);
				alloc_on_ = false;
				acv_.notify_all();
				return;
			}
			alloc_end_ = to;
			acv_.notify_all();
		}
	}
	// blocks until the pages of [.., end) exist (or pre-allocation has been given up)
	void wait_allocated(off_t end)
	{
		if (!alloc_on_) return;
		std::unique_lock<std::mutex> lk(amu_);
		if (end > alloc_want_) { alloc_want_ = end; acv_.notify_all(); }
		acv_.wait(lk, [&]() { return !alloc_on_ || alloc_end_ >= end; });
	}
	void grow_locked()
	{
		if (alloc_on_) return;                       // (the allocator extends the file; a truncate beside it could cut what it had added)
		if (!use_map_ || off_ <= file_end_) return;
		const off_t had = file_end_;
		off_t want = (off_ + (off_t)kGrow) & ~((off_t)kGrow - 1);
		struct stat sb;
		flock(fd_, LOCK_EX);
		if (fstat(fd_, &sb) != 0) use_map_ = false;
		else if (sb.st_size >= want) file_end_ = sb.st_size;               // (another shard has extended it already: never shrink)
		else if (ftruncate(fd_, want) == 0) { file_end_ = want; extended_ = true; }
		else use_map_ = false;
		flock(fd_, LOCK_UN);
		// the file is sparse from here on: its pages are allocated by the writers' stores, which cannot fail politely -- so look now
		// whether the file system has room for the text handed out beyond the old end of the file (a small output on a nearly full
		// file system must still go through; what arrives before the next step -- at most 256 MB -- is covered by the SIGBUS message)
		// A file system that reports no size at all (tmpfs / ramfs without a limit, some FUSE and 9p mounts: f_blocks == 0) is not
		// asked.  On tmpfs the pages are RAM: there the figure that matters is what the host (and this cgroup) can still hold, not the
		// mount's nominal size -- half a GB is left alone for everybody else.
		struct statvfs vfs;
		struct statfs sfs;
		const uint64_t due = (uint64_t)(off_ - std::max<off_t>(had, 0)) + ((uint64_t)1 << 20);
		if (!use_map_ || discard_) return;
		if (fstatvfs(fd_, &vfs) == 0 && vfs.f_blocks != 0 && (uint64_t)vfs.f_bavail * (uint64_t)vfs.f_frsize < due) {
			run_fail("no space left for the output file (%llu MB to write, %llu MB free)", (unsigned long long)(due >> 20),
			         (unsigned long long)(((uint64_t)vfs.f_bavail * (uint64_t)vfs.f_frsize) >> 20));
			discard_ = true;
			return;
		}
		if (fstatfs(fd_, &sfs) == 0 && (unsigned long)sfs.f_type == 0x01021994UL /* TMPFS_MAGIC */) {
			const int64_t avail = host_memory_available();
			static const uint64_t reserve = (uint64_t)(getenv("KART_AMD_MEM_RESERVE_MB") ? std::max<long long>(0, atoll(getenv("KART_AMD_MEM_RESERVE_MB"))) : 512) << 20;
			if (avail >= 0 && (uint64_t)avail < due + reserve) {
				run_fail("the output file lives in memory (tmpfs) and the host cannot hold it: %llu MB to write, %lld MB of memory available to this process group",
				         (unsigned long long)(due >> 20), (long long)(avail >> 20));
				discard_ = true;
			}
		}
	}
	char *window(off_t index)
	{
		std::lock_guard<std::mutex> lk(win_mu_);
		std::map<off_t, char *>::iterator it = win_.find(index);
		if (it != win_.end()) return it->second;
		void *m = mmap(nullptr, win_size_, PROT_READ | PROT_WRITE, MAP_SHARED, fd_, index * (off_t)win_size_);
		if (m == MAP_FAILED) return nullptr;
		win_[index] = (char *)m;
		if (guarded_) SigbusGuard::add(m, win_size_);
		return (char *)m;
	}
	// the item at [at, at + n) has been handled (copied, written, or dropped after a failure), by whichever path: each window it
	// covers counts its bytes, and a window that holds all it will ever get from this Writer -- its bytes from first_off_ on, which
	// are handed out in order, so the queue has passed its end -- goes to the unmapping thread.  Nothing is mapped there again.
	void complete(off_t at, size_t n)
	{
		if (!release_ || n == 0) return;
		const off_t W = (off_t)win_size_, end = at + (off_t)n;
		std::lock_guard<std::mutex> lk(win_mu_);
		while (at < end) {
			const off_t wi = at / W, w_end = (wi + 1) * W, upto = std::min(end, w_end);
			off_t &d = done_[wi];
			d += upto - at;
			at = upto;
			if (d < w_end - std::max(wi * W, first_off_)) continue;
			done_.erase(wi);
			std::map<off_t, char *>::iterator it = win_.find(wi);
			if (it == win_.end()) continue;                  // (none of it went through the mapping)
			{
				std::lock_guard<std::mutex> ul(umu_);
				retired_.push_back(it->second);
			}
			ucv_.notify_one();
			win_.erase(it);
		}
	}
	void unmap_loop()
	{
		std::unique_lock<std::mutex> lk(umu_);
		for (;;) {
			ucv_.wait(lk, [this]() { return unmap_stop_ || !retired_.empty(); });
			if (retired_.empty()) return;
			char *w = retired_.front();
			retired_.pop_front();
			lk.unlock();
			const double t0 = now_s();
			SigbusGuard::remove(w);
			munmap(w, win_size_);
			const double dt = now_s() - t0;
			lk.lock();
			times_.unmap_beside += dt;
			times_.windows_beside++;
		}
	}
	void loop(bool by_pwrite)
	{
		for (;;) {
			Item it;
			{
				std::unique_lock<std::mutex> lk(mu_);
				cv_.wait(lk, [this]() { return stop_ || !q_.empty(); });
				if (q_.empty()) return;
				it = std::move(q_.front());
				q_.pop_front();
			}
			off_t at = it.off;
			size_t hold_at = 0;
			if (by_pwrite) it.map = false;
			size_t bytes = it.text.size();
			if (!it.pieces.empty()) { bytes = 0; for (const TextPiece &tp : it.pieces) bytes += tp.n; }
			if (it.map) wait_allocated(it.off + (off_t)bytes);
			turn_acquire();
			const size_t n_parts = it.pieces.empty() ? 1 : it.pieces.size();
			for (size_t part = 0; part < n_parts && !discard_; ++part) {
			const char *p = it.text.data();
			size_t left = it.text.size();
			if (!it.pieces.empty()) {
				const TextPiece &tp = it.pieces[part];
				left = tp.n;
				if (tp.p) p = tp.p;
				else { p = it.text.data() + hold_at; hold_at += tp.n; }
			}
			while (it.map && left > 0) {
				// experiment switch (mode_): 0 a mapping per chunk (1.60-1.65 s per 20 M reads), 1 windows (1.35-1.9 s), 2 windows + MADV_POPULATE_WRITE
				// (2.2-2.3 s), 3 windows kept until finish() (the form before they were released during the run); pwrite: 3.4 s
				const int mode = mode_;
				if (mode == 0) {
					static const size_t page = (size_t)sysconf(_SC_PAGESIZE);
					off_t base = at - (off_t)((size_t)at % page);
					size_t span = (size_t)(at - base) + left;
					void *m = mmap(nullptr, span, PROT_READ | PROT_WRITE, MAP_SHARED, fd_, base);
					if (m == MAP_FAILED) break;
					memcpy((char *)m + (at - base), p, left);
					munmap(m, span);
					p += left; at += (off_t)left; left = 0;
					break;
				}
				off_t wi = at / (off_t)win_size_;
				char *w = window(wi);
				if (!w) break;
				size_t in = (size_t)(at - wi * (off_t)win_size_), n = std::min(left, win_size_ - in);
#ifdef MADV_POPULATE_WRITE
				if (mode == 2) {	// the pages of the range in one call instead of one write fault per 4 KB page
					size_t a = in & ~(size_t)4095, b = std::min(win_size_, (in + n + 4095) & ~(size_t)4095);
					madvise(w + a, b - a, MADV_POPULATE_WRITE);
				}
#endif
				memcpy(w + in, p, n);
				p += n; left -= n; at += (off_t)n;
			}
			while (left > 0) {
				ssize_t wr = seekable_ ? ::pwrite(fd_, p, left, at) : ::write(fd_, p, left);
				if (wr <= 0) { run_fail("write to the output: %s", strerror(errno)); discard_ = true; break; }
				p += wr; left -= (size_t)wr; at += wr;
			}
			}
			turn_release();
			if (seekable_) complete(it.off, bytes);
			if (it.pending) {
				std::lock_guard<std::mutex> lk(*it.done_mu);
				it.pending->fetch_sub(1);
				it.done_cv->notify_all();
			}
		}
	}
	int fd_;
	bool last_writer_ = true, guarded_ = false;
	std::atomic<bool> discard_{false};           // the run has failed (run_fail): the items still in the queue are dropped, the run returns an error
	std::atomic<int32_t> *failed_flag_ = nullptr;
	off_t off_ = 0, file_end_ = 0;
	bool seekable_ = false, use_map_ = false, extended_ = false;
	// taking turns with the other shard processes
	std::atomic<int32_t> *turn_ = nullptr;
	int32_t turn_id_ = 0;
	std::mutex tmu_;
	bool have_turn_ = false, yielding_ = false;
	int turn_active_ = 0;
	double turn_since_ = 0;
	// page allocation ahead of the text
	std::thread alloc_th_;
	std::mutex amu_;
	std::condition_variable acv_;
	off_t alloc_from_ = 0, alloc_end_ = 0, alloc_want_ = 0;
	std::atomic<bool> alloc_on_{false};
	bool alloc_stop_ = false;
	std::mutex mu_, win_mu_;
	std::map<off_t, char *> win_;
	// releasing the windows during the run (complete(), unmap_loop())
	const size_t win_size_;
	int mode_ = 1;
	bool release_ = false;
	off_t first_off_ = 0;                          // where this Writer's text starts (a shard's part, a rewritten tail: inside a window)
	std::map<off_t, off_t> done_;                  // window -> its bytes copied so far (win_mu_)
	std::thread unmap_th_;
	std::mutex umu_;
	std::condition_variable ucv_;
	std::deque<char *> retired_;
	bool unmap_stop_ = false;
	WriterTimes times_;
	std::condition_variable cv_;
	std::deque<Item> q_;
	bool stop_ = false;
	std::vector<std::thread> th_;
};
