// host/detail/types.inc -- small helpers and the per-read data (ReadItem_t, SeedPair_t, AlignmentCandidate_t, AlignmentReport_t).
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
// ----------------------------------------------------------------------------------------------
// small helpers
// ----------------------------------------------------------------------------------------------
inline int nt4(unsigned char ch)  // nst_nt4_table, src/BWT_Index/bntseq.c:40-57
{
	switch (ch) {
	case 'A': case 'a': return 0;
	case 'C': case 'c': return 1;
	case 'G': case 'g': return 2;
	case 'T': case 't': return 3;
	default: return 4;
	}
}

// GetComplementaryBase, src/tools.cpp:3-17, as a table (it runs over every base of every mate 2 and of every reverse-strand
// record): A/a -> T, C/c -> G, G/g -> C, T/t -> A, anything else -> N
struct CompTable {
	char t[256];
	constexpr CompTable() : t()
	{
		for (int i = 0; i < 256; ++i) t[i] = 'N';
		t['A'] = t['a'] = 'T'; t['C'] = t['c'] = 'G'; t['G'] = t['g'] = 'C'; t['T'] = t['t'] = 'A';
	}
};
constexpr CompTable kComp;
inline char comp_base(char c) { return kComp.t[(unsigned char)c]; }

// out[i] = comp_base(in[n - 1 - i]) (GetComplementarySeq) and out[i] = in[n - 1 - i], 16 bytes per step where the CPU has SSSE3:
// these two loops run over every mate 2 on input and over every reverse-strand record on output
__attribute__((target("ssse3"))) void revcomp_ssse3(char *out, const char *in, size_t n)
{
	const __m128i rev = _mm_set_epi8(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
	const __m128i up = _mm_set1_epi8((char)0xDF), cA = _mm_set1_epi8('A'), cC = _mm_set1_epi8('C'), cG = _mm_set1_epi8('G'), cT = _mm_set1_epi8('T'), cN = _mm_set1_epi8('N');
	size_t i = 0;
	for (; i + 16 <= n; i += 16) {
		__m128i v = _mm_shuffle_epi8(_mm_loadu_si128((const __m128i *)(in + n - 16 - i)), rev);
		__m128i u = _mm_and_si128(v, up);
		__m128i a = _mm_cmpeq_epi8(u, cA), c = _mm_cmpeq_epi8(u, cC), g = _mm_cmpeq_epi8(u, cG), t = _mm_cmpeq_epi8(u, cT);
		__m128i any = _mm_or_si128(_mm_or_si128(a, c), _mm_or_si128(g, t));
		__m128i r = _mm_or_si128(_mm_or_si128(_mm_and_si128(a, cT), _mm_and_si128(c, cG)), _mm_or_si128(_mm_and_si128(g, cC), _mm_and_si128(t, cA)));
		r = _mm_or_si128(r, _mm_andnot_si128(any, cN));
		_mm_storeu_si128((__m128i *)(out + i), r);
	}
	for (; i < n; ++i) out[i] = comp_base(in[n - 1 - i]);
}
__attribute__((target("ssse3"))) void reverse_ssse3(char *out, const char *in, size_t n)
{
	const __m128i rev = _mm_set_epi8(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
	size_t i = 0;
	for (; i + 16 <= n; i += 16) _mm_storeu_si128((__m128i *)(out + i), _mm_shuffle_epi8(_mm_loadu_si128((const __m128i *)(in + n - 16 - i)), rev));
	for (; i < n; ++i) out[i] = in[n - 1 - i];
}
inline void revcomp_into(char *out, const char *in, size_t n)
{
	static const bool simd = __builtin_cpu_supports("ssse3");
	if (simd) { revcomp_ssse3(out, in, n); return; }
	for (size_t i = 0; i < n; ++i) out[i] = comp_base(in[n - 1 - i]);
}
inline void reverse_into(char *out, const char *in, size_t n)
{
	static const bool simd = __builtin_cpu_supports("ssse3");
	if (simd) { reverse_ssse3(out, in, n); return; }
	for (size_t i = 0; i < n; ++i) out[i] = in[n - 1 - i];
}

std::string revcomp(std::string_view s)  // GetComplementarySeq, src/tools.cpp:19-29
{
	std::string r(s.size(), 'N');
	for (size_t i = 0, n = s.size(); i < n; ++i) r[i] = comp_base(s[n - 1 - i]);
	return r;
}

double now_s()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

bool slurp(const std::string &path, std::vector<unsigned char> &buf)
{
	FILE *fp = fopen(path.c_str(), "rb");
	if (!fp) return false;
	fseek(fp, 0, SEEK_END);
	long sz = ftell(fp);
	fseek(fp, 0, SEEK_SET);
	buf.resize((size_t)sz);
	size_t got = sz ? fread(buf.data(), 1, (size_t)sz, fp) : 0;
	fclose(fp);
	return got == (size_t)sz;
}

// ----------------------------------------------------------------------------------------------
// data carried per read (ReadItem_t, SeedPair_t, AlignmentCandidate_t, AlignmentReport_t;
// src/structure.h:106-154)
// ----------------------------------------------------------------------------------------------
struct Pair {
	bool simple;
	int rPos;
	int64_t gPos;
	int rLen, gLen;
	int64_t posDiff;
};

struct Candidate {
	int score = 0;
	int64_t posDiff = 0;
	int mate = -1;   // PairedAlnCanIdx
	std::vector<Pair> pairs;
};

// SamFlag of a record the reference never assigns (src/AlignmentCandidates.cpp:636-640: AlnReportArr is new-ed without
// initialising SamFlag; SURVEY App. B-12).  The reference prints heap contents there; this pipeline prints a defined
// value: 0, or KART_AMD_UNSET_FLAG when set -- the parity tests use a sentinel to find exactly those records.
int g_unset_flag = 0;

// A run that cannot go on (no room for the output, a write error) records WHY and comes back from run_mapping() with a
// status -- the library never calls exit() on the caller's process for it.  First message wins; printed to stderr as well.
std::atomic<bool> g_run_failed{false};
std::mutex g_run_err_mu;
std::string g_run_err;
void run_error_reset() { std::lock_guard<std::mutex> lk(g_run_err_mu); g_run_failed.store(false); g_run_err.clear(); }
bool run_failed() { return g_run_failed.load(std::memory_order_relaxed); }
void run_fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void run_fail(const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	std::lock_guard<std::mutex> lk(g_run_err_mu);
	if (g_run_failed.exchange(true)) return;
	g_run_err = buf;
	fprintf(stderr, "Error! %s\n", buf);
}

struct Report {
	int score = 0;          // AlnScore
	int flag = g_unset_flag;   // SamFlag (never-set records print g_unset_flag)
	int mate = -1;          // PairedAlnCanIdx
	bool fwd = true;        // coor.bDir
	std::string cigar;
	int64_t gPos = 0;
	int chr = 0;            // coor.ChromosomeIdx (uninitialised in the reference when never assigned; here 0)
};

struct Read {
	// views into the mapped input file, or into the batch's own storage (reverse-complemented mates, the
	// getline()/gzgets() readers); no per-read allocation
	std::string_view name, seq, qual;
	// -un / -un2 (empty otherwise): the record as it lies in the input text, from the first byte of its header line through the last line the reader took for it
	std::string_view raw;
	bool qual_rev = false;     // `qual` is the file's bytes of a mate that is held reversed: the held string is its reverse
	int rlen = 0;
	int mapq = 0, score = 0, sub_score = 0, can_num = 0, best = 0;
	std::vector<Report> rep;
};

typedef std::vector<std::pair<int, char>> CigarVec;

bool pair_by_gpos(const Pair &a, const Pair &b)  // CompByGenomePos, src/AlignmentCandidates.cpp:17-21
{
	if (a.gPos == b.gPos) return a.rPos < b.rPos;
	return a.gPos < b.gPos;
}

struct Ctx {
	const Options &opt;
	const RefData &ref;
	KernelBackend &kern;
	int min_seed_len;
	bool fastq = true;
	bool frag_service = false;     // -pacbio: GenerateNormalPairAlignment runs on the device in one call per batch (KernelBackend::fragments_batch)
	std::map<std::string_view, int> bam_ref_id;   // -bo: contig name -> reference id
	size_t lib = 0;                // the library being mapped: its place in Options::files1
	// -un / -un2: where the unmapped reads of either input file go (null: nowhere), and the writers of the library being mapped (map_library)
	FILE *un_out[2] = {nullptr, nullptr};
	class Writer *un_writer[2] = {nullptr, nullptr};
	bool un() const { return un_out[0] != nullptr; }
	bool stats = false;            // -stats: every chunk tallies the records it prints (ChunkState::tally)
	std::string rg_field;          // -R: "\tRG:Z:<ID>" of the library being mapped, the last field of every record it prints; empty: none
	const char *refseq() const { return ref.seq.get(); }
};

// What one 4000-read chunk contributes to the run-wide pairing statistics (iPaired / iDistance,
// src/Mapping.cpp:13,20,209-213), and for which EstDistance values its pairing decisions hold.
struct PairStats {
	int64_t paired = 0, distance = 0;
	// every "dist < EstiDistance" test of CheckPairedAlignmentCandidates (:372) narrows the interval
	// (lo, hi] of EstDistance values that would have produced the same outcome
	int64_t lo = -1, hi = INT64_MAX;
	bool rescue_used = false;      // rescue windows depend on min(EstDistance, MaxInsertSize)
};

// ----------------------------------------------------------------------------------------------
// chaining (GenerateAlignmentCandidateForIlluminaSeq / ForPacBioSeq, src/AlignmentCandidates.cpp:82-130,
// 171-224) runs on the device: KernelBackend::candidates_batch -> kg_candidates_batch (chain_kernel in
// seed_kernels.hip); chunk_stage_a unpacks its output with from_seed()
// ----------------------------------------------------------------------------------------------
Pair from_seed(const kg_seed &s)
{
	Pair p;
	p.simple = true; p.rPos = s.rPos; p.gPos = s.gPos; p.rLen = p.gLen = s.len; p.posDiff = s.gPos - s.rPos;
	return p;
}
