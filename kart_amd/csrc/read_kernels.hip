// read_kernels.hip -- the stream's input side, on the device (gfx950): FASTQ or FASTA text in, the reads of a batch out; and grouped seeding's two helpers.
// = GetNextChunk / GetNextEntry (reference src/GetData.cpp:29-143) for a whole window of text at once:
//   fq_count_kernel / fq_index_kernel   the lines of the window: every '\n' ends one (getline); byte-parallel, 16 bytes per lane,
//                                       per-tile counts -> scan -> scatter of the line ends in order.
//   fq_record_kernel                    four lines = one record (header, sequence, '+', qualities) with the reference's own
//                                       arithmetic: name = IdentifyHeaderBegPos/EndPos (:29-49), rlen = sequence line length - 1
//                                       (the last character of a line is taken to be the newline, :66-69), qualities cut to rlen.
//   fq_plan_kernel                      how many whole chunks of ReadChunkSize reads the window yields (GetNextChunk's loop, :109-143),
//                                       where the next window starts, and whether something the device path does not take lies ahead
//                                       (an empty read ends a chunk early in the reference; such windows go to the host's reader).
//   fq_materialise_kernel               the reads as the reference holds them: characters as in the file, the second read of a
//                                       pair reverse-complemented (:125-135; GetComplementarySeq, src/tools.cpp:3-29).
// FASTA (kg_stream_set_input; GetNextEntry with FastQFormat == false, :76-104): the same line index, then
//   fa_line_kernel -> scan              every line: is it a header (line 0 of the window, or first byte '>'), and how many sequence characters it
//                                       adds (its length - 1: the last byte is taken to be the newline); the scan of both gives every line its
//                                       record and the characters in front of it
//   fa_head_kernel / fa_record_kernel   the header line of every record; one lane per record: name, first sequence line, number of lines, rlen
//   fa_materialise_kernel               the sequence lines of a read gathered into its characters (a one-line record: fq_materialise_kernel's copy)
// the plan counts records where FASTQ counts four lines; a record is whole only if a header follows it in the window or the file ends there.
// Byte work, HBM-bound, no MFMA.  Everything is integer / character arithmetic; the reads are those of the host pipeline's readers (tests/test_stream_gpu.py).
#include "text_device.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace kg {

namespace {

// 4-bit mask of the bytes of x equal to the byte replicated in pat (bit i = byte i, lowest address first)
__device__ __forceinline__ uint32_t eq_mask4(uint32_t x, uint32_t pat)
{
	uint32_t t = x ^ pat;
	uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);       // 0x80 in every zero byte of t, exactly
	return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// the 16 bytes of this thread: newline mask (and whether a NUL byte lies among them), restricted to the window
__device__ __forceinline__ uint32_t newline_mask16(const FqWindow &w, int64_t p, bool &nul)
{
	nul = false;
	if (p >= w.end || p + 16 <= w.begin) return 0;
	const uint4 v = *reinterpret_cast<const uint4 *>(w.text + p);
	uint32_t nl = eq_mask4(v.x, 0x0A0A0A0Au) | (eq_mask4(v.y, 0x0A0A0A0Au) << 4) | (eq_mask4(v.z, 0x0A0A0A0Au) << 8) | (eq_mask4(v.w, 0x0A0A0A0Au) << 12);
	uint32_t z = eq_mask4(v.x, 0u) | (eq_mask4(v.y, 0u) << 4) | (eq_mask4(v.z, 0u) << 8) | (eq_mask4(v.w, 0u) << 12);
	int lo = (int)(w.begin > p ? w.begin - p : 0), hi = (int)(w.end - p < 16 ? w.end - p : 16);
	uint32_t keep = (hi >= 16 ? 0xFFFFu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
	nul = (z & keep) != 0;
	return nl & keep;
}

struct Widen32 {                       // (the scans of 32-bit lengths into 64-bit offsets)
	__host__ __device__ __forceinline__ int64_t operator()(const int32_t &x) const { return (int64_t)x; }
};
using Wide32Iter = hipcub::TransformInputIterator<int64_t, Widen32, const int32_t *>;

}  // namespace

// ---- lines ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fq_count_kernel(FqArgs a, int f, int64_t n_tiles)
{
	const FqWindow &w = a.w[f];
	const int64_t ta = w.begin & ~(int64_t)15;
	__shared__ int wave_sum[4];
	for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		bool nul;
		uint32_t m = newline_mask16(w, ta + t * kFqTile + (int64_t)threadIdx.x * 16, nul);
		if (nul) a.meta[FQM_NUL] = 1;
		int c = __popc(m);
		for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
		if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
		__syncthreads();
		if (threadIdx.x == 0) w.tile_lines[t] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
		__syncthreads();
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) w.tile_lines[n_tiles] = 0;
}

__global__ __launch_bounds__(256) void fq_index_kernel(FqArgs a, int f, int64_t n_tiles)
{
	const FqWindow &w = a.w[f];
	const int64_t ta = w.begin & ~(int64_t)15;
	__shared__ int wave_sum[4];
	for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		bool nul;
		const int64_t p = ta + t * kFqTile + (int64_t)threadIdx.x * 16;
		uint32_t m = newline_mask16(w, p, nul);
		int c = __popc(m);
		int incl = wave_inclusive_scan(c);
		if ((threadIdx.x & 63) == 63) wave_sum[threadIdx.x >> 6] = incl;
		__syncthreads();
		int64_t at = (int64_t)w.tile_lines[t] + (incl - c);
		for (int q = 0; q < (int)(threadIdx.x >> 6); ++q) at += wave_sum[q];
		while (m) {
			int b = __ffs(m) - 1;
			m &= m - 1;
			if (at < w.line_capacity) w.line_end[at] = (uint32_t)(p + b + 1);
			else a.meta[FQM_OVERFLOW] = 1;
			at++;
		}
		__syncthreads();
	}
	// the total, and the last line of a file that does not end in a newline (getline returns it as it is)
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		int64_t lines = w.tile_lines[n_tiles];
		if (w.eof && w.end > w.begin && w.text[w.end - 1] != '\n') {
			if (lines < w.line_capacity) w.line_end[lines] = (uint32_t)w.end;
			else a.meta[FQM_OVERFLOW] = 1;
			lines++;
		}
		a.meta[FQM_LINES0 + f] = lines;
	}
}

// ---- records -------------------------------------------------------------------------------------------------------------------
// IdentifyHeaderBegPos / IdentifyHeaderEndPos on a header line of `len` bytes (its newline included), src/GetData.cpp:29-49: the name is
// h[p1, p1 + name_len)
__device__ __forceinline__ void parse_header(const uint8_t *h, int len, int &p1, int &name_len)
{
	int p2 = len - 1;
	p1 = len - 1;
	bool f1 = false, f2 = false;
	// (sixteen characters per load -- a header is two or three of them -- instead of a byte load per character, each at a different memory line
	//  per lane; the window has 4 KB of slack behind its last byte)
	for (int base = 0; base < len && !(f1 && f2); base += 16) {
		const U128 u = *reinterpret_cast<const U128 *>(h + base);
		const uint32_t x0 = (uint32_t)u.lo, x1 = (uint32_t)(u.lo >> 32), x2 = (uint32_t)u.hi, x3 = (uint32_t)(u.hi >> 32);
		auto mask16 = [&](uint32_t pat) { return eq_mask4(x0, pat) | (eq_mask4(x1, pat) << 4) | (eq_mask4(x2, pat) << 8) | (eq_mask4(x3, pat) << 12); };
		const int lo = base == 0 ? 1 : 0, hi = len - base < 16 ? len - base : 16;              // characters 1 .. len - 1 of the line
		const uint32_t valid = (hi >= 16 ? 0xFFFFu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
		const uint32_t other = ~(mask16(0x3E3E3E3Eu) | mask16(0x40404040u)) & valid;          // not '>' and not '@'
		const uint32_t sep = (mask16(0x20202020u) | mask16(0x2F2F2F2Fu) | mask16(0x09090909u)) & valid;   // ' ', '/', '\t'
		if (!f1 && other) { p1 = base + __ffs((int)other) - 1; f1 = true; }
		if (!f2 && sep) { p2 = base + __ffs((int)sep) - 1; f2 = true; }
	}
	name_len = p2 > p1 ? p2 - p1 : 0;
}

__global__ __launch_bounds__(256) void fq_record_kernel(FqArgs a, int f)
{
	const FqWindow &w = a.w[f];
	// (launched behind fq_index_kernel of the same window on the same stream: the line count is final)
	int64_t lines = a.meta[FQM_LINES0 + f];
	if (lines > w.line_capacity) lines = w.line_capacity;
	const int64_t recs = lines >> 2;
	for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < recs; j += (int64_t)gridDim.x * blockDim.x) {
		const uint32_t l0 = j == 0 ? (uint32_t)w.begin : w.line_end[4 * j - 1], l1 = w.line_end[4 * j], l2 = w.line_end[4 * j + 1],
		               l3 = w.line_end[4 * j + 2], l4 = w.line_end[4 * j + 3];
		int p1, name_len;
		parse_header(w.text + l0, (int)(l1 - l0), p1, name_len);
		const uint8_t *h = w.text + l0;
		const int rlen = (int)(l2 - l1) - 1;
		int qlen = (int)(l4 - l3);
		if (qlen > rlen) qlen = rlen;
		if (qlen < 0) qlen = 0;
		w.rec_hdr[j] = l0;
		w.rec_name[j] = (uint32_t)(p1 & 0xFFFF) | ((uint32_t)name_len << 16);
		w.rec_seq[j] = l1;
		w.rec_qual[j] = l3;
		w.rec_rlen[j] = rlen;
		w.rec_qlen[j] = qlen;
		// an empty read ends a chunk early in the reference (src/GetData.cpp:117,121); a header too long for the 16-bit fields,
		// a read beyond any short-read length: not taken here
		bool bad = rlen <= 0 || rlen > (1 << 20) || p1 > 0xFFFF || name_len > 0xFFFF;
		// the text of a gz file: gzgets() hands out at most 999 bytes per call (a longer line arrives in pieces that the reference takes for the
		// record's next lines), and an entry whose first line does not start with '@' / '>' or names nothing ends after that line
		// (src/GetData.cpp:152-162): such a record is the caller's line reader's
		if (a.gz_lines) bad = bad || l1 - l0 > 999u || l2 - l1 > 999u || l3 - l2 > 999u || l4 - l3 > 999u || (h[0] != '@' && h[0] != '>') || name_len == 0;
		if (bad) atomicMin((long long *)&a.meta[FQM_BAD0 + f], (long long)j);
		const int64_t i = a.two_files ? 2 * j + f : j;
		if (i < a.max_reads) a.read_len[i] = rlen > 0 ? rlen : 0;
	}
}

// ---- FASTA: lines -> records ------------------------------------------------------------------------------------------------------
// every line of the window: a header counts one record (high word), any other line adds its length - 1 characters (low word: the sum over a
// window stays below 2^32, as the window's bytes do).  Entries [lines, n_scan] are zero, so the scan's entry `lines` holds the totals.
__global__ __launch_bounds__(256) void fa_line_kernel(FqArgs a, int f, int64_t n_scan)
{
	const FqWindow &w = a.w[f];
	int64_t lines = a.meta[FQM_LINES0 + f];
	if (lines > w.line_capacity) lines = w.line_capacity;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_scan; i += (int64_t)gridDim.x * blockDim.x) {
		uint64_t v = 0;
		if (i < lines) {
			const uint32_t l0 = i == 0 ? (uint32_t)w.begin : w.line_end[i - 1], l1 = w.line_end[i];
			v = (i == 0 || w.text[l0] == '>') ? 1ull << 32 : (uint64_t)(l1 - l0 - 1u);
		}
		w.line_acc[i] = v;
	}
}

// (behind the scan) the header line of every record, the number of lines behind the last one, and the record count
__global__ __launch_bounds__(256) void fa_head_kernel(FqArgs a, int f)
{
	const FqWindow &w = a.w[f];
	int64_t lines = a.meta[FQM_LINES0 + f];
	if (lines > w.line_capacity) lines = w.line_capacity;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < lines; i += (int64_t)gridDim.x * blockDim.x) {
		const int64_t j = (int64_t)(w.line_acc[i] >> 32);
		if ((int64_t)(w.line_acc[i + 1] >> 32) != j && j < w.rec_capacity) w.rec_line[j] = (uint32_t)i;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		// (more records than the table holds: the plan takes nothing, FQM_OVERFLOW; the table's last record then simply runs to the last line, so that
		//  every entry fa_record_kernel reads has been written)
		const int64_t recs = (int64_t)(w.line_acc[lines] >> 32);
		w.rec_line[recs <= w.rec_capacity ? recs : w.rec_capacity] = (uint32_t)lines;
		if (recs > w.rec_capacity) a.meta[FQM_OVERFLOW] = 1;
		a.meta[FQM_RECS0 + f] = recs;
	}
}

// one lane per record (GetNextEntry, src/GetData.cpp:76-104 / gzGetNextEntry :145-182)
__global__ __launch_bounds__(256) void fa_record_kernel(FqArgs a, int f)
{
	const FqWindow &w = a.w[f];
	int64_t recs = a.meta[FQM_RECS0 + f];
	if (recs > w.rec_capacity) recs = w.rec_capacity;
	int64_t lines = a.meta[FQM_LINES0 + f];
	if (lines > w.line_capacity) lines = w.line_capacity;
	for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < recs; j += (int64_t)gridDim.x * blockDim.x) {
		const uint32_t hl = w.rec_line[j], nx = w.rec_line[j + 1];
		// (fa_head_kernel wrote both: a header line, and a later line or the number of lines.  Nothing below is indexed by anything else)
		if (!(hl < nx && (int64_t)nx <= lines)) { a.meta[FQM_OVERFLOW] = 1; continue; }
		const uint32_t l0 = hl == 0 ? (uint32_t)w.begin : w.line_end[hl - 1], l1 = w.line_end[hl];
		int p1, name_len;
		parse_header(w.text + l0, (int)(l1 - l0), p1, name_len);
		const int n_seq = (int)(nx - hl) - 1;
		const uint32_t chars = (uint32_t)w.line_acc[nx] - (uint32_t)w.line_acc[hl];
		const int rlen = chars > (1u << 20) ? (1 << 20) + 1 : (int)chars;
		w.rec_hdr[j] = l0;
		w.rec_name[j] = (uint32_t)(p1 & 0xFFFF) | ((uint32_t)name_len << 16);
		w.rec_seq[j] = l1;
		w.rec_qual[j] = hl + 1;
		w.rec_rlen[j] = rlen;
		w.rec_qlen[j] = n_seq;
		// an empty read ends a chunk early in the reference (src/GetData.cpp:116,124); a header too long for the 16-bit fields, a read beyond any
		// short-read length: not taken here
		bool bad = rlen <= 0 || rlen > (1 << 20) || p1 > 0xFFFF || name_len > 0xFFFF;
		// the text of a gz file: exactly one sequence line per entry, at most 999 bytes per gzgets() call, and an entry whose first line does not
		// start with '@' / '>' or names nothing is empty (:152-167)
		if (a.gz_lines) {
			const uint8_t c = w.text[l0];
			bad = bad || n_seq != 1 || l1 - l0 > 999u || (n_seq >= 1 && w.line_end[hl + 1] - l1 > 999u) || (c != '@' && c != '>') || name_len == 0;
		}
		// (the window's last record may go on in the next window: the plan does not take it, and what it looks like so far says nothing)
		if (bad && (j + 1 < recs || w.eof)) atomicMin((long long *)&a.meta[FQM_BAD0 + f], (long long)j);
		const int64_t i = a.two_files ? 2 * j + f : j;
		if (i < a.max_reads) a.read_len[i] = rlen > 0 ? rlen : 0;
	}
}

__global__ void fq_reset_kernel(FqArgs a)
{
	const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i0 < FQM_WORDS) a.meta[i0] = (i0 == FQM_BAD0 || i0 == FQM_BAD1) ? 0x7fffffffffffffffll : 0;
	for (int64_t i = i0; i <= a.max_reads; i += (int64_t)gridDim.x * blockDim.x) a.read_len[i] = 0;
}

// GetNextChunk's loop over the window: whole chunks only, unless the files end here in a regular way
__global__ void fq_plan_kernel(FqArgs a)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	const int64_t kNone = 0x7fffffffffffffffll;
	const int64_t L0 = a.meta[FQM_LINES0], L1 = a.two_files ? a.meta[FQM_LINES1] : 0;
	// whole records of either window.  FASTA: a record is whole only if a header line follows it in the window, or the window ends where the file does
	// (its sequence may go on in the next window)
	const int64_t R0 = a.fasta ? a.meta[FQM_RECS0] : 0, R1 = a.fasta && a.two_files ? a.meta[FQM_RECS1] : 0;
	const int64_t recs0 = a.fasta ? (a.w[0].eof || R0 == 0 ? R0 : R0 - 1) : L0 >> 2, recs1 = a.fasta ? (a.w[1].eof || R1 == 0 ? R1 : R1 - 1) : L1 >> 2;
	int64_t avail, bad = kNone;
	if (a.two_files) {
		avail = 2 * (recs0 < recs1 ? recs0 : recs1);
		if (a.meta[FQM_BAD0] != kNone) bad = 2 * a.meta[FQM_BAD0];
		if (a.meta[FQM_BAD1] != kNone && 2 * a.meta[FQM_BAD1] + 1 < bad) bad = 2 * a.meta[FQM_BAD1] + 1;
	} else {
		avail = recs0;
		bad = a.meta[FQM_BAD0];
	}
	const bool at_eof = a.w[0].eof && (!a.two_files || a.w[1].eof);
	const bool whole_records = a.fasta || ((L0 & 3) == 0 && (!a.two_files || (L1 & 3) == 0));
	const bool regular_end = at_eof && whole_records && (!a.two_files || recs0 == recs1) && (!(a.paired && !a.two_files) || (recs0 & 1) == 0);
	int64_t take = avail < a.want_reads ? avail : a.want_reads;
	int64_t stop = FQ_STOP_NONE;
	if (bad < take) { take = bad; stop = FQ_STOP_IRREGULAR; }
	if (a.meta[FQM_NUL] || a.meta[FQM_OVERFLOW]) { take = 0; stop = FQ_STOP_IRREGULAR; }
	const bool full = stop == FQ_STOP_NONE && take == avail && regular_end;
	if (!full) {
		take = take / a.chunk_reads * a.chunk_reads;
		// the rest of the file is less than a chunk and does not end in the regular way (a lone mate, a partial record): the host's
		// reader takes it from here
		if (stop == FQ_STOP_NONE && at_eof && avail - take < a.chunk_reads) stop = FQ_STOP_TAIL;
	}
	const int64_t t0 = a.two_files ? take >> 1 : take, t1 = a.two_files ? take >> 1 : 0;
	a.meta[FQM_READS] = take;
	a.meta[FQM_CHUNKS] = (take + a.chunk_reads - 1) / a.chunk_reads;
	a.meta[FQM_BASES] = a.read_off[take];
	if (a.fasta) {
		// the header of the first record not taken (rec_line[R] = the number of lines: behind the last line)
		auto start_of = [](const FqWindow &w, int64_t t) { const uint32_t l = t ? w.rec_line[t] : 0u; return l ? (int64_t)w.line_end[l - 1] : w.begin; };
		a.meta[FQM_USED0] = start_of(a.w[0], t0);
		a.meta[FQM_USED1] = a.two_files ? start_of(a.w[1], t1) : 0;
	} else {
		a.meta[FQM_USED0] = t0 ? (int64_t)a.w[0].line_end[4 * t0 - 1] : a.w[0].begin;
		a.meta[FQM_USED1] = a.two_files ? (t1 ? (int64_t)a.w[1].line_end[4 * t1 - 1] : a.w[1].begin) : 0;
	}
	a.meta[FQM_STOP] = stop;
	a.meta[FQM_DONE] = full ? 1 : 0;
}

// ---- the long pieces (bases, qualities) by EIGHT lanes per line: lane `sub` of the eight moves bytes [16 sub + 128 k, 16 sub + 128 k + 16) -- the eight cover 128
// consecutive bytes per step.  With a line per lane the 64 lanes of a load touched 64 different 128-byte lines for 16 bytes each, and the lines did not
// stay in the L2 until the lane came back for the next 16: the counters showed 242 GB per 100 M reads moved by sam_format_kernel for 76 GB of text, 181 GB
// by fq_materialise_kernel for 31 GB (profiles/r05zj_bench_pmc_summary.json).  Exact: nothing is written outside [p, p + n).
__device__ __forceinline__ void group_copy(uint8_t *p, const uint8_t *src, int n, int sub)
{
	for (int off = sub << 4; off < n; off += 128) {
		if (off + 16 <= n) *reinterpret_cast<U128 *>(p + off) = *reinterpret_cast<const U128 *>(src + off);
		else for (int k = off; k < n; ++k) p[k] = src[k];
	}
}

template <bool kComp>
__device__ __forceinline__ void group_copy_reversed(uint8_t *p, const uint8_t *src, int n, int sub)
{
	for (int off = sub << 4; off < n; off += 128) {
		if (off + 16 <= n) {
			const U128 v = *reinterpret_cast<const U128 *>(src + n - 16 - off);
			U128 o;
			o.lo = __builtin_bswap64(v.hi); o.hi = __builtin_bswap64(v.lo);
			if (kComp) { o.lo = comp8(o.lo); o.hi = comp8(o.hi); }
			*reinterpret_cast<U128 *>(p + off) = o;
		} else for (int k = off; k < n; ++k) p[k] = kComp ? comp_char(src[n - 1 - k]) : src[n - 1 - k];
	}
}

// EIGHT lanes per read (round 5; a wave per read and a byte per lane in rounds 3-4, then a lane per read): its characters into the batch's character
// array, reverse-complemented for the second read of a pair -- 16 bytes per lane, 128 consecutive bytes per group and step (group_copy above)
__global__ __launch_bounds__(256) void fq_materialise_kernel(FqArgs a)
{
	const int sub = threadIdx.x & 7;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; i < a.n_reads; i += ((int64_t)gridDim.x * blockDim.x) >> 3) {
		const int f = a.two_files ? (int)(i & 1) : 0;
		const int64_t j = a.two_files ? i >> 1 : i;
		const FqWindow &w = a.w[f];
		const uint8_t *src = w.text + w.rec_seq[j];
		const int n = w.rec_rlen[j];
		uint8_t *dst = a.enc + a.read_off[i];
		if (a.paired && (i & 1)) group_copy_reversed<true>(dst, src, n, sub);
		else group_copy(dst, src, n, sub);
	}
}

// FASTA: one sequence line of n characters by the eight lanes of its read.  As group_copy, but a line's last partial piece goes as the line's LAST sixteen
// bytes (it overlaps the piece before it with the same bytes) instead of byte by byte: a 60-column line is three whole pieces and one such.  Exact as well.
__device__ __forceinline__ void line_copy(uint8_t *p, const uint8_t *src, int n, int sub)
{
	for (int off = sub << 4; off < n; off += 128) {
		const int at = off + 16 <= n ? off : n - 16;
		if (at >= 0) *reinterpret_cast<U128 *>(p + at) = *reinterpret_cast<const U128 *>(src + at);
		else for (int k = off; k < n; ++k) p[k] = src[k];
	}
}

__device__ __forceinline__ void line_copy_revcomp(uint8_t *p, const uint8_t *src, int n, int sub)
{
	for (int off = sub << 4; off < n; off += 128) {
		const int at = off + 16 <= n ? off : n - 16;
		if (at >= 0) {
			const U128 v = *reinterpret_cast<const U128 *>(src + n - 16 - at);
			U128 o;
			o.lo = comp8(__builtin_bswap64(v.hi)); o.hi = comp8(__builtin_bswap64(v.lo));
			*reinterpret_cast<U128 *>(p + at) = o;
		} else for (int k = off; k < n; ++k) p[k] = comp_char(src[n - 1 - k]);
	}
}

// FASTA: eight lanes per read as above.  A record of one sequence line is the FASTQ case; otherwise line by line -- every line's characters but its last
// byte behind those of the lines before it, or (mate 2) in front of them, reverse-complemented
__global__ __launch_bounds__(256) void fa_materialise_kernel(FqArgs a)
{
	const int sub = threadIdx.x & 7;
	for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; i < a.n_reads; i += ((int64_t)gridDim.x * blockDim.x) >> 3) {
		const int f = a.two_files ? (int)(i & 1) : 0;
		const int64_t j = a.two_files ? i >> 1 : i;
		const FqWindow &w = a.w[f];
		uint32_t ls = w.rec_seq[j];
		const int n = w.rec_rlen[j], n_lines = w.rec_qlen[j];
		uint8_t *dst = a.enc + a.read_off[i];
		const bool rc = a.paired && (i & 1);
		if (n_lines == 1) {
			if (rc) group_copy_reversed<true>(dst, w.text + ls, n, sub);
			else group_copy(dst, w.text + ls, n, sub);
			continue;
		}
		const uint32_t *le = w.line_end + w.rec_qual[j];
		int at = 0;
		for (int k = 0; k < n_lines; ++k) {
			const uint32_t e = le[k];
			const int m = (int)(e - ls) - 1;
			if (rc) line_copy_revcomp(dst + (n - at - m), w.text + ls, m, sub);
			else line_copy(dst + at, w.text + ls, m, sub);
			at += m;
			ls = e;
		}
	}
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
hipError_t scan_lengths(const int32_t *len, int64_t *off, int64_t n, void *temp, size_t temp_bytes, hipStream_t stream)
{
	Wide32Iter it(len, Widen32());
	size_t need = 0;
	hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, it, off, (int)n, stream);
	if (e != hipSuccess) return e;
	if (need > temp_bytes) return hipErrorInvalidValue;
	return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, it, off, (int)n, stream);
}

size_t fq_scan_temp_bytes(int64_t max_items)
{
	size_t b1 = 0, b2 = 0;
	Wide32Iter it((const int32_t *)nullptr, Widen32());
	(void)hipcub::DeviceScan::ExclusiveSum(nullptr, b1, it, (int64_t *)nullptr, (int)max_items);
	(void)hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (const int32_t *)nullptr, (int32_t *)nullptr, (int)max_items);
	return b1 > b2 ? b1 : b2;
}

size_t fa_scan_temp_bytes(int64_t max_lines)
{
	size_t b = 0;
	(void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)(max_lines + 1));
	return b;
}

hipError_t launch_fq_parse(const FqArgs &a, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream)
{
	hipError_t e;
	kt_begin(KT_FQ_PARSE, stream);
	hipLaunchKernelGGL(fq_reset_kernel, dim3(grid_of(a.max_reads + 1, 256, n_cu * 8)), dim3(256), 0, stream, a);
	for (int f = 0; f < (a.two_files ? 2 : 1); ++f) {
		const FqWindow &w = a.w[f];
		const int64_t ta = w.begin & ~(int64_t)15;
		const int64_t n_tiles = w.end > ta ? (w.end - ta + kFqTile - 1) / kFqTile : 0;
		hipLaunchKernelGGL(fq_count_kernel, dim3(grid_of(n_tiles, 1, n_cu * 64)), dim3(256), 0, stream, a, f, n_tiles);
		size_t tb = scan_temp_bytes;
		if ((e = hipcub::DeviceScan::ExclusiveSum(scan_temp, tb, (const int32_t *)w.tile_lines, w.tile_lines, (int)(n_tiles + 1), stream)) != hipSuccess) return e;
		hipLaunchKernelGGL(fq_index_kernel, dim3(grid_of(n_tiles, 1, n_cu * 64)), dim3(256), 0, stream, a, f, n_tiles);
		if (a.fasta) {
			// (a line is at least one byte: the window holds no more lines than bytes)
			const int64_t n_scan = std::min<int64_t>(w.line_capacity, w.end - w.begin + 1);
			hipLaunchKernelGGL(fa_line_kernel, dim3(grid_of(n_scan + 1, 256, n_cu * 16)), dim3(256), 0, stream, a, f, n_scan);
			tb = scan_temp_bytes;
			if ((e = hipcub::DeviceScan::ExclusiveSum(scan_temp, tb, (const uint64_t *)w.line_acc, w.line_acc, (int)(n_scan + 1), stream)) != hipSuccess) return e;
			hipLaunchKernelGGL(fa_head_kernel, dim3(grid_of(n_scan, 256, n_cu * 16)), dim3(256), 0, stream, a, f);
			hipLaunchKernelGGL(fa_record_kernel, dim3(grid_of(std::min<int64_t>(w.rec_capacity, n_scan), 256, n_cu * 16)), dim3(256), 0, stream, a, f);
		} else
		hipLaunchKernelGGL(fq_record_kernel, dim3(grid_of(w.line_capacity / 4, 256, n_cu * 16)), dim3(256), 0, stream, a, f);
	}
	if ((e = scan_lengths(a.read_len, a.read_off, a.max_reads + 1, scan_temp, scan_temp_bytes, stream)) != hipSuccess) return e;
	hipLaunchKernelGGL(fq_plan_kernel, dim3(1), dim3(64), 0, stream, a);
	kt_end(KT_FQ_PARSE, stream);
	return hipGetLastError();
}

hipError_t launch_fq_materialise(const FqArgs &a, int n_cu, hipStream_t stream)
{
	if (a.n_reads <= 0) return hipSuccess;
	kt_begin(KT_FQ_MATERIALISE, stream);
	if (a.fasta) hipLaunchKernelGGL(fa_materialise_kernel, dim3(grid_of(a.n_reads * 8, 256, n_cu * 16)), dim3(256), 0, stream, a);
	else hipLaunchKernelGGL(fq_materialise_kernel, dim3(grid_of(a.n_reads * 8, 256, n_cu * 16)), dim3(256), 0, stream, a);
	kt_end(KT_FQ_MATERIALISE, stream);
	return hipGetLastError();
}

// ---- grouped seeding (abi_stream.hip): a lane's batch as one segment of its group's batch ------------------------------------------
// slot i of the segment: offset of the read in the GROUP's character array (the lane's part starts at enc_base) and its length;
// the slots behind the n reads are empty
__global__ __launch_bounds__(256) void group_publish_kernel(const int64_t *local_off, int64_t n, int64_t slots, int64_t enc_base, int64_t *g_off, int32_t *g_len)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride) {
		const int64_t at = local_off[i < n ? i : n];
		g_off[i] = enc_base + at;
		g_len[i] = i < n ? (int32_t)(local_off[i + 1] - at) : 0;
	}
}

// the lane's seed offsets out of the group's: seed_off[i] = g_seed_off[i] - first, i = 0 .. n (the slot behind a segment's last read
// holds the segment's end: empty slots have no seeds)
__global__ __launch_bounds__(256) void group_rebase_kernel(const int64_t *g_seed_off, int64_t n, int64_t first, int64_t *seed_off)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) seed_off[i] = g_seed_off[i] - first;
}

hipError_t launch_group_publish(const int64_t *local_off, int64_t n, int64_t slots, int64_t enc_base, int64_t *g_off, int32_t *g_len, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(group_publish_kernel, dim3(grid_of(slots, 256, n_cu * 8)), dim3(256), 0, stream, local_off, n, slots, enc_base, g_off, g_len);
	return hipGetLastError();
}

hipError_t launch_group_rebase(const int64_t *g_seed_off, int64_t n, int64_t first, int64_t *seed_off, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(group_rebase_kernel, dim3(grid_of(n + 1, 256, n_cu * 8)), dim3(256), 0, stream, g_seed_off, n, first, seed_off);
	return hipGetLastError();
}

}  // namespace kg
