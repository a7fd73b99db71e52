// stream_kernels.hip -- FASTQ or FASTA text in, SAM text or BAM records out, on the device (gfx950).
//
// Input side = GetNextChunk / GetNextEntry (reference src/GetData.cpp:29-143) for a whole window of text at once:
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
// Output side = OutputPairedAlignments / OutputSingledAlignments (src/Mapping.cpp:177-315) for every kg_aln_record of the batch:
//   sam_size_kernel                     exact byte count of the line(s) of every read -> scan -> offsets
//   sam_format_kernel                   one wave per 64 reads: every lane prints the numeric fields of one read into the LDS, then all
//                                       lanes move each read's pieces -- name, FLAG .. TLEN, sequence (reverse-complemented for a
//                                       record shown on the other strand), qualities (reversed likewise), NM / AS / XS.
//   bam_size_kernel / bam_format_kernel the same records as BAM (kg_stream_set_format): fixed-width fields, bases packed to 4 bits, qualities less 33
//   (all four are templates on kMd: with kg_stream_set_tags(KG_STREAM_TAG_MD) every mapped record carries MD:Z behind XS, kernels/md_tag.inc; without, the
//   instantiation is the code as it was before the tag existed; and on kRg: with kg_stream_set_read_group EVERY record carries RG:Z as its last field,
//   a constant of the batch copied from SamArgs::rg like a contig name -- the line feed of a SAM line then comes from the copy, not from the tags)
// Byte work, HBM-bound, no MFMA.  Everything is integer / character arithmetic; results are bit-identical to the host pipeline's
// text (tests/test_stream_gpu.py, and every SAM parity test runs through this path).
#include "stream_kernels.hpp"

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

__device__ __forceinline__ int wave_inclusive_scan(int v)
{
	const int lane = threadIdx.x & 63;
	for (int d = 1; d < 64; d <<= 1) {
		int t = __shfl_up(v, d);
		if (lane >= d) v += t;
	}
	return v;
}

}  // namespace

// sixteen bytes at any address (one unaligned load / store)
struct __attribute__((packed, aligned(1))) SamU128 { uint64_t lo, hi; };

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
		const SamU128 u = *reinterpret_cast<const SamU128 *>(h + base);
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

// GetComplementaryBase, src/tools.cpp:3-17
__device__ __forceinline__ uint8_t comp_char(uint8_t c)
{
	const uint8_t u = c & 0xDFu;
	return u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N';
}

// ---- one line by ONE lane, 16 bytes per load and store (round 5).  Rounds 3-4 moved a line with all 64 lanes, a byte per lane and instruction: 31 bytes per
// store instruction, the largest kernel of a run; assembling lines in the LDS first (the verdict's suggestion) was slower still -- 41 ms against 31 ms per 20 M
// reads at 4 KB, 61 ms at 16 KB: fewer waves per CU for the same byte-wide loads (profiles/r05t_ab_sam_buf.log).  Here every lane copies its OWN read's line
// piece by piece with unaligned 16-byte accesses: a wave instruction moves 1 KB, and the 64 lines of a wave are consecutive in the output.  A piece's last
// partial word is copied whole where the line still has room behind it (the next piece overwrites the surplus), byte by byte at the line's end.

__device__ __forceinline__ uint64_t comp8(uint64_t x)          // GetComplementaryBase (src/tools.cpp:3-17) on eight characters
{
	const uint64_t u = x & 0xDFDFDFDFDFDFDFDFull;
	auto is = [&](uint64_t c) { const uint64_t t = u ^ (c * 0x0101010101010101ull); return ((~(((t & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | t | 0x7F7F7F7F7F7F7F7Full)) >> 7) * 0xFFull; };
	const uint64_t mA = is(0x41), mC = is(0x43), mG = is(0x47), mT = is(0x54);
	return (mA & 0x5454545454545454ull) | (mC & 0x4747474747474747ull) | (mG & 0x4343434343434343ull) | (mT & 0x4141414141414141ull) | (~(mA | mC | mG | mT) & 0x4E4E4E4E4E4E4E4Eull);
}

// n bytes of src to p; `end` = the end of the line (writing up to 15 bytes past the piece is fine below it)
__device__ __forceinline__ uint8_t *lane_copy(uint8_t *p, const uint8_t *end, const uint8_t *src, int n)
{
	int k = 0;
	for (; k + 16 <= n; k += 16) *reinterpret_cast<SamU128 *>(p + k) = *reinterpret_cast<const SamU128 *>(src + k);
	if (k < n) {
		if (p + k + 16 <= end) *reinterpret_cast<SamU128 *>(p + k) = *reinterpret_cast<const SamU128 *>(src + k);
		else for (; k < n; ++k) p[k] = src[k];
	}
	return p + n;
}

// the same with the source read backwards (qualities reversed; kComp: the reverse complement of the bases, GetComplementarySeq src/tools.cpp:19-29)
template <bool kComp>
__device__ __forceinline__ uint8_t *lane_copy_reversed(uint8_t *p, const uint8_t *src, int n)
{
	int k = 0;
	for (; k + 16 <= n; k += 16) {
		const SamU128 v = *reinterpret_cast<const SamU128 *>(src + n - 16 - k);
		SamU128 o;
		o.lo = __builtin_bswap64(v.hi); o.hi = __builtin_bswap64(v.lo);
		if (kComp) { o.lo = comp8(o.lo); o.hi = comp8(o.hi); }
		*reinterpret_cast<SamU128 *>(p + k) = o;
	}
	for (; k < n; ++k) p[k] = kComp ? comp_char(src[n - 1 - k]) : src[n - 1 - k];
	return p + n;
}

// ---- the long pieces (bases, qualities) by EIGHT lanes per line: lane `sub` of the eight moves bytes [16 sub + 128 k, 16 sub + 128 k + 16) -- the eight cover 128
// consecutive bytes per step.  With a line per lane the 64 lanes of a load touched 64 different 128-byte lines for 16 bytes each, and the lines did not
// stay in the L2 until the lane came back for the next 16: the counters showed 242 GB per 100 M reads moved by sam_format_kernel for 76 GB of text, 181 GB
// by fq_materialise_kernel for 31 GB (profiles/r05zj_bench_pmc_summary.json).  Exact: nothing is written outside [p, p + n).
__device__ __forceinline__ void group_copy(uint8_t *p, const uint8_t *src, int n, int sub)
{
	for (int off = sub << 4; off < n; off += 128) {
		if (off + 16 <= n) *reinterpret_cast<SamU128 *>(p + off) = *reinterpret_cast<const SamU128 *>(src + off);
		else for (int k = off; k < n; ++k) p[k] = src[k];
	}
}

template <bool kComp>
__device__ __forceinline__ void group_copy_reversed(uint8_t *p, const uint8_t *src, int n, int sub)
{
	for (int off = sub << 4; off < n; off += 128) {
		if (off + 16 <= n) {
			const SamU128 v = *reinterpret_cast<const SamU128 *>(src + n - 16 - off);
			SamU128 o;
			o.lo = __builtin_bswap64(v.hi); o.hi = __builtin_bswap64(v.lo);
			if (kComp) { o.lo = comp8(o.lo); o.hi = comp8(o.hi); }
			*reinterpret_cast<SamU128 *>(p + off) = o;
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
		if (at >= 0) *reinterpret_cast<SamU128 *>(p + at) = *reinterpret_cast<const SamU128 *>(src + at);
		else for (int k = off; k < n; ++k) p[k] = src[k];
	}
}

__device__ __forceinline__ void line_copy_revcomp(uint8_t *p, const uint8_t *src, int n, int sub)
{
	for (int off = sub << 4; off < n; off += 128) {
		const int at = off + 16 <= n ? off : n - 16;
		if (at >= 0) {
			const SamU128 v = *reinterpret_cast<const SamU128 *>(src + n - 16 - at);
			SamU128 o;
			o.lo = comp8(__builtin_bswap64(v.hi)); o.hi = comp8(__builtin_bswap64(v.lo));
			*reinterpret_cast<SamU128 *>(p + at) = o;
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

// ---- SAM text ------------------------------------------------------------------------------------------------------------------
namespace {

// the quality column of a read without qualities (FASTA)
__device__ const uint8_t kNoQual[16] = {'*'};

// characters "%d" / "%lld" print.  Every number of a SAM line fits 32 bits in practice (positions are contig-relative, contig
// lengths are 32-bit in the index format); 32-bit division by the constant 10 is a multiply, a 64-bit one a subroutine.
__device__ __forceinline__ int u32_chars(uint32_t u)
{
	return u < 10u ? 1 : u < 100u ? 2 : u < 1000u ? 3 : u < 10000u ? 4 : u < 100000u ? 5 : u < 1000000u ? 6 : u < 10000000u ? 7 : u < 100000000u ? 8 : u < 1000000000u ? 9 : 10;
}
__device__ __forceinline__ int int_chars(long long v)
{
	if (v >= -2147483647ll && v <= 2147483647ll) {
		const int x = (int)v;
		return x < 0 ? 1 + u32_chars((uint32_t)(-x)) : u32_chars((uint32_t)x);
	}
	int n = v < 0 ? 2 : 1;
	unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
	while (u >= 10) { u /= 10; n++; }
	return n;
}

__device__ __forceinline__ char *put_int(char *p, long long v)
{
	if (v >= -2147483647ll && v <= 2147483647ll) {
		const int x = (int)v;
		uint32_t u = x < 0 ? (uint32_t)(-x) : (uint32_t)x;
		if (x < 0) *p++ = '-';
		const int n = u32_chars(u);
		for (int i = n - 1; i >= 0; --i) { p[i] = (char)('0' + (int)(u % 10u)); u /= 10u; }
		return p + n;
	}
	const int n = int_chars(v);
	unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
	if (v < 0) p[0] = '-';
	for (int i = n - 1; i >= (v < 0 ? 1 : 0); --i) { p[i] = (char)('0' + (int)(u % 10)); u /= 10; }
	return p + n;
}

__device__ __forceinline__ char *put_lit(char *p, const char *s, int n)
{
	for (int i = 0; i < n; ++i) p[i] = s[i];
	return p + n;
}

struct ReadText {                      // where the name and the qualities of read r lie, and its length
	const uint8_t *name, *qual;
	int name_len, qlen, rlen;
	bool held_reversed;                // the second read of a pair: held reverse-complemented, its qualities reversed
};

__device__ __forceinline__ ReadText read_text(const SamArgs &a, int64_t r)
{
	const int f = a.two_files ? (int)(r & 1) : 0;
	const int64_t j = a.two_files ? r >> 1 : r;
	const FqWindow &w = a.w[f];
	ReadText t;
	const uint32_t nm = w.rec_name[j];
	t.name = w.text + w.rec_hdr[j] + (nm & 0xFFFFu);
	t.name_len = (int)(nm >> 16);
	t.qual = a.fasta ? kNoQual : w.text + w.rec_qual[j];
	t.qlen = a.fasta ? 1 : w.rec_qlen[j];
	t.rlen = (int)(a.read_off[r + 1] - a.read_off[r]);
	t.held_reversed = a.paired && (r & 1);
	return t;
}

#define SAM_UNMAPPED_MID "\t*\t0\t0\t*\t*\t0\t0\t"
#define SAM_UNMAPPED_TAIL "\tAS:i:0\tXS:i:0\n"

#include "kernels/md_tag.inc"

// MD in a lane's LDS slot (the lane-per-read path of either format kernel): at most this many characters; a record with a longer one takes the
// record-by-record path, which prints it straight into the output
constexpr int kMdLds = 58;

// the bytes of the read group field behind a record (SamArgs::rg), where the kernel writes one
template <bool kRg> __device__ __forceinline__ int rg_bytes(const SamArgs &a)
{
	if constexpr (kRg) return a.rg_len;
	else return 0;
}

// the bytes of one record's line (src/Mapping.cpp:181-186 / 225-230 unmapped, :199-223 / 246-262 / 297-302 mapped); kMd: "\tMD:Z:" and the string;
// kRg: "\tRG:Z:<ID>" on either kind
template <bool kMd, bool kRg>
__device__ int record_size(const SamArgs &a, const ReadText &t, const kg_aln_record &rec, const uint8_t *seq, const MdArg<kMd> &md)
{
	if (rec.kind == KG_ALN_UNMAPPED)
		return t.name_len + 1 + int_chars(rec.flag) + (int)(sizeof(SAM_UNMAPPED_MID) - 1) + t.rlen + 1 + t.qlen + (int)(sizeof(SAM_UNMAPPED_TAIL) - 1) + rg_bytes<kRg>(a);
	if (rec.kind != KG_ALN_MAPPED) return 0;
	int n = t.name_len + 1 + int_chars(rec.flag) + 1 + (a.chr_name_off[rec.chr + 1] - a.chr_name_off[rec.chr]) + 1 + int_chars(rec.pos) + 1 + int_chars(rec.mapq) + 1 + rec.cigar_len;
	n += rec.has_mate ? 3 + int_chars(rec.mate_pos) + 1 + int_chars(rec.tlen) + 1 : 7;
	n += t.rlen + 1 + t.qlen;
	n += 6 + int_chars(t.rlen - rec.score) + 6 + int_chars(rec.score) + 6 + int_chars(rec.sub_score) + 1;
	if constexpr (kMd) {
		MdCount c;
		md_walk(md.r, rec, seq, t.rlen, c);
		n += 6 + c.n;
	}
	return n + rg_bytes<kRg>(a);
}

}  // namespace

template <bool kMd, bool kRg>
__global__ __launch_bounds__(256) void sam_size_kernel(SamArgs a, MdArg<kMd> md)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const kg_aln_record &first = a.records[r];
		int n = 0;
		if (first.kind == KG_ALN_HOST) {
			a.host_list[atomicAdd(&a.ctl[0], 1ull)] = (int32_t)r;
		} else {
			const ReadText t = read_text(a, r);
			for (int64_t at = r; at >= 0; at = a.records[at].next) n += record_size<kMd, kRg>(a, t, a.records[at], a.enc + a.read_off[r], md);
		}
		a.sam_len[r] = n;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) a.sam_len[a.n_reads] = 0;
}

// One wave per 64 consecutive reads, two phases.
//   1. lane l prints the numeric fields of read base + l ("\tFLAG\t", "\tPOS\tMAPQ\tCIGAR\t=\tPNEXT\tTLEN\t", the tags) into its own slot
//      of the wave's LDS block and leaves there what the copy phase needs (where the name, the qualities, the characters and the
//      contig name lie, where the line goes): 64 records are fetched and printed side by side, not one after the other.
//   2. for each of the 64 reads all lanes move the pieces -- name, contig name, sequence and qualities straight from the FASTQ
//      text / the read characters -- to the output; everything this phase needs per read comes from the LDS.
// A read with further records chained behind it (-m) takes the record-by-record path (format_chain).
namespace {

constexpr int kFmtA = 16, kFmtB = 96, kFmtT = 64, kFmtSlot = kFmtA + kFmtB + kFmtT;     // bytes of a lane's strings (every string 16-byte aligned: they are read back 16 bytes at a time)
// with MD:Z: the tags in front of it (three numbers of at most 11 characters: 52 with the line feed), "\tMD:Z:" and kMdLds characters
constexpr int kFmtTMd = 128, kFmtSlotMd = kFmtA + kFmtB + kFmtTMd;
static_assert(52 + 6 + kMdLds <= kFmtTMd && kFmtTMd % 16 == 0 && kFmtTMd < 256, "the tags with MD must fit the lane's slot and FmtDesc::nT");

struct FmtDesc {                       // what phase 2 needs for one read
	const uint8_t *name, *qual, *seq, *chr;
	uint8_t *out;
	int32_t room_end_lo;               // (low bits of the end offset: checked against the bytes written)
	int16_t name_len, n_chr, rlen, qlen;
	uint8_t nA, nB, nT, flags;         // flags: 1 print, 2 reverse-complement, 4 qualities reversed, 8 chained records follow
};

// the fields of one record as text: A = "\tFLAG[\t]", B = the middle, T = the tags
// kMdMode 0: no MD:Z (the code as it was).  1: a mapped record's MD behind XS, in T -- md_over: it has more than kMdLds characters and T is not whole.
// 2: T of a mapped record ends behind XS; the caller prints "\tMD:Z:", the string and the line feed itself (print_md_tail)
// kRg: T of either kind ends before the line feed: the caller puts the read group (SamArgs::rg) and the line feed behind the last field
template <int kMdMode, bool kRg>
__device__ __forceinline__ void print_fields(const ReadText &t, const kg_aln_record &rec, char *A, char *B, char *T, int &nA, int &nB, int &nT, const MdRef *R = nullptr,
                                             const uint8_t *seq = nullptr, bool *md_over = nullptr)
{
	const bool mapped = rec.kind == KG_ALN_MAPPED;
	char *q = A;
	*q++ = '\t'; q = put_int(q, rec.flag);
	if (mapped) *q++ = '\t';
	nA = (int)(q - A);
	q = B;
	if (mapped) {
		*q++ = '\t'; q = put_int(q, rec.pos); *q++ = '\t'; q = put_int(q, rec.mapq); *q++ = '\t';
		for (int i = 0; i < rec.cigar_len; ++i) *q++ = rec.cigar[i];
		if (rec.has_mate) { q = put_lit(q, "\t=\t", 3); q = put_int(q, rec.mate_pos); *q++ = '\t'; q = put_int(q, rec.tlen); *q++ = '\t'; }
		else q = put_lit(q, "\t*\t0\t0\t", 7);
	} else q = put_lit(q, SAM_UNMAPPED_MID, (int)(sizeof(SAM_UNMAPPED_MID) - 1));
	nB = (int)(q - B);
	q = T;
	if (mapped) {
		q = put_lit(q, "\tNM:i:", 6); q = put_int(q, t.rlen - rec.score);
		q = put_lit(q, "\tAS:i:", 6); q = put_int(q, rec.score);
		q = put_lit(q, "\tXS:i:", 6); q = put_int(q, rec.sub_score);
		if constexpr (kMdMode == 1) {
			q = put_lit(q, "\tMD:Z:", 6);
			MdWrite w(q, kMdLds);
			md_walk(*R, rec, seq, t.rlen, w);
			*md_over = w.n > kMdLds;
			q += w.n > kMdLds ? kMdLds : w.n;
		}
		if constexpr (kMdMode != 2 && !kRg) *q++ = '\n';
	} else q = put_lit(q, SAM_UNMAPPED_TAIL, (int)(sizeof(SAM_UNMAPPED_TAIL) - 1) - (kRg ? 1 : 0));
	nT = (int)(q - T);
}

// (one lane) "\tMD:Z:", the string and (kLf) the line feed of a mapped record at p, of which `room` bytes belong to the read's lines; returns their true number --
// where that exceeds the room nothing is written past it, and the caller's count of the line's bytes shows the disagreement
template <bool kLf>
__device__ __forceinline__ int print_md_tail(const MdRef &R, const kg_aln_record &rec, const uint8_t *seq, int rlen, uint8_t *p, int64_t room)
{
	const int cap = room > 0x7FFFFFFFll ? 0x7FFFFFFF : room < 0 ? 0 : (int)room;
	if (cap >= 6) put_lit(reinterpret_cast<char *>(p), "\tMD:Z:", 6);
	MdWrite w(reinterpret_cast<char *>(p) + 6, cap >= 6 ? cap - 6 : 0);
	md_walk(R, rec, seq, rlen, w);
	if constexpr (kLf) {
		if (6 + w.n < cap) p[6 + w.n] = '\n';
	}
	return 6 + w.n + (kLf ? 1 : 0);
}

// all lanes: one line from its pieces; returns the end
__device__ __forceinline__ uint8_t *copy_line(uint8_t *__restrict__ p, int lane, const uint8_t *__restrict__ name, int name_len, const char *A, int nA,
                                              const uint8_t *__restrict__ chr, int n_chr, const char *B, int nB, const uint8_t *__restrict__ seq, int rlen, bool flip,
                                              const uint8_t *__restrict__ qual, int qlen, bool qrev, const char *T, int nT)
{
	// (every piece is at most a few wave-widths long: the loads of all pieces are issued before the first store is needed)
	for (int k = lane; k < name_len; k += 64) p[k] = name[k];
	p += name_len;
	if (lane < nA) p[lane] = (uint8_t)A[lane];
	p += nA;
	for (int k = lane; k < n_chr; k += 64) p[k] = chr[k];
	p += n_chr;
	for (int k = lane; k < nB; k += 64) p[k] = (uint8_t)B[k];
	p += nB;
	// the read as the record shows it: as held, or its reverse complement (GetComplementarySeq) with the qualities reversed
	if (flip) { for (int k = lane; k < rlen; k += 64) p[k] = comp_char(seq[rlen - 1 - k]); }
	else { for (int k = lane; k < rlen; k += 64) p[k] = seq[k]; }
	p += rlen;
	if (lane == 0) *p = '\t';
	p += 1;
	if (qrev) { for (int k = lane; k < qlen; k += 64) p[k] = qual[qlen - 1 - k]; }
	else { for (int k = lane; k < qlen; k += 64) p[k] = qual[k]; }
	p += qlen;
	if (lane < nT) p[lane] = (uint8_t)T[lane];
	return p + nT;
}

}  // namespace

template <bool kMd, bool kRg>
__global__ __launch_bounds__(64) void sam_format_kernel(SamArgs a, MdArg<kMd> md)
{
	constexpr int kFmtSlot = kMd ? kFmtSlotMd : kg::kFmtSlot;
	__shared__ __attribute__((aligned(16))) char str[64 * kFmtSlot];
	__shared__ FmtDesc desc[64];
	__shared__ int chain_len[kMd ? 4 : 3];      // [3]: the bytes print_md_tail made
	__shared__ int chunk_pre[65];          // phase 2b: chunks of the lines before line i
	const int lane = threadIdx.x;
	const int64_t n_groups = (a.n_reads + 63) >> 6;
	for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
		// ---- phase 1: lane = read -------------------------------------------------------------------------------------------
		{
			const int64_t r = (g << 6) + lane;
			FmtDesc d;
			d.flags = 0;
			if (r < a.n_reads) {
				const kg_aln_record &rec = a.records[r];
				const int kind = rec.kind;
				if (kind == KG_ALN_UNMAPPED || kind == KG_ALN_MAPPED || (kind != KG_ALN_HOST && rec.next >= 0)) {
					const ReadText t = read_text(a, r);
					const int64_t o0 = a.sam_off[r], o1 = a.sam_off[r + 1];
					d.name = t.name; d.qual = t.qual; d.seq = a.enc + a.read_off[r];
					d.out = a.sam + o0;
					d.room_end_lo = (int32_t)(o1 - o0);
					d.name_len = (int16_t)t.name_len; d.rlen = (int16_t)t.rlen; d.qlen = (int16_t)t.qlen;
					d.chr = a.chr_names; d.n_chr = 0;
					const bool mapped = kind == KG_ALN_MAPPED;
					if (mapped) { d.chr = a.chr_names + a.chr_name_off[rec.chr]; d.n_chr = (int16_t)(a.chr_name_off[rec.chr + 1] - a.chr_name_off[rec.chr]); }
					const bool flip = mapped && rec.flip;
					int nA = 0, nB = 0, nT = 0;
					// (reads beyond what the 16-bit fields and the output buffer hold take the record-by-record path, which checks)
					const bool wide = t.rlen > 32000 || t.name_len > 32000 || o1 > a.sam_capacity;
					bool chained = rec.next >= 0 || wide || (kind != KG_ALN_UNMAPPED && kind != KG_ALN_MAPPED);
					if constexpr (kMd) {
						// (an MD beyond the slot: the record-by-record path as well)
						bool over = false;
						if (!chained) print_fields<1, kRg>(t, rec, str + lane * kFmtSlot, str + lane * kFmtSlot + kFmtA, str + lane * kFmtSlot + kFmtA + kFmtB, nA, nB, nT, &md.r, d.seq, &over);
						chained = chained || over;
					} else
					if (!chained) print_fields<0, kRg>(t, rec, str + lane * kFmtSlot, str + lane * kFmtSlot + kFmtA, str + lane * kFmtSlot + kFmtA + kFmtB, nA, nB, nT);
					d.nA = (uint8_t)nA; d.nB = (uint8_t)nB; d.nT = (uint8_t)nT;
					d.flags = (uint8_t)(1 | (flip ? 2 : 0) | (flip != t.held_reversed ? 4 : 0) | (chained ? 8 : 0));
				}
			}
			desc[lane] = d;
		}
		__syncthreads();
		// ---- phase 2: every lane its own line (the strings it printed in phase 1 lie in its LDS slot) ------------------------------
		{
			const FmtDesc d = desc[lane];
			if ((d.flags & 1) && !(d.flags & 8)) {
				const uint8_t *S = reinterpret_cast<const uint8_t *>(str) + lane * kFmtSlot;
				uint8_t *p = d.out;
				const uint8_t *const end = d.out + d.room_end_lo;
				uint8_t *const bases = d.out + d.name_len + d.nA + d.n_chr + d.nB;      // (from here on other lanes write, phase 2b: no surplus past it)
				p = lane_copy(p, bases, d.name, d.name_len);
				p = lane_copy(p, bases, S, d.nA);
				p = lane_copy(p, bases, d.chr, d.n_chr);
				p = lane_copy(p, bases, S + kFmtA, d.nB);
				p += d.rlen;
				*p++ = '\t';
				p += d.qlen;
				p = lane_copy(p, end, S + kFmtA + kFmtB, d.nT);
				if constexpr (kRg) {
					// (every lane reads the same bytes of the stream's buffer: one fetch per instruction)
					p = lane_copy(p, end, a.rg, a.rg_len);
					*p++ = '\n';
				}
				if (p != end) atomicAdd(&a.ctl[1], 1ull);
			}
		}
		// ---- phase 2b: the bases and the qualities of the 64 lines as ONE list of 16-byte chunks (a line's bases first, then its qualities; 20 chunks for a
		//      150-base read), lane l taking chunks l, l + 64, ...: consecutive lanes move consecutive chunks of a line -- whole 128-byte lines of memory per
		//      instruction on either side, every lane busy in every step.  The read as the record shows it: as held, or its reverse complement
		//      (GetComplementarySeq) with the qualities reversed.  (A line per lane moved the same bytes with the same number of instructions but touched
		//      64 different memory lines per instruction; eight or sixteen lanes per line left lanes idle: 83 ms against 77 per 100 M reads.)
		{
			const FmtDesc &dm = desc[lane];
			const bool on = (dm.flags & 1) && !(dm.flags & 8);
			const int mine = on ? ((dm.rlen + 15) >> 4) + ((dm.qlen + 15) >> 4) : 0;
			const int incl = wave_inclusive_scan(mine);
			if (lane == 0) chunk_pre[0] = 0;
			chunk_pre[lane + 1] = incl;
		}
		__syncthreads();
		{
			const int total = chunk_pre[64];
			int line = 0;
			for (int idx = lane; idx < total; idx += 64) {
				while (idx >= chunk_pre[line + 1]) ++line;
				const FmtDesc &d = desc[line];
				const int c = idx - chunk_pre[line];
				const int n_seq = (d.rlen + 15) >> 4;
				const bool is_seq = c < n_seq;
				const int off = (is_seq ? c : c - n_seq) << 4, n = is_seq ? d.rlen : d.qlen;
				const uint8_t *src = is_seq ? d.seq : d.qual;
				uint8_t *dst = d.out + d.name_len + d.nA + d.n_chr + d.nB + (is_seq ? 0 : d.rlen + 1) + off;
				const bool rev = is_seq ? (d.flags & 2) != 0 : (d.flags & 4) != 0;
				if (off + 16 <= n) {
					SamU128 v = *reinterpret_cast<const SamU128 *>(rev ? src + n - 16 - off : src + off);
					if (rev) {
						const uint64_t lo = __builtin_bswap64(v.hi), hi = __builtin_bswap64(v.lo);
						v.lo = lo; v.hi = hi;
						if (is_seq) { v.lo = comp8(v.lo); v.hi = comp8(v.hi); }
					}
					*reinterpret_cast<SamU128 *>(dst) = v;
				} else {
					for (int k = off; k < n; ++k) {
						const uint8_t b = rev ? src[n - 1 - k] : src[k];
						dst[k - off] = rev && is_seq ? comp_char(b) : b;
					}
				}
			}
		}
		__syncthreads();
		// ... and, all lanes per read, the rare ones with chained records (-m) or beyond the 16-bit fields
		for (int i = 0; i < 64;) {
			if (!(desc[i].flags & 1) || !(desc[i].flags & 8)) { ++i; continue; }
			// -m: every record chained behind the read's own, one after the other (lane 0 prints the fields of each)
			const int64_t r = (g << 6) + i;
			const ReadText t = read_text(a, r);
			const uint8_t *const seq = a.enc + a.read_off[r];
			uint8_t *p = a.sam + a.sam_off[r];
			const int64_t room = a.sam_off[r + 1];
			if (room > a.sam_capacity) { if (lane == 0) atomicAdd(&a.ctl[1], 1ull); ++i; continue; }
			char *S = str + i * kFmtSlot;                    // (the read's own slot is free: nothing was printed into it)
			for (int64_t at = r; at >= 0; at = a.records[at].next) {
				const kg_aln_record &rec = a.records[at];
				if (rec.kind != KG_ALN_UNMAPPED && rec.kind != KG_ALN_MAPPED) continue;
				const bool mapped = rec.kind == KG_ALN_MAPPED;
				__syncthreads();
				if (lane == 0) print_fields<kMd ? 2 : 0, kRg>(t, rec, S, S + kFmtA, S + kFmtA + kFmtB, chain_len[0], chain_len[1], chain_len[2]);
				__syncthreads();
				const uint8_t *cn = a.chr_names;
				int nc = 0;
				if (mapped) { cn = a.chr_names + a.chr_name_off[rec.chr]; nc = a.chr_name_off[rec.chr + 1] - a.chr_name_off[rec.chr]; }
				const bool flip = mapped && rec.flip;
				p = copy_line(p, lane, t.name, t.name_len, S, chain_len[0], cn, nc, S + kFmtA, chain_len[1], seq, t.rlen, flip, t.qual, t.qlen, flip != t.held_reversed,
				              S + kFmtA + kFmtB, chain_len[2]);
				if constexpr (kMd) {
					if (mapped) {
						if (lane == 0) chain_len[3] = print_md_tail<!kRg>(md.r, rec, seq, t.rlen, p, room - (int64_t)(p - a.sam));
						__syncthreads();
						p += chain_len[3];
						if ((int64_t)(p - a.sam) > room) break;      // (the size kernel counted another string: the check below reports it, nothing more is written)
					}
				}
				if constexpr (kRg) {
					// the read group and the line feed behind the record's last field, unmapped records too
					if ((int64_t)(p - a.sam) + a.rg_len + 1 > room) { p += a.rg_len + 1; break; }      // (as above)
					for (int k = lane; k < a.rg_len; k += 64) p[k] = a.rg[k];
					if (lane == 0) p[a.rg_len] = '\n';
					p += a.rg_len + 1;
				}
			}
			if (lane == 0 && (int64_t)(p - a.sam) != room) atomicAdd(&a.ctl[1], 1ull);
			++i;
		}
		__syncthreads();
	}
}

// ---- BAM records -----------------------------------------------------------------------------------------------------------------
// The same records as BAM (SAM/BAM specification v1, section 4.2) instead of text: for every read the device decides, its records in print
// order, each behind its block_size, byte for byte what the host's encoder (host/detail/bam.inc, bam_from_sam_line) makes of the line
// sam_format_kernel prints for the record -- that encoder parses the printed line, so its view of the line is the contract:
//   l_read_name is a byte, FLAG / n_cigar_op 16 bits, POS / PNEXT / TLEN 32 bits (each cut to its width);
//   a one-character read "*" shown as held is "no sequence" (l_seq 0);
//   the qualities are l_seq bytes of 0xFF unless the column holds exactly l_seq characters -- fewer, a lone "*", or a tab among them
//   (the column ends there) all give 0xFF; NM / AS / XS in the smallest integer type that holds the value;
//   a quality line shorter than its read brings its line feed along as its last quality (GetNextEntry cuts the line to the read's length, not at
//   the line feed): the printed line breaks there, the record ends with its 0xFF qualities, and the tags -- a piece of text that is no record -- go.
namespace {

constexpr int kBamCore = 36;                                     // block_size + the 32 fixed bytes
constexpr int kBamH = 48, kBamC = 96, kBamT = 32, kBamSlot = kBamH + kBamC + kBamT;     // a lane's core, CIGAR words (KG_ALN_CIGAR_MAX / 2 ops at most) and tags
static_assert(KG_ALN_CIGAR_MAX / 2 * 4 <= kBamC, "the CIGAR words of a record must fit the lane's slot");
// with MD:Z: the three integer tags (7 bytes each at most), 'M' 'D' 'Z', kMdLds characters and the NUL
constexpr int kBamTMd = 96, kBamSlotMd = kBamH + kBamC + kBamTMd;
static_assert(21 + 3 + kMdLds + 1 <= kBamTMd && kBamTMd % 16 == 0, "the tags with MD must fit the lane's slot");

struct BamDesc {                       // what phase 2 needs for one read
	const uint8_t *name, *qual, *seq;
	uint8_t *out;
	int32_t room;
	int16_t name_len, lseq;
	uint8_t nC, nT, flags, pad;        // flags: 1 print, 2 reverse-complement, 4 qualities reversed, 8 record-by-record path, 16 qualities are 0xFF
};

__device__ __forceinline__ int bam_tag_bytes(int v)
{
	return 3 + (v < 0 ? (v >= -128 ? 1 : v >= -32768 ? 2 : 4) : (v < 256 ? 1 : v < 65536 ? 2 : 4));
}

__device__ __forceinline__ uint8_t *bam_put_tag(uint8_t *q, char c0, char c1, int v)
{
	const int n = bam_tag_bytes(v) - 3;
	q[0] = (uint8_t)c0; q[1] = (uint8_t)c1;
	q[2] = (uint8_t)(v < 0 ? (n == 1 ? 'c' : n == 2 ? 's' : 'i') : (n == 1 ? 'C' : n == 2 ? 'S' : 'I'));
	for (int i = 0; i < n; ++i) q[3 + i] = (uint8_t)((uint32_t)v >> (8 * i));
	return q + 3 + n;
}

__device__ __forceinline__ int bam_cigar_op(char ch)              // index in "MIDNSHP=X", or -1
{
	return ch == 'M' ? 0 : ch == 'I' ? 1 : ch == 'D' ? 2 : ch == 'N' ? 3 : ch == 'S' ? 4 : ch == 'H' ? 5 : ch == 'P' ? 6 : ch == '=' ? 7 : ch == 'X' ? 8 : -1;
}

// the SEQ column of a record: "*" alone means no sequence (a read held as "*" and shown as held; its complement is 'N')
__device__ __forceinline__ int bam_lseq(const SamArgs &a, int64_t r, int rlen, const kg_aln_record &rec)
{
	const bool flip = rec.kind == KG_ALN_MAPPED && rec.flip;
	return rlen == 1 && !flip && a.enc[a.read_off[r]] == '*' ? 0 : rlen;
}

// the read's qualities end in their line's line feed
__device__ __forceinline__ bool bam_qual_breaks(const ReadText &t) { return t.qlen > 0 && t.qual[t.qlen - 1] == '\n'; }

__device__ __forceinline__ int bam_block_bytes(int name_len, int lseq) { return kBamCore + name_len + 1 + ((lseq + 1) >> 1) + lseq; }

__device__ __forceinline__ int bam_cigar_ops(const kg_aln_record &rec)
{
	int ops = 0;
	for (int i = 0; i < rec.cigar_len; ++i) ops += bam_cigar_op(rec.cigar[i]) >= 0 ? 1 : 0;
	return ops > kBamC / 4 ? kBamC / 4 : ops;       // (a number in front of every operation: never more)
}

// rg: the bytes of the read group field ('R' 'G' 'Z' <ID> NUL) behind the tags of a record that has its tags, 0 = none
template <bool kMd>
__device__ int bam_record_size(const ReadText &t, const kg_aln_record &rec, int lseq, const uint8_t *seq, const MdArg<kMd> &md, int rg)
{
	if (rec.kind != KG_ALN_UNMAPPED && rec.kind != KG_ALN_MAPPED) return 0;
	if (bam_qual_breaks(t)) return bam_block_bytes(t.name_len, lseq) + (rec.kind == KG_ALN_MAPPED ? 4 * bam_cigar_ops(rec) : 0);
	if (rec.kind == KG_ALN_UNMAPPED) return bam_block_bytes(t.name_len, lseq) + 8 + rg;
	int n = bam_block_bytes(t.name_len, lseq) + 4 * bam_cigar_ops(rec) + bam_tag_bytes(t.rlen - rec.score) + bam_tag_bytes(rec.score) + bam_tag_bytes(rec.sub_score);
	if constexpr (kMd) {
		MdCount c;
		md_walk(md.r, rec, seq, t.rlen, c);
		n += 3 + c.n + 1;
	}
	return n + rg;
}

__device__ __forceinline__ int bam_reg2bin(int64_t beg, int64_t end)      // SAMv1 5.3
{
	--end;
	if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

// one record's core (H: nine words), CIGAR words (C) and tags (T); nC / nT in bytes
// kMdMode 0: no MD:Z (the code as it was).  1: a mapped record's MD behind XS, in T -- md_n > kMdLds: it has that many characters and T is not whole.
// 2: T ends behind XS and block_size counts the 3 + md_n + 1 bytes of MD behind it, which the caller writes itself (bam_md_tail); md_n < 0: the record has none
// rg: block_size counts that many bytes of a read group field behind the tags (and MD), which the caller copies there -- unless the record has no tags (nT == 0)
template <int kMdMode>
__device__ __forceinline__ void bam_build(const ReadText &t, const kg_aln_record &rec, int lseq, uint32_t *H, uint32_t *C, uint8_t *T, int &nC, int &nT, int rg, const MdRef *R = nullptr,
                                          const uint8_t *seq = nullptr, int *md_n = nullptr)
{
	const bool mapped = rec.kind == KG_ALN_MAPPED;
	int ops = 0;
	int64_t ref_len = 0;
	uint8_t *q = T;
	if (mapped) {
		uint32_t num = 0;
		for (int i = 0; i < rec.cigar_len; ++i) {
			const char ch = rec.cigar[i];
			if (ch >= '0' && ch <= '9') { num = num * 10u + (uint32_t)(ch - '0'); continue; }
			const int op = bam_cigar_op(ch);
			if (op >= 0 && ops < kBamC / 4) {
				C[ops++] = num << 4 | (uint32_t)op;
				if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += num;
			}
			num = 0;
		}
		q = bam_put_tag(q, 'N', 'M', t.rlen - rec.score);
		q = bam_put_tag(q, 'A', 'S', rec.score);
		q = bam_put_tag(q, 'X', 'S', rec.sub_score);
	} else {
		q = bam_put_tag(q, 'A', 'S', 0);
		q = bam_put_tag(q, 'X', 'S', 0);
	}
	int md_tail = 0;                          // bytes of MD behind T
	if constexpr (kMdMode != 0) {
		*md_n = -1;
		if (mapped && !bam_qual_breaks(t)) {
			if constexpr (kMdMode == 1) {
				q[0] = 'M'; q[1] = 'D'; q[2] = 'Z';
				MdWrite w(reinterpret_cast<char *>(q) + 3, kMdLds);
				md_walk(*R, rec, seq, t.rlen, w);
				*md_n = w.n;
				q += 3 + (w.n > kMdLds ? kMdLds : w.n);
				*q++ = 0;
			} else {
				MdCount c;
				md_walk(*R, rec, seq, t.rlen, c);
				*md_n = c.n;
				md_tail = 3 + c.n + 1;
			}
		}
	}
	nC = 4 * ops;
	nT = bam_qual_breaks(t) ? 0 : (int)(q - T);
	const int64_t pos = mapped ? rec.pos - 1 : -1;
	const int bin = bam_reg2bin(pos, pos + (ref_len > 0 ? ref_len : 1));
	const bool mate = mapped && rec.has_mate;
	H[0] = (uint32_t)(bam_block_bytes(t.name_len, lseq) + nC + nT + md_tail + (nT ? rg : 0) - 4);
	H[1] = mapped ? (uint32_t)rec.chr : 0xFFFFFFFFu;
	H[2] = (uint32_t)pos;
	H[3] = (uint32_t)((t.name_len + 1) & 255) | (uint32_t)((mapped ? rec.mapq : 0) & 255) << 8 | (uint32_t)(bin & 0xFFFF) << 16;
	H[4] = (uint32_t)(ops & 0xFFFF) | (uint32_t)(rec.flag & 0xFFFF) << 16;
	H[5] = (uint32_t)lseq;
	H[6] = mate ? (uint32_t)rec.chr : 0xFFFFFFFFu;
	H[7] = mate ? (uint32_t)(rec.mate_pos - 1) : 0xFFFFFFFFu;
	H[8] = mate ? (uint32_t)rec.tlen : 0u;
}

// the 4-bit code of a base: its place in "=ACMGRSVTWYHKDBN", either case; anything else 15 (codes of 'A' .. 'P' and 'Q' .. 'Z', a nibble each)
__device__ __forceinline__ uint32_t bam_code4(uint32_t c)
{
	const uint32_t i = (c & 0xDFu) - 0x41u;
	if (i < 16u) return (uint32_t)(0xFFF3FCFFB4FFD2E1ull >> (4u * i)) & 15u;
	if (i < 26u) return (uint32_t)(0xFAF97F865Full >> (4u * (i - 16u))) & 15u;
	return c == '=' ? 0u : 15u;
}

// eight bases (lowest address first) -> four bytes, the first base of each pair in the high nibble
__device__ __forceinline__ uint32_t bam_pack8(uint64_t x)
{
	uint32_t o = 0;
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const uint32_t hi = bam_code4((uint32_t)(x >> (16 * j)) & 255u), lo = bam_code4((uint32_t)(x >> (16 * j + 8)) & 255u);
		o |= (hi << 4 | lo) << (8 * j);
	}
	return o;
}

// q - 33 in each of eight bytes, every byte on its own: no borrow from a byte below '!' into its neighbour
__device__ __forceinline__ uint64_t bam_qual8(uint64_t x)
{
	const uint64_t H = 0x8080808080808080ull;
	return ((x | H) - 0x2121212121212121ull) ^ (~x & H);
}

__device__ __forceinline__ bool has_tab8(uint64_t x)
{
	const uint64_t t = x ^ 0x0909090909090909ull;
	return ((t - 0x0101010101010101ull) & ~t & 0x8080808080808080ull) != 0;
}

// base i of the read as the record shows it
__device__ __forceinline__ uint32_t bam_shown(const uint8_t *seq, int lseq, bool flip, int i)
{
	return flip ? comp_char(seq[lseq - 1 - i]) : seq[i];
}

// all lanes: one record from its pieces (core, CIGAR words and tags in the LDS); returns the end
__device__ __forceinline__ uint8_t *bam_copy_record(uint8_t *__restrict__ p, int lane, const uint8_t *H, const uint8_t *__restrict__ name, int name_len, const uint8_t *C, int nC,
                                                    const uint8_t *__restrict__ seq, int lseq, bool flip, const uint8_t *__restrict__ qual, int qlen, bool qrev, const uint8_t *T, int nT)
{
	if (lane < kBamCore) p[lane] = H[lane];
	p += kBamCore;
	for (int k = lane; k < name_len; k += 64) p[k] = name[k];
	p += name_len;
	if (lane == 0) *p = 0;
	p += 1;
	for (int k = lane; k < nC; k += 64) p[k] = C[k];
	p += nC;
	const int nb = (lseq + 1) >> 1;
	for (int k = lane; k < nb; k += 64) {
		const uint32_t hi = bam_code4(bam_shown(seq, lseq, flip, 2 * k)), lo = 2 * k + 1 < lseq ? bam_code4(bam_shown(seq, lseq, flip, 2 * k + 1)) : 0u;
		p[k] = (uint8_t)(hi << 4 | lo);
	}
	p += nb;
	bool fill = qlen != lseq || (lseq == 1 && qual[0] == '*') || (qlen > 0 && qual[qlen - 1] == '\n');
	if (!fill) {
		bool tab = false;
		for (int k = lane; k < qlen; k += 64) tab = tab || qual[k] == '\t';
		fill = __any(tab ? 1 : 0) != 0;
	}
	for (int k = lane; k < lseq; k += 64) p[k] = fill ? (uint8_t)0xFF : (uint8_t)((qrev ? qual[lseq - 1 - k] : qual[k]) - 33);
	p += lseq;
	if (lane < nT) p[lane] = T[lane];
	return p + nT;
}

// (one lane) 'M' 'D' 'Z', the md_n characters and the NUL of a mapped record at p, of which `room` bytes belong to the read's records; nothing is written past
// the room (the caller's count of the record's bytes shows a disagreement)
__device__ __forceinline__ void bam_md_tail(const MdRef &R, const kg_aln_record &rec, const uint8_t *seq, int rlen, uint8_t *p, int64_t room, int md_n)
{
	if (room < 3 + (int64_t)md_n + 1) return;
	p[0] = 'M'; p[1] = 'D'; p[2] = 'Z';
	MdWrite w(reinterpret_cast<char *>(p) + 3, md_n);
	md_walk(R, rec, seq, rlen, w);
	p[3 + md_n] = 0;
}

}  // namespace

template <bool kMd, bool kRg>
__global__ __launch_bounds__(256) void bam_size_kernel(SamArgs a, MdArg<kMd> md)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const kg_aln_record &first = a.records[r];
		int n = 0;
		if (first.kind == KG_ALN_HOST) {
			a.host_list[atomicAdd(&a.ctl[0], 1ull)] = (int32_t)r;
		} else {
			const ReadText t = read_text(a, r);
			for (int64_t at = r; at >= 0; at = a.records[at].next) n += bam_record_size<kMd>(t, a.records[at], bam_lseq(a, r, t.rlen, a.records[at]), a.enc + a.read_off[r], md, rg_bytes<kRg>(a));
		}
		a.sam_len[r] = n;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) a.sam_len[a.n_reads] = 0;
}

// One wave per 64 consecutive reads, the two phases of sam_format_kernel:
//   1. lane l builds the core, the CIGAR words and the tags of read base + l in its own slot of the wave's LDS block;
//   2. every lane copies its own record's core, name, CIGAR words and tags; then the packed bases and the qualities of the 64 records go
//      as ONE list of 16-byte chunks, lane l taking chunks l, l + 64, ...: a chunk of packed bases is made of 32 bases (two loads), the
//      reversed form reads them from the read's other end and complements them; a chunk of qualities is 16 of them less 33.
// A read with further records chained behind it (-m), or beyond the 16-bit descriptor fields, takes the record-by-record path.
template <bool kMd, bool kRg>
__global__ __launch_bounds__(64) void bam_format_kernel(SamArgs a, MdArg<kMd> md)
{
	constexpr int kBamSlot = kMd ? kBamSlotMd : kg::kBamSlot;
	__shared__ __attribute__((aligned(16))) uint8_t str[64 * kBamSlot];
	__shared__ BamDesc desc[64];
	__shared__ int chain_len[kMd ? 3 : 2];      // [2]: the characters of the record's MD, or -1
	__shared__ int chunk_pre[65];
	__shared__ int tab_seen[65];           // [64]: some line of the group; [i]: line i -- a tab among its qualities (the column ends there: 0xFF)
	const int lane = threadIdx.x;
	const int64_t n_groups = (a.n_reads + 63) >> 6;
	for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
		// ---- phase 1: lane = read -------------------------------------------------------------------------------------------
		{
			const int64_t r = (g << 6) + lane;
			BamDesc d;
			d.flags = 0; d.lseq = 0; d.name_len = 0; d.nC = 0; d.nT = 0;
			tab_seen[lane] = 0;
			if (lane == 0) tab_seen[64] = 0;
			if (r < a.n_reads) {
				const kg_aln_record &rec = a.records[r];
				const int kind = rec.kind;
				if (kind == KG_ALN_UNMAPPED || kind == KG_ALN_MAPPED || (kind != KG_ALN_HOST && rec.next >= 0)) {
					const ReadText t = read_text(a, r);
					const int64_t o0 = a.sam_off[r], o1 = a.sam_off[r + 1];
					const int lseq = bam_lseq(a, r, t.rlen, rec);
					d.name = t.name; d.qual = t.qual; d.seq = a.enc + a.read_off[r];
					d.out = a.sam + o0;
					d.room = (int32_t)(o1 - o0);
					d.name_len = (int16_t)t.name_len; d.lseq = (int16_t)lseq;
					const bool flip = kind == KG_ALN_MAPPED && rec.flip;
					int nC = 0, nT = 0;
					const bool wide = t.rlen > 32000 || t.name_len > 32000 || o1 > a.sam_capacity;
					bool chained = rec.next >= 0 || wide || (kind != KG_ALN_UNMAPPED && kind != KG_ALN_MAPPED);
					uint8_t *S = str + lane * kBamSlot;
					if constexpr (kMd) {
						// (an MD beyond the slot: the record-by-record path as well)
						int md_n = -1;
						if (!chained) bam_build<1>(t, rec, lseq, reinterpret_cast<uint32_t *>(S), reinterpret_cast<uint32_t *>(S + kBamH), S + kBamH + kBamC, nC, nT, rg_bytes<kRg>(a), &md.r, d.seq, &md_n);
						chained = chained || md_n > kMdLds;
					} else
					if (!chained) bam_build<0>(t, rec, lseq, reinterpret_cast<uint32_t *>(S), reinterpret_cast<uint32_t *>(S + kBamH), S + kBamH + kBamC, nC, nT, rg_bytes<kRg>(a));
					d.nC = (uint8_t)nC; d.nT = (uint8_t)nT;
					const bool qfill = t.qlen != lseq || (lseq == 1 && t.qual[0] == '*') || bam_qual_breaks(t);
					d.flags = (uint8_t)(1 | (flip ? 2 : 0) | (flip != t.held_reversed ? 4 : 0) | (chained ? 8 : 0) | (qfill ? 16 : 0));
				}
			}
			desc[lane] = d;
		}
		__syncthreads();
		// ---- phase 2: every lane its own record's short pieces (built in phase 1 in its LDS slot) --------------------------------------
		{
			const BamDesc d = desc[lane];
			if ((d.flags & 1) && !(d.flags & 8)) {
				const uint8_t *S = str + lane * kBamSlot;
				uint8_t *p = d.out;
				const uint8_t *const end = d.out + d.room;
				uint8_t *const bases = d.out + kBamCore + d.name_len + 1 + d.nC;       // (from here on other lanes write, phase 2b: no surplus past it)
				p = lane_copy(p, bases, S, kBamCore);
				p = lane_copy(p, bases, d.name, d.name_len);
				*p++ = 0;
				p = lane_copy(p, bases, S + kBamH, d.nC);
				p += ((d.lseq + 1) >> 1) + d.lseq;
				p = lane_copy(p, end, S + kBamH + kBamC, d.nT);
				if constexpr (kRg) {
					// (a record without tags -- its quality line broke the printed line -- has no read group either)
					if (d.nT) p = lane_copy(p, end, a.rg, a.rg_len);
				}
				if (p != end) atomicAdd(&a.ctl[1], 1ull);
			}
		}
		// ---- phase 2b: the packed bases and the qualities of the 64 records as one list of 16-byte chunks --------------------------------
		{
			const BamDesc &dm = desc[lane];
			const bool on = (dm.flags & 1) && !(dm.flags & 8);
			const int mine = on ? ((((dm.lseq + 1) >> 1) + 15) >> 4) + ((dm.lseq + 15) >> 4) : 0;
			const int incl = wave_inclusive_scan(mine);
			if (lane == 0) chunk_pre[0] = 0;
			chunk_pre[lane + 1] = incl;
		}
		__syncthreads();
		{
			const int total = chunk_pre[64];
			int line = 0;
			for (int idx = lane; idx < total; idx += 64) {
				while (idx >= chunk_pre[line + 1]) ++line;
				const BamDesc &d = desc[line];
				const int c = idx - chunk_pre[line];
				const int lseq = d.lseq, nb = (lseq + 1) >> 1;
				const int n_seq = (nb + 15) >> 4;
				uint8_t *const base = d.out + kBamCore + d.name_len + 1 + d.nC;
				if (c < n_seq) {
					const bool flip = (d.flags & 2) != 0;
					uint8_t *dst = base + (c << 4);
					const int b0 = c << 5;                                   // first base of the chunk
					if (b0 + 32 <= lseq) {
						uint64_t w0, w1, w2, w3;
						if (flip) {
							const SamU128 lo = *reinterpret_cast<const SamU128 *>(d.seq + lseq - 32 - b0), hi = *reinterpret_cast<const SamU128 *>(d.seq + lseq - 16 - b0);
							w0 = comp8(__builtin_bswap64(hi.hi)); w1 = comp8(__builtin_bswap64(hi.lo));
							w2 = comp8(__builtin_bswap64(lo.hi)); w3 = comp8(__builtin_bswap64(lo.lo));
						} else {
							const SamU128 lo = *reinterpret_cast<const SamU128 *>(d.seq + b0), hi = *reinterpret_cast<const SamU128 *>(d.seq + b0 + 16);
							w0 = lo.lo; w1 = lo.hi; w2 = hi.lo; w3 = hi.hi;
						}
						SamU128 o;
						o.lo = (uint64_t)bam_pack8(w0) | (uint64_t)bam_pack8(w1) << 32;
						o.hi = (uint64_t)bam_pack8(w2) | (uint64_t)bam_pack8(w3) << 32;
						*reinterpret_cast<SamU128 *>(dst) = o;
					} else {
						for (int k = c << 4; k < nb; ++k) {
							const uint32_t hi = bam_code4(bam_shown(d.seq, lseq, flip, 2 * k)), lo = 2 * k + 1 < lseq ? bam_code4(bam_shown(d.seq, lseq, flip, 2 * k + 1)) : 0u;
							base[k] = (uint8_t)(hi << 4 | lo);
						}
					}
				} else {
					const int off = (c - n_seq) << 4;
					uint8_t *dst = base + nb + off;
					const bool rev = (d.flags & 4) != 0, fill = (d.flags & 16) != 0;
					if (off + 16 <= lseq) {
						SamU128 v;
						v.lo = v.hi = ~0ull;
						if (!fill) {
							v = *reinterpret_cast<const SamU128 *>(rev ? d.qual + lseq - 16 - off : d.qual + off);
							if (has_tab8(v.lo) || has_tab8(v.hi)) { tab_seen[line] = 1; tab_seen[64] = 1; }
							if (rev) { const uint64_t lo = __builtin_bswap64(v.hi), hi = __builtin_bswap64(v.lo); v.lo = lo; v.hi = hi; }
							v.lo = bam_qual8(v.lo); v.hi = bam_qual8(v.hi);
						}
						*reinterpret_cast<SamU128 *>(dst) = v;
					} else {
						for (int k = off; k < lseq; ++k) {
							const uint8_t b = fill ? (uint8_t)0 : rev ? d.qual[lseq - 1 - k] : d.qual[k];
							if (!fill && b == '\t') { tab_seen[line] = 1; tab_seen[64] = 1; }
							dst[k - off] = fill ? (uint8_t)0xFF : (uint8_t)(b - 33);
						}
					}
				}
			}
		}
		__syncthreads();
		// ... a tab among a record's qualities: the column the host's encoder sees is shorter than the read
		if (tab_seen[64]) {
			for (int i = 0; i < 64; ++i) {
				if (!tab_seen[i]) continue;
				const BamDesc &d = desc[i];
				uint8_t *q = d.out + kBamCore + d.name_len + 1 + d.nC + ((d.lseq + 1) >> 1);
				for (int k = lane; k < d.lseq; k += 64) q[k] = 0xFF;
			}
		}
		// ... and, all lanes per read, the rare ones with chained records (-m) or beyond the 16-bit fields
		for (int i = 0; i < 64; ++i) {
			if (!(desc[i].flags & 1) || !(desc[i].flags & 8)) continue;
			const int64_t r = (g << 6) + i;
			const ReadText t = read_text(a, r);
			const uint8_t *const seq = a.enc + a.read_off[r];
			uint8_t *p = a.sam + a.sam_off[r];
			const int64_t room = a.sam_off[r + 1];
			if (room > a.sam_capacity) { if (lane == 0) atomicAdd(&a.ctl[1], 1ull); continue; }
			uint8_t *S = str + i * kBamSlot;                 // (the read's own slot is free: nothing was built in it)
			for (int64_t at = r; at >= 0; at = a.records[at].next) {
				const kg_aln_record &rec = a.records[at];
				if (rec.kind != KG_ALN_UNMAPPED && rec.kind != KG_ALN_MAPPED) continue;
				const int lseq = bam_lseq(a, r, t.rlen, rec);
				__syncthreads();
				if constexpr (kMd) {
					if (lane == 0) bam_build<2>(t, rec, lseq, reinterpret_cast<uint32_t *>(S), reinterpret_cast<uint32_t *>(S + kBamH), S + kBamH + kBamC, chain_len[0], chain_len[1], rg_bytes<kRg>(a), &md.r, seq, &chain_len[2]);
				} else
				if (lane == 0) bam_build<0>(t, rec, lseq, reinterpret_cast<uint32_t *>(S), reinterpret_cast<uint32_t *>(S + kBamH), S + kBamH + kBamC, chain_len[0], chain_len[1], rg_bytes<kRg>(a));
				__syncthreads();
				const bool flip = rec.kind == KG_ALN_MAPPED && rec.flip;
				p = bam_copy_record(p, lane, S, t.name, t.name_len, S + kBamH, chain_len[0], seq, lseq, flip, t.qual, t.qlen, flip != t.held_reversed, S + kBamH + kBamC, chain_len[1]);
				if constexpr (kMd) {
					if (chain_len[2] >= 0) {
						if (lane == 0) bam_md_tail(md.r, rec, seq, t.rlen, p, room - (int64_t)(p - a.sam), chain_len[2]);
						p += 3 + chain_len[2] + 1;
						if ((int64_t)(p - a.sam) > room) break;      // (the size kernel counted another string: the check below reports it, nothing more is written)
					}
				}
				if constexpr (kRg) {
					// the read group behind the record's tags (a record without tags has none)
					if (chain_len[1] > 0) {
						if ((int64_t)(p - a.sam) + a.rg_len > room) { p += a.rg_len; break; }      // (as above)
						for (int k = lane; k < a.rg_len; k += 64) p[k] = a.rg[k];
						p += a.rg_len;
					}
				}
			}
			if (lane == 0 && (int64_t)(p - a.sam) != room) atomicAdd(&a.ctl[1], 1ull);
		}
		__syncthreads();
	}
}

__global__ void sam_reset_kernel(SamArgs a)
{
	if (threadIdx.x < 4) a.ctl[threadIdx.x] = 0;
}

// Measurement aid (KG_STREAM_CHECKSUM, bench.py's gpu_pipeline leg): the batch's SAM text summed on the device -- ctl[2] += the sum of its bytes,
// ctl[3] += its line feeds -- so that a run whose text is never copied into file pages still shows WHICH text it made (both figures are
// independent of how the text is cut into batches).  16 bytes per lane and step, one pair of atomics per wave.
__global__ __launch_bounds__(256) void sam_checksum_kernel(SamArgs a)
{
	const int64_t bytes = a.sam_off[a.n_reads];
	const int64_t n16 = bytes >> 4;
	unsigned long long sum = 0, lines = 0;
	const uint4 *src = reinterpret_cast<const uint4 *>(a.sam);
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
		const uint4 v = src[i];
		const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			sum += (w[k] & 255u) + ((w[k] >> 8) & 255u) + ((w[k] >> 16) & 255u) + (w[k] >> 24);
			const uint32_t x = w[k] ^ 0x0A0A0A0Au;                                   // a zero byte where the text holds '\n'
			lines += __popc(((x - 0x01010101u) & ~x) & 0x80808080u);
		}
	}
	if (blockIdx.x == 0 && threadIdx.x < (bytes & 15)) {
		const uint8_t c = a.sam[(n16 << 4) + threadIdx.x];
		sum += c; lines += c == 10 ? 1 : 0;
	}
	for (int off = 32; off > 0; off >>= 1) { sum += __shfl_down(sum, off); lines += __shfl_down(lines, off); }
	if ((threadIdx.x & 63) == 0 && (sum | lines)) { atomicAdd(&a.ctl[2], sum); atomicAdd(&a.ctl[3], lines); }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
namespace {

struct Widen32 {
	__host__ __device__ __forceinline__ int64_t operator()(const int32_t &x) const { return (int64_t)x; }
};
using Wide32Iter = hipcub::TransformInputIterator<int64_t, Widen32, const int32_t *>;

inline int grid_of(int64_t items, int block, int max_blocks)
{
	int64_t g = (items + block - 1) / block;
	if (g < 1) g = 1;
	if (g > max_blocks) g = max_blocks;
	return (int)g;
}

}  // namespace

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
	size_t tb = scan_temp_bytes;
	Wide32Iter it(a.read_len, Widen32());
	if ((e = hipcub::DeviceScan::ExclusiveSum(scan_temp, tb, it, a.read_off, (int)(a.max_reads + 1), stream)) != hipSuccess) return e;
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

// one of the four instantiations of a kernel pair: format and MD:Z at run time, the read group (kRg) as the caller found it
template <bool kRg> static void launch_size(const SamArgs &a, bool bam, const MdRef *md, dim3 grid, hipStream_t stream)
{
	if (bam && md) hipLaunchKernelGGL((bam_size_kernel<true, kRg>), grid, dim3(256), 0, stream, a, MdArg<true>{*md});
	else if (bam) hipLaunchKernelGGL((bam_size_kernel<false, kRg>), grid, dim3(256), 0, stream, a, MdArg<false>{});
	else if (md) hipLaunchKernelGGL((sam_size_kernel<true, kRg>), grid, dim3(256), 0, stream, a, MdArg<true>{*md});
	else hipLaunchKernelGGL((sam_size_kernel<false, kRg>), grid, dim3(256), 0, stream, a, MdArg<false>{});
}
template <bool kRg> static void launch_format(const SamArgs &a, bool bam, const MdRef *md, dim3 grid, hipStream_t stream)
{
	if (bam && md) hipLaunchKernelGGL((bam_format_kernel<true, kRg>), grid, dim3(64), 0, stream, a, MdArg<true>{*md});
	else if (bam) hipLaunchKernelGGL((bam_format_kernel<false, kRg>), grid, dim3(64), 0, stream, a, MdArg<false>{});
	else if (md) hipLaunchKernelGGL((sam_format_kernel<true, kRg>), grid, dim3(64), 0, stream, a, MdArg<true>{*md});
	else hipLaunchKernelGGL((sam_format_kernel<false, kRg>), grid, dim3(64), 0, stream, a, MdArg<false>{});
}

// the size of every read's text and their scan, then the text itself; bam: BAM records in the place of the SAM lines (they count into the same slots)
hipError_t launch_text_size(const SamArgs &a, bool bam, const MdRef *md, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream)
{
	kt_begin(KT_SAM_SIZE, stream);
	hipLaunchKernelGGL(sam_reset_kernel, dim3(1), dim3(64), 0, stream, a);
	const dim3 grid(grid_of(a.n_reads, 256, n_cu * 16));
	if (a.rg_len > 0) launch_size<true>(a, bam, md, grid, stream);
	else launch_size<false>(a, bam, md, grid, stream);
	size_t tb = scan_temp_bytes;
	Wide32Iter it(a.sam_len, Widen32());
	hipError_t e = hipcub::DeviceScan::ExclusiveSum(scan_temp, tb, it, a.sam_off, (int)(a.n_reads + 1), stream);
	if (e != hipSuccess) return e;
	kt_end(KT_SAM_SIZE, stream);
	return hipGetLastError();
}

hipError_t launch_text_format(const SamArgs &a, bool bam, const MdRef *md, int n_cu, hipStream_t stream)
{
	if (a.n_reads <= 0) return hipSuccess;
	kt_begin(KT_SAM_FORMAT, stream);
	const dim3 grid(grid_of((a.n_reads + 63) / 64, 1, n_cu * 64));
	if (a.rg_len > 0) launch_format<true>(a, bam, md, grid, stream);
	else launch_format<false>(a, bam, md, grid, stream);
	kt_end(KT_SAM_FORMAT, stream);
	return hipGetLastError();
}

hipError_t launch_sam_checksum(const SamArgs &a, int n_cu, hipStream_t stream)
{
	if (a.n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(sam_checksum_kernel, dim3(n_cu * 8), dim3(256), 0, stream, a);
	return hipGetLastError();
}

}  // namespace kg
