// sam_kernels.hip -- the stream's output side, on the device (gfx950): the records of a batch as SAM text, and the side's two entry points.
// = OutputPairedAlignments / OutputSingledAlignments (reference src/Mapping.cpp:177-315) for every kg_aln_record of the batch:
//   sam_size_kernel                     exact byte count of the line(s) of every read -> scan -> offsets
//   sam_format_kernel                   one wave per 64 reads: every lane prints the numeric fields of one read into the LDS, then all
//                                       lanes move each read's pieces -- name, FLAG .. TLEN, sequence (reverse-complemented for a
//                                       record shown on the other strand), qualities (reversed likewise), NM / AS / XS.
//   (templates on kMd: with kg_stream_set_tags(KG_STREAM_TAG_MD) every mapped record carries MD:Z behind XS, kernels/md_tag.inc; without, the
//   instantiation is the code as it was before the tag existed; and on kRg: with kg_stream_set_read_group EVERY record carries RG:Z as its last field,
//   a constant of the batch copied from SamArgs::rg like a contig name -- the line feed of a SAM line then comes from the copy, not from the tags)
// Byte work, HBM-bound, no MFMA.  Everything is integer / character arithmetic; results are bit-identical to the host pipeline's
// text (tests/test_stream_gpu.py, and every SAM parity test runs through this path).
#include "text_device.hpp"

namespace kg {

namespace {

// characters "%d" / "%lld" print.  Every number of a SAM line fits 32 bits in practice (positions are contig-relative, contig
// lengths are 32-bit in the index format); 32-bit division by the constant 10 is a multiply, a 64-bit one a subroutine.
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

#define SAM_UNMAPPED_MID "\t*\t0\t0\t*\t*\t0\t0\t"
#define SAM_UNMAPPED_TAIL "\tAS:i:0\tXS:i:0\n"

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
__global__ __launch_bounds__(256) void sam_size_kernel(SamArgs a, MdArg<kMd> md)
{
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_reads; r += (int64_t)gridDim.x * blockDim.x)
		size_read(a, r, [&](const ReadText &t, const kg_aln_record &rec) { return record_size<kMd, kRg>(a, t, rec, a.enc + a.read_off[r], md); });
	if (blockIdx.x == 0 && threadIdx.x == 0) a.sam_len[a.n_reads] = 0;
}

// One wave per 64 consecutive reads, two phases.
//   1. lane l prints the numeric fields of read base + l ("\tFLAG\t", "\tPOS\tMAPQ\tCIGAR\t=\tPNEXT\tTLEN\t", the tags) into its own slot
//      of the wave's LDS block and leaves there what the copy phase needs (where the name, the qualities, the characters and the
//      contig name lie, where the line goes): 64 records are fetched and printed side by side, not one after the other.
//   2. for each of the 64 reads all lanes move the pieces -- name, contig name, sequence and qualities straight from the FASTQ
//      text / the read characters -- to the output; everything this phase needs per read comes from the LDS.
// A read with further records chained behind it (-m) takes the record-by-record path (format_chain).
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
				if (ReadRoute::prints(rec)) {
					const ReadText t = read_text(a, r);
					const int64_t o0 = a.sam_off[r], o1 = a.sam_off[r + 1];
					d.name = t.name; d.qual = t.qual; d.seq = a.enc + a.read_off[r];
					d.out = a.sam + o0;
					d.room_end_lo = (int32_t)(o1 - o0);
					d.name_len = (int16_t)t.name_len; d.rlen = (int16_t)t.rlen; d.qlen = (int16_t)t.qlen;
					d.chr = a.chr_names; d.n_chr = 0;
					if (rec.kind == KG_ALN_MAPPED) { d.chr = a.chr_names + a.chr_name_off[rec.chr]; d.n_chr = (int16_t)(a.chr_name_off[rec.chr + 1] - a.chr_name_off[rec.chr]); }
					int nA = 0, nB = 0, nT = 0;
					ReadRoute o(a, rec, t, o1);
					if constexpr (kMd) {
						// (an MD beyond the slot: the record-by-record path as well)
						bool over = false;
						if (!o.chained) print_fields<1, kRg>(t, rec, str + lane * kFmtSlot, str + lane * kFmtSlot + kFmtA, str + lane * kFmtSlot + kFmtA + kFmtB, nA, nB, nT, &md.r, d.seq, &over);
						o.chained = o.chained || over;
					} else
					if (!o.chained) print_fields<0, kRg>(t, rec, str + lane * kFmtSlot, str + lane * kFmtSlot + kFmtA, str + lane * kFmtSlot + kFmtA + kFmtB, nA, nB, nT);
					d.nA = (uint8_t)nA; d.nB = (uint8_t)nB; d.nT = (uint8_t)nT;
					d.flags = o.flags();
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
		// ---- phase 2b: the bases and the qualities of the 64 lines as one list of 16-byte chunks (text_device.hpp: a line's bases first, then its qualities;
		//      20 chunks for a 150-base read).  The read as the record shows it: as held, or its reverse complement (GetComplementarySeq) with the qualities
		//      reversed.
		{
			const FmtDesc &dm = desc[lane];
			const bool on = (dm.flags & 1) && !(dm.flags & 8);
			chunk_list(chunk_pre, lane, on ? ((dm.rlen + 15) >> 4) + ((dm.qlen + 15) >> 4) : 0);
		}
		__syncthreads();
		for_each_chunk(chunk_pre, lane, [&](int line, int c) {
			const FmtDesc &d = desc[line];
			const int n_seq = (d.rlen + 15) >> 4;
			const bool is_seq = c < n_seq;
			const int off = (is_seq ? c : c - n_seq) << 4, n = is_seq ? d.rlen : d.qlen;
			const uint8_t *src = is_seq ? d.seq : d.qual;
			uint8_t *dst = d.out + d.name_len + d.nA + d.n_chr + d.nB + (is_seq ? 0 : d.rlen + 1) + off;
			const bool rev = is_seq ? (d.flags & 2) != 0 : (d.flags & 4) != 0;
			if (off + 16 <= n) {
				U128 v = *reinterpret_cast<const U128 *>(rev ? src + n - 16 - off : src + off);
				if (rev) {
					const uint64_t lo = __builtin_bswap64(v.hi), hi = __builtin_bswap64(v.lo);
					v.lo = lo; v.hi = hi;
					if (is_seq) { v.lo = comp8(v.lo); v.hi = comp8(v.hi); }
				}
				*reinterpret_cast<U128 *>(dst) = v;
			} else {
				for (int k = off; k < n; ++k) {
					const uint8_t b = rev ? src[n - 1 - k] : src[k];
					dst[k - off] = rev && is_seq ? comp_char(b) : b;
				}
			}
		});
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

// ---- launches: the output side's entry points.  The format is picked here; MD:Z and the read group pick one of a format's four instantiations here / in bam_kernels.hip
// the size of every read's text and their scan, then the text itself; bam: BAM records in the place of the SAM lines (they count into the same slots)
hipError_t launch_text_size(const SamArgs &a, bool bam, const MdRef *md, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream)
{
	kt_begin(KT_SAM_SIZE, stream);
	hipLaunchKernelGGL(sam_reset_kernel, dim3(1), dim3(64), 0, stream, a);
	const dim3 grid(grid_of(a.n_reads, 256, n_cu * 16));
	if (bam) launch_bam_size(a, md, grid, stream);
	else if (md && a.rg_len > 0) hipLaunchKernelGGL((sam_size_kernel<true, true>), grid, dim3(256), 0, stream, a, MdArg<true>{*md});
	else if (md) hipLaunchKernelGGL((sam_size_kernel<true, false>), grid, dim3(256), 0, stream, a, MdArg<true>{*md});
	else if (a.rg_len > 0) hipLaunchKernelGGL((sam_size_kernel<false, true>), grid, dim3(256), 0, stream, a, MdArg<false>{});
	else hipLaunchKernelGGL((sam_size_kernel<false, false>), grid, dim3(256), 0, stream, a, MdArg<false>{});
	hipError_t e = scan_lengths(a.sam_len, a.sam_off, a.n_reads + 1, scan_temp, scan_temp_bytes, stream);
	if (e != hipSuccess) return e;
	kt_end(KT_SAM_SIZE, stream);
	return hipGetLastError();
}

hipError_t launch_text_format(const SamArgs &a, bool bam, const MdRef *md, int n_cu, hipStream_t stream)
{
	if (a.n_reads <= 0) return hipSuccess;
	kt_begin(KT_SAM_FORMAT, stream);
	const dim3 grid(grid_of((a.n_reads + 63) / 64, 1, n_cu * 64));
	if (bam) launch_bam_format(a, md, grid, stream);
	else if (md && a.rg_len > 0) hipLaunchKernelGGL((sam_format_kernel<true, true>), grid, dim3(64), 0, stream, a, MdArg<true>{*md});
	else if (md) hipLaunchKernelGGL((sam_format_kernel<true, false>), grid, dim3(64), 0, stream, a, MdArg<true>{*md});
	else if (a.rg_len > 0) hipLaunchKernelGGL((sam_format_kernel<false, true>), grid, dim3(64), 0, stream, a, MdArg<false>{});
	else hipLaunchKernelGGL((sam_format_kernel<false, false>), grid, dim3(64), 0, stream, a, MdArg<false>{});
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
