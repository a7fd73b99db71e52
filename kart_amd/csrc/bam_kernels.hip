// bam_kernels.hip -- bam_size_kernel / bam_format_kernel (gfx950; kg_stream_set_format): the pair of sam_kernels.hip, templates on kMd and kRg alike.
// The same records as BAM (SAM/BAM specification v1, section 4.2) instead of text: for every read the device decides, its records in print
// order, each behind its block_size, byte for byte what the host's encoder (host/detail/bam.inc, bam_from_sam_line) makes of the line
// sam_format_kernel prints for the record -- that encoder parses the printed line, so its view of the line is the contract:
//   l_read_name is a byte, FLAG / n_cigar_op 16 bits, POS / PNEXT / TLEN 32 bits (each cut to its width);
//   a one-character read "*" shown as held is "no sequence" (l_seq 0);
//   the qualities are l_seq bytes of 0xFF unless the column holds exactly l_seq characters -- fewer, a lone "*", or a tab among them
//   (the column ends there) all give 0xFF; NM / AS / XS in the smallest integer type that holds the value;
//   a quality line shorter than its read brings its line feed along as its last quality (GetNextEntry cuts the line to the read's length, not at
//   the line feed): the printed line breaks there, the record ends with its 0xFF qualities, and the tags -- a piece of text that is no record -- go.
#include "text_device.hpp"

namespace kg {

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
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_reads; r += (int64_t)gridDim.x * blockDim.x)
		size_read(a, r, [&](const ReadText &t, const kg_aln_record &rec) { return bam_record_size<kMd>(t, rec, bam_lseq(a, r, t.rlen, rec), a.enc + a.read_off[r], md, rg_bytes<kRg>(a)); });
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
				if (ReadRoute::prints(rec)) {
					const ReadText t = read_text(a, r);
					const int64_t o0 = a.sam_off[r], o1 = a.sam_off[r + 1];
					const int lseq = bam_lseq(a, r, t.rlen, rec);
					d.name = t.name; d.qual = t.qual; d.seq = a.enc + a.read_off[r];
					d.out = a.sam + o0;
					d.room = (int32_t)(o1 - o0);
					d.name_len = (int16_t)t.name_len; d.lseq = (int16_t)lseq;
					int nC = 0, nT = 0;
					ReadRoute o(a, rec, t, o1);
					uint8_t *S = str + lane * kBamSlot;
					if constexpr (kMd) {
						// (an MD beyond the slot: the record-by-record path as well)
						int md_n = -1;
						if (!o.chained) bam_build<1>(t, rec, lseq, reinterpret_cast<uint32_t *>(S), reinterpret_cast<uint32_t *>(S + kBamH), S + kBamH + kBamC, nC, nT, rg_bytes<kRg>(a), &md.r, d.seq, &md_n);
						o.chained = o.chained || md_n > kMdLds;
					} else
					if (!o.chained) bam_build<0>(t, rec, lseq, reinterpret_cast<uint32_t *>(S), reinterpret_cast<uint32_t *>(S + kBamH), S + kBamH + kBamC, nC, nT, rg_bytes<kRg>(a));
					d.nC = (uint8_t)nC; d.nT = (uint8_t)nT;
					const bool qfill = t.qlen != lseq || (lseq == 1 && t.qual[0] == '*') || bam_qual_breaks(t);
					d.flags = (uint8_t)(o.flags() | (qfill ? 16 : 0));
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
			chunk_list(chunk_pre, lane, on ? ((((dm.lseq + 1) >> 1) + 15) >> 4) + ((dm.lseq + 15) >> 4) : 0);
		}
		__syncthreads();
		for_each_chunk(chunk_pre, lane, [&](int line, int c) {
			const BamDesc &d = desc[line];
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
						const U128 lo = *reinterpret_cast<const U128 *>(d.seq + lseq - 32 - b0), hi = *reinterpret_cast<const U128 *>(d.seq + lseq - 16 - b0);
						w0 = comp8(__builtin_bswap64(hi.hi)); w1 = comp8(__builtin_bswap64(hi.lo));
						w2 = comp8(__builtin_bswap64(lo.hi)); w3 = comp8(__builtin_bswap64(lo.lo));
					} else {
						const U128 lo = *reinterpret_cast<const U128 *>(d.seq + b0), hi = *reinterpret_cast<const U128 *>(d.seq + b0 + 16);
						w0 = lo.lo; w1 = lo.hi; w2 = hi.lo; w3 = hi.hi;
					}
					U128 o;
					o.lo = (uint64_t)bam_pack8(w0) | (uint64_t)bam_pack8(w1) << 32;
					o.hi = (uint64_t)bam_pack8(w2) | (uint64_t)bam_pack8(w3) << 32;
					*reinterpret_cast<U128 *>(dst) = o;
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
					U128 v;
					v.lo = v.hi = ~0ull;
					if (!fill) {
						v = *reinterpret_cast<const U128 *>(rev ? d.qual + lseq - 16 - off : d.qual + off);
						if (has_tab8(v.lo) || has_tab8(v.hi)) { tab_seen[line] = 1; tab_seen[64] = 1; }
						if (rev) { const uint64_t lo = __builtin_bswap64(v.hi), hi = __builtin_bswap64(v.lo); v.lo = lo; v.hi = hi; }
						v.lo = bam_qual8(v.lo); v.hi = bam_qual8(v.hi);
					}
					*reinterpret_cast<U128 *>(dst) = v;
				} else {
					for (int k = off; k < lseq; ++k) {
						const uint8_t b = fill ? (uint8_t)0 : rev ? d.qual[lseq - 1 - k] : d.qual[k];
						if (!fill && b == '\t') { tab_seen[line] = 1; tab_seen[64] = 1; }
						dst[k - off] = fill ? (uint8_t)0xFF : (uint8_t)(b - 33);
					}
				}
			}
		});
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

// the pair's launches for launch_text_size / launch_text_format (sam_kernels.hip): MD:Z and the read group pick the instantiation, as there
void launch_bam_size(const SamArgs &a, const MdRef *md, dim3 grid, hipStream_t stream)
{
	if (md && a.rg_len > 0) hipLaunchKernelGGL((bam_size_kernel<true, true>), grid, dim3(256), 0, stream, a, MdArg<true>{*md});
	else if (md) hipLaunchKernelGGL((bam_size_kernel<true, false>), grid, dim3(256), 0, stream, a, MdArg<true>{*md});
	else if (a.rg_len > 0) hipLaunchKernelGGL((bam_size_kernel<false, true>), grid, dim3(256), 0, stream, a, MdArg<false>{});
	else hipLaunchKernelGGL((bam_size_kernel<false, false>), grid, dim3(256), 0, stream, a, MdArg<false>{});
}

void launch_bam_format(const SamArgs &a, const MdRef *md, dim3 grid, hipStream_t stream)
{
	if (md && a.rg_len > 0) hipLaunchKernelGGL((bam_format_kernel<true, true>), grid, dim3(64), 0, stream, a, MdArg<true>{*md});
	else if (md) hipLaunchKernelGGL((bam_format_kernel<true, false>), grid, dim3(64), 0, stream, a, MdArg<true>{*md});
	else if (a.rg_len > 0) hipLaunchKernelGGL((bam_format_kernel<false, true>), grid, dim3(64), 0, stream, a, MdArg<false>{});
	else hipLaunchKernelGGL((bam_format_kernel<false, false>), grid, dim3(64), 0, stream, a, MdArg<false>{});
}

}  // namespace kg
