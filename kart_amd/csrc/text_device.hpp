// text_device.hpp -- what more than one unit of the stream's text stage uses (read_kernels / sam_kernels / bam_kernels / un_kernels .hip; nothing else
// includes it; the layout: DESIGN.md section 4).  Everything device-side here is __device__ __forceinline__ or a plain type: no kernel, no state.
#pragma once
#include "stream_kernels.hpp"

namespace kg {

// bam_kernels.hip: the BAM pair's launches, for launch_text_size / launch_text_format (sam_kernels.hip)
void launch_bam_size(const SamArgs &a, const MdRef *md, dim3 grid, hipStream_t stream);
void launch_bam_format(const SamArgs &a, const MdRef *md, dim3 grid, hipStream_t stream);
// read_kernels.hip (the one unit with the scans): exclusive scan of n 32-bit lengths into 64-bit offsets; temp: what fq_scan_temp_bytes(n) asks for
hipError_t scan_lengths(const int32_t *len, int64_t *off, int64_t n, void *temp, size_t temp_bytes, hipStream_t stream);

namespace {           // (internal to each unit that includes this, as the helpers were in the units they came from)

inline int grid_of(int64_t items, int block, int max_blocks)
{
	int64_t g = (items + block - 1) / block;
	if (g < 1) g = 1;
	if (g > max_blocks) g = max_blocks;
	return (int)g;
}

// ---- bytes ---------------------------------------------------------------------------------------------------------------------
// sixteen bytes at any address (one unaligned load / store)
struct __attribute__((packed, aligned(1))) U128 { uint64_t lo, hi; };

__device__ __forceinline__ int wave_inclusive_scan(int v)
{
	const int lane = threadIdx.x & 63;
	for (int d = 1; d < 64; d <<= 1) {
		int t = __shfl_up(v, d);
		if (lane >= d) v += t;
	}
	return v;
}

// GetComplementaryBase, src/tools.cpp:3-17
__device__ __forceinline__ uint8_t comp_char(uint8_t c)
{
	const uint8_t u = c & 0xDFu;
	return u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N';
}

__device__ __forceinline__ uint64_t comp8(uint64_t x)          // GetComplementaryBase (src/tools.cpp:3-17) on eight characters
{
	const uint64_t u = x & 0xDFDFDFDFDFDFDFDFull;
	auto is = [&](uint64_t c) { const uint64_t t = u ^ (c * 0x0101010101010101ull); return ((~(((t & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | t | 0x7F7F7F7F7F7F7F7Full)) >> 7) * 0xFFull; };
	const uint64_t mA = is(0x41), mC = is(0x43), mG = is(0x47), mT = is(0x54);
	return (mA & 0x5454545454545454ull) | (mC & 0x4747474747474747ull) | (mG & 0x4343434343434343ull) | (mT & 0x4141414141414141ull) | (~(mA | mC | mG | mT) & 0x4E4E4E4E4E4E4E4Eull);
}

// ---- one line by ONE lane: every lane copies its OWN read's line piece by piece with unaligned 16-byte accesses -- a wave instruction moves 1 KB, the 64 lines
// of a wave are consecutive in the output (all 64 lanes on one line, or lines assembled in the LDS first, were slower: profiles/r05t_ab_sam_buf.log).  A piece's
// last partial word is copied whole where the line still has room behind it (the next piece overwrites the surplus), byte by byte at the line's end.
// n bytes of src to p; `end` = the end of the line (writing up to 15 bytes past the piece is fine below it)
__device__ __forceinline__ uint8_t *lane_copy(uint8_t *p, const uint8_t *end, const uint8_t *src, int n)
{
	int k = 0;
	for (; k + 16 <= n; k += 16) *reinterpret_cast<U128 *>(p + k) = *reinterpret_cast<const U128 *>(src + k);
	if (k < n) {
		if (p + k + 16 <= end) *reinterpret_cast<U128 *>(p + k) = *reinterpret_cast<const U128 *>(src + k);
		else for (; k < n; ++k) p[k] = src[k];
	}
	return p + n;
}

// ---- the long pieces of 64 lines (SAM: bases and qualities; BAM: packed bases and qualities; -un: whole records) as ONE list of 16-byte chunks, line after
// line, lane l taking chunks l, l + 64, ...: consecutive lanes move consecutive chunks of a line -- whole 128-byte lines of memory per instruction on either
// side, every lane busy in every step.  (A line per lane moved the same bytes with the same number of instructions but touched 64 different memory lines per
// instruction; eight or sixteen lanes per line left lanes idle: 83 ms against 77 per 100 M reads.)
// every lane of the wave: `mine` = the chunks of line `lane`; chunk_pre[i] = the chunks of the lines before line i, [64] their total.  A barrier before the walk
__device__ __forceinline__ void chunk_list(int *chunk_pre, int lane, int mine)
{
	const int incl = wave_inclusive_scan(mine);
	if (lane == 0) chunk_pre[0] = 0;
	chunk_pre[lane + 1] = incl;
}

// f(line, c) for every chunk of this lane: chunk c of line `line`
template <class F>
__device__ __forceinline__ void for_each_chunk(const int *chunk_pre, int lane, F f)
{
	const int total = chunk_pre[64];
	int line = 0;
	for (int idx = lane; idx < total; idx += 64) {
		while (idx >= chunk_pre[line + 1]) ++line;
		f(line, idx - chunk_pre[line]);
	}
}

// ---- a read of the batch ---------------------------------------------------------------------------------------------------------
// the quality column of a read without qualities (FASTA)
__device__ const uint8_t kNoQual[16] = {'*'};

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

// characters "%u" prints
__device__ __forceinline__ int u32_chars(uint32_t u)
{
	return u < 10u ? 1 : u < 100u ? 2 : u < 1000u ? 3 : u < 10000u ? 4 : u < 100000u ? 5 : u < 1000000u ? 6 : u < 10000000u ? 7 : u < 100000000u ? 8 : u < 1000000000u ? 9 : 10;
}

#include "kernels/md_tag.inc"

// MD in a lane's LDS slot (the lane-per-read path of either format kernel): at most this many characters; a record with a longer one takes the
// record-by-record path, which prints it straight into the output
constexpr int kMdLds = 58;

// the bytes of the read group field behind a record (SamArgs::rg), where the kernel writes one
template <bool kRg> __device__ __forceinline__ int rg_bytes(const SamArgs &a) { return kRg ? a.rg_len : 0; }

// ---- what the two formats' kernels do alike -----------------------------------------------------------------------------------------
// the size kernel of either format, read r: a read the device does not print (KG_ALN_HOST) into host_list, for any other the sum of size(t, record) over its
// own record and those chained behind it (-m) into sam_len.  (The grid-stride loop stays in the kernels: outside a kernel blockDim is not folded to the uniform block size.)
template <class Size>
__device__ __forceinline__ void size_read(const SamArgs &a, int64_t r, Size size)
{
	const kg_aln_record &first = a.records[r];
	int n = 0;
	if (first.kind == KG_ALN_HOST) {
		a.host_list[atomicAdd(&a.ctl[0], 1ull)] = (int32_t)r;
	} else {
		const ReadText t = read_text(a, r);
		for (int64_t at = r; at >= 0; at = a.records[at].next) n += size(t, a.records[at]);
	}
	a.sam_len[r] = n;
}

// phase 1 of either format kernel, read r with its own record rec: does the read print here, and on which path.  (Two steps, the second behind the loads
// of the read's text and offsets, where the kernels decided before: asking both at once moved those loads and cost either format kernel 12 VGPRs.)
struct ReadRoute {
	// flip: the other strand is shown; qrev: the qualities go reversed (a second mate is held reversed); wide: beyond the descriptors' 16-bit fields or the
	// output buffer; chained: the record-by-record path -- wide, records behind the read's own (-m), or its own is none to print
	bool flip, qrev, wide, chained;
	static __device__ __forceinline__ bool prints(const kg_aln_record &rec)
	{
		const int kind = rec.kind;
		return kind == KG_ALN_UNMAPPED || kind == KG_ALN_MAPPED || (kind != KG_ALN_HOST && rec.next >= 0);
	}
	__device__ __forceinline__ ReadRoute(const SamArgs &a, const kg_aln_record &rec, const ReadText &t, int64_t o1)
	{
		const int kind = rec.kind;
		flip = kind == KG_ALN_MAPPED && rec.flip;
		qrev = flip != t.held_reversed;
		wide = t.rlen > 32000 || t.name_len > 32000 || o1 > a.sam_capacity;
		chained = rec.next >= 0 || wide || (kind != KG_ALN_UNMAPPED && kind != KG_ALN_MAPPED);
	}
	__device__ __forceinline__ uint8_t flags() const { return (uint8_t)(1 | (flip ? 2 : 0) | (qrev ? 4 : 0) | (chained ? 8 : 0)); }      // FmtDesc / BamDesc
};

}  // namespace

}  // namespace kg
