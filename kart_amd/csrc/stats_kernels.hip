// stats_kernels.hip -- the tally of a batch's output records, per chunk, on the device (gfx950; kg_stream_set_stats, kg_tally_records).
//
//   stats_tally_kernel  one workgroup per chunk, the chunk's row (KG_STATS_WORDS uint32_t, 8.4 KB) in LDS.  Lanes stride over the chunk's reads and follow
//                       each read's `next` chain into the records behind n_reads.  The 26 words every record may touch (records, FLAG bits, pair classes,
//                       CIGAR sums) are counted in registers and reach the row once per wave; the MAPQ and insert-size bins are LDS atomics, two per
//                       record at most.  Then the row is stored whole, consecutive lanes consecutive words: no global atomics, every word written.
// A record is read once (112 bytes); the work is HBM-bound.  Plain C++, vector loads and stores only.
#include "stats_kernels.hpp"

namespace kg {

namespace {

constexpr int kStatsBlock = 256;
constexpr int kStatsScalars = KG_STATS_MAPQ0;          // words [0, KG_STATS_MAPQ0): counted per lane

static_assert(KG_STATS_FLAG0 + KG_STATS_FLAG_BITS == KG_STATS_PROPER, "the FLAG bits end where the pair classes begin");
static_assert(KG_STATS_CIGAR0 + 2 * KG_STATS_CIGAR_CLASSES == KG_STATS_MAPQ0, "the CIGAR sums end where the MAPQ bins begin");
static_assert(KG_STATS_MAPQ0 + KG_STATS_MAPQ_BINS == KG_STATS_ISIZE0, "the MAPQ bins end where the insert sizes begin");

// M, I, D, S, anything else
__device__ __forceinline__ int cigar_class(char c) { return c == 'M' ? 0 : c == 'I' ? 1 : c == 'D' ? 2 : c == 'S' ? 3 : 4; }

}  // namespace

__global__ __launch_bounds__(kStatsBlock) void stats_tally_kernel(StatsArgs a)
{
	__shared__ uint32_t row[KG_STATS_WORDS];
	const int c = blockIdx.x;
	for (int i = threadIdx.x; i < KG_STATS_WORDS; i += kStatsBlock) row[i] = 0;
	__syncthreads();
	uint32_t cnt[kStatsScalars];
#pragma unroll
	for (int i = 0; i < kStatsScalars; ++i) cnt[i] = 0;
	// (a chunk's range outside the reads is a table this kernel does not understand: nothing of it is read)
	int64_t q0 = a.chunk_off[c], q1 = a.chunk_off[c + 1];
	if (q0 < 0) q0 = 0;
	if (q1 > a.n_reads) q1 = a.n_reads;
	const int64_t behind = a.n_records - a.n_reads;        // the longest chain there can be: a longer one goes in circles
	for (int64_t q = q0 + threadIdx.x; q < q1; q += kStatsBlock) {
		int64_t at = q;
		for (int64_t step = 0; step <= behind; ++step) {
			const kg_aln_record &rec = a.records[at];
			const int kind = rec.kind;
			if (kind == KG_ALN_HOST) break;                // the caller decides the read, and counts what it prints for it
			if (kind == KG_ALN_UNMAPPED || kind == KG_ALN_MAPPED) {
				const bool shown = kind == KG_ALN_MAPPED;      // the record prints its own MAPQ, mate columns and CIGAR (else 0, "*", "*")
				const uint32_t flag = (uint32_t)rec.flag;
				const bool mapped = (flag & 4) == 0, paired = (flag & 1) != 0;
				cnt[KG_STATS_RECORDS] += 1;
#pragma unroll
				for (int b = 0; b < KG_STATS_FLAG_BITS; ++b) cnt[KG_STATS_FLAG0 + b] += (flag >> b) & 1u;
				cnt[KG_STATS_PROPER] += (paired && (flag & 2) && mapped) ? 1u : 0u;
				cnt[KG_STATS_BOTH_MAPPED] += (paired && (flag & 12) == 0) ? 1u : 0u;
				cnt[KG_STATS_SINGLETON] += (paired && mapped && (flag & 8)) ? 1u : 0u;
				if (mapped) {
					const uint32_t mq = shown ? (uint32_t)rec.mapq : 0u;        // (a negative MAPQ is no MAPQ: bin 63 with everything above)
					atomicAdd(&row[KG_STATS_MAPQ0 + (mq < KG_STATS_MAPQ_BINS ? mq : KG_STATS_MAPQ_BINS - 1)], 1u);
					const int len = shown && rec.cigar_len < KG_ALN_CIGAR_MAX ? rec.cigar_len : 0;
					uint32_t v = 0;
					for (int i = 0; i < len; ++i) {
						const char ch = rec.cigar[i];
						if (ch >= '0' && ch <= '9') { v = v * 10u + (uint32_t)(ch - '0'); continue; }
						const int k = cigar_class(ch);
#pragma unroll
						for (int j = 0; j < KG_STATS_CIGAR_CLASSES; ++j) {
							cnt[KG_STATS_CIGAR0 + 2 * j] += j == k ? v : 0u;
							cnt[KG_STATS_CIGAR0 + 2 * j + 1] += j == k ? 1u : 0u;
						}
						v = 0;
					}
				}
				if (paired && shown && rec.has_mate && rec.tlen > 0)
					atomicAdd(&row[KG_STATS_ISIZE0 + (rec.tlen < KG_STATS_ISIZE_MAX ? rec.tlen : KG_STATS_ISIZE_MAX)], 1u);
			}
			const int64_t next = rec.next;
			if (next < a.n_reads || next >= a.n_records) break;
			at = next;
		}
	}
	// the lanes' counts: one sum per wave, one LDS atomic per wave and word
#pragma unroll
	for (int i = 0; i < kStatsScalars; ++i) {
		uint32_t v = cnt[i];
		for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
		if ((threadIdx.x & 63) == 0 && v) atomicAdd(&row[i], v);
	}
	__syncthreads();
	uint32_t *out = a.rows + (size_t)c * KG_STATS_WORDS;
	for (int i = threadIdx.x; i < KG_STATS_WORDS; i += kStatsBlock) out[i] = row[i];
}

hipError_t launch_stats_tally(const StatsArgs &a, hipStream_t stream)
{
	if (a.n_chunks <= 0) return hipSuccess;
	kt_begin(KT_STATS, stream);
	hipLaunchKernelGGL(stats_tally_kernel, dim3((unsigned)a.n_chunks), dim3(kStatsBlock), 0, stream, a);
	kt_end(KT_STATS, stream);
	return hipGetLastError();
}

}  // namespace kg
