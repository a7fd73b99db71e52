// align_device.hpp -- device helpers that more than one unit of the alignment stage uses (align_pair / align_plan / align_finish .hip;
// nothing else includes it).  Everything here is __device__ __forceinline__ or a plain type: no kernel, no state.
#pragma once
#include "align_launch.hpp"

namespace kg {

namespace {           // (internal to each unit that includes this, as the helpers were in the single unit they came from)

// ---- small helpers --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int text_code(const AlnArgs &a, int64_t g)       // base of the indexed text (forward + reverse complement)
{
	return (a.ix.text[(uint64_t)g >> 2] >> (((uint32_t)g & 3) << 1)) & 3;
}
__device__ __forceinline__ char text_char(const AlnArgs &a, int64_t g)      // RefSequence[g]: always upper-case ACGT
{
	int c = text_code(a, g);
	return c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : 'T';
}

struct __attribute__((packed, aligned(1))) AlnU64u { uint64_t v; };

// 32 bases of the 2-bit text from position p (base i in bits 2 i); beyond the end of the text: zeros
__device__ __forceinline__ uint64_t text_word32(const AlnArgs &a, int64_t p)
{
	if (p > a.two_genome_size) return 0;                 // (the text buffer has 16 bytes of slack behind its last base)
	const uint8_t *tp = a.ix.text + ((uint64_t)p >> 2);
	uint64_t lo = reinterpret_cast<const AlnU64u *>(tp)->v, hi = tp[8];
	int sh = ((int)p & 3) << 1;
	return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

__device__ __forceinline__ int chunk_of(const AlnArgs &a, int64_t r)
{
	// (the chunks of a batch are equally long but for the last: the proportional guess is right, two independent loads confirm it;
	//  the search below -- ~8 dependent loads for the 250 chunks of a 1 M-read batch -- is only the fallback)
	if (a.n_chunks > 1 && a.n_reads > 0) {
		int c = (int)((r * (int64_t)a.n_chunks) / a.n_reads);
		c = c < 0 ? 0 : c > a.n_chunks - 1 ? a.n_chunks - 1 : c;
		if (a.chunk_off[c] <= r && r < a.chunk_off[c + 1]) return c;
	}
	int lo = 0, hi = a.n_chunks - 1;
	while (lo < hi) {
		int mid = (lo + hi + 1) >> 1;
		if (a.chunk_off[mid] <= r) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// ChrLocMap.lower_bound(g): index of the first key >= g, n_ends when there is none
__device__ __forceinline__ int end_lower_bound(const AlnArgs &a, int64_t g)
{
	int lo = 0, hi = a.n_ends;
	while (lo < hi) {
		int mid = (lo + hi) >> 1;
		if (a.contig_end[mid] < g) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// A lane's share of a list whose end is a device counter: the wave's requests are summed and ONE returning atomic takes them all.
// (Every lane asking for itself was the stage's hidden cost: the counters are single addresses -- ctl[0..6] --, fifty million returning
// atomics per 100 M-read step queue at one L2 channel at about one per clock, ~25 ms per kernel whatever else the kernel does.)
// EVERY lane of the wave calls it, at a point where the wave has reconverged (need = 0: nothing for this lane).
__device__ __forceinline__ unsigned long long wave_reserve(unsigned long long *counter, unsigned long long need)
{
	const int lane = threadIdx.x & 63;
	unsigned long long incl = need;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const unsigned long long t = ((unsigned long long)(uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), off) << 32) | (uint32_t)__shfl_up((int)(uint32_t)incl, off);
		if (lane >= off) incl += t;
	}
	const unsigned long long total = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(incl >> 32), 63) << 32) | (uint32_t)__shfl((int)(uint32_t)incl, 63);
	if (total == 0) return 0;
	unsigned long long base = 0;
	if (lane == 63) base = atomicAdd(counter, total);
	base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), 63) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 63);
	return base + incl - need;
}

// why a pair went back to the host (kg_align_reasons)
enum { WHY_PAIR_PRODUCT = 0, WHY_RESCUE_DIR1 = 1, WHY_RESCUE_WINDOW = 2, WHY_RESCUE_READ = 3, WHY_RESCUE_RUNS = 4, WHY_RESCUE_SEEDS = 5, WHY_SEEDS = 6,
       WHY_GAPS = 7, WHY_PARTITION = 8, WHY_CAPACITY = 9, WHY_CIGAR = 10, WHY_SCORE = 11, WHY_READ_LEN = 12 };

__device__ __forceinline__ void flag_host(const AlnArgs &a, int64_t r, int why)       // the pair of read r goes back to the host
{
	atomicAdd(&a.ctl[8 + why], 1ull);
	int c = chunk_of(a, r);
	int64_t base = a.chunk_off[c];
	if (a.chunk_paired[c]) {
		int64_t first = base + (((r - base) >> 1) << 1);
		a.r_host[first] = 1;
		a.r_host[first + 1] = 1;
	} else a.r_host[r] = 1;
}

// ---- the wave as a unit ----
__device__ __forceinline__ void wave_sync_mem()          // the wave's stores to the per-candidate arrays are visible to all its lanes
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ int wave_max(int v) { for (int off = 32; off > 0; off >>= 1) { const int t = __shfl_xor(v, off); v = t > v ? t : v; } return v; }
__device__ __forceinline__ int wave_sum(int v) { for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off); return v; }

// what pass 1 decided for a pair
enum : uint8_t { W_NONE = 0, W_SIMPLE = 1, W_IMMEDIATE = 2, W_JOB = 3, W_PLAN = 4, W_PENDING = 5 };

}  // namespace

}  // namespace kg
