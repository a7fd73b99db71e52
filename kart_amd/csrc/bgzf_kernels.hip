// bgzf_kernels.hip -- BGZF blocks made on the device: plan, deflate, pack (bgzf_kernels.hpp; one block's deflate: kernels/bgzf_block.inc).
#include "bgzf_kernels.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "kernels/bgzf_block.inc"
#include "kernels/bgzf_inflate.inc"

namespace kg {

namespace {

inline int grid_of(int64_t items, int block, int max_blocks)
{
	int64_t g = (items + block - 1) / block;
	if (g < 1) g = 1;
	if (g > max_blocks) g = max_blocks;
	return (int)g;
}

struct MaxI64 {
	__host__ __device__ __forceinline__ int64_t operator()(const int64_t &a, const int64_t &b) const { return a > b ? a : b; }
};

}  // namespace

// ---- plan ----------------------------------------------------------------------------------------------------------------------
// blocks of every range (a range that is empty, or -- the caller checks its cuts -- runs backwards, makes none)
__global__ __launch_bounds__(256) void bgzf_count_kernel(BgzfArgs a)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_cuts; i += stride) {
		const int64_t len = i + 1 < a.n_cuts ? a.cuts[i + 1] - a.cuts[i] : 0;
		a.range_first[i] = len > 0 ? (len + kBgzfPayload - 1) / kBgzfPayload : 0;
	}
}

// the block table from the scanned counts; the sizes start at zero, so that the slots behind the last block add nothing to the scan of the sizes
__global__ __launch_bounds__(256) void bgzf_table_kernel(BgzfArgs a)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x, at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t n_blocks = a.range_first[a.n_cuts - 1];
	const bool fits = n_blocks <= a.max_blocks;
	if (at == 0) {
		a.ctl[BGZ_BLOCKS] = (unsigned long long)n_blocks;
		a.ctl[BGZ_RUN] = fits ? (unsigned long long)n_blocks : 0ull;
		if (fits) a.block_src[n_blocks] = a.src_bytes;
	}
	for (int64_t i = at; i <= a.max_blocks; i += stride) a.block_bytes[i] = 0;
	if (!fits) return;
	for (int64_t i = at; i + 1 < a.n_cuts; i += stride) {
		const int64_t first = a.range_first[i], n = a.range_first[i + 1] - first, from = a.cuts[i];
		for (int64_t k = 0; k < n; ++k) a.block_src[first + k] = from + k * kBgzfPayload;
	}
}

// ---- deflate -------------------------------------------------------------------------------------------------------------------
// one workgroup per block at a time; the whole of BlockShared is the workgroup's LDS (one workgroup per CU)
__global__ __launch_bounds__(bgzf::kThreads) void bgzf_deflate_kernel(BgzfArgs a)
{
	__shared__ bgzf::BlockShared sh;
	const int64_t n_blocks = (int64_t)a.ctl[BGZ_RUN];
	for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
		const int64_t from = a.block_src[b], to = a.block_src[b + 1];
		int bytes = 0;
		if (from >= 0 && to <= a.src_bytes && to - from <= kBgzfPayload)
			bytes = bgzf::deflate_block(sh, a.src + from, (int)(to - from), (uint32_t *)(a.slots + b * kBgzfSlot), &a.ctl[BGZ_ERRORS]);
		if (threadIdx.x == 0) a.block_bytes[b] = bytes;
		__syncthreads();
	}
}

// ---- pack ----------------------------------------------------------------------------------------------------------------------
// member b from its slot to dst[block_off[b] ..): whole words where dst is aligned, the few bytes in front and behind one by one
__global__ __launch_bounds__(256) void bgzf_pack_kernel(BgzfArgs a)
{
	const int64_t n_blocks = (int64_t)a.ctl[BGZ_RUN];
	if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[BGZ_BYTES] = (unsigned long long)a.block_off[a.max_blocks];
	for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
		const int64_t at = a.block_off[b];
		const int size = a.block_bytes[b];
		if (size <= 0 || size > kBgzfSlot || at < 0 || at + size > a.dst_capacity) continue;
		const uint8_t *slot = a.slots + b * kBgzfSlot;
		const uint32_t *slot_w = (const uint32_t *)slot;
		uint8_t *dst = a.dst + at;
		const int lead = (int)((4 - (at & 3)) & 3), head = lead < size ? lead : size, words = (size - head) / 4, tail = size - head - 4 * words;
		uint32_t *dst_w = (uint32_t *)(dst + head);
		for (int w = threadIdx.x; w < words; w += blockDim.x) {
			const int s = head + 4 * w, sh = (s & 3) * 8;
			const uint32_t lo = slot_w[s >> 2];
			dst_w[w] = sh ? (lo >> sh) | (slot_w[(s >> 2) + 1] << (32 - sh)) : lo;     // (sh != 0: s + 4 <= size leaves the next word inside the slot)
		}
		if ((int)threadIdx.x < head) dst[threadIdx.x] = slot[threadIdx.x];
		if ((int)threadIdx.x < tail) dst[head + 4 * words + threadIdx.x] = slot[head + 4 * words + threadIdx.x];
	}
}

// ---- a stream batch's cuts -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bgzf_stream_cuts_kernel(const int64_t *sam_off, int64_t n_reads, int chunk_reads, int64_t *cuts)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_reads; r += stride) {
		const int64_t at = sam_off[r];
		const bool cut = r == n_reads || r % chunk_reads == 0 || sam_off[r + 1] == at;
		cuts[r] = cut ? at : 0;
	}
}

// ---- inflate -------------------------------------------------------------------------------------------------------------------
// one wave per member at a time: a workgroup IS a wave, so that its barriers are fences, and ~8 KiB of LDS let sixteen of them share a CU
__global__ __launch_bounds__(bgzf::kWave) void bgzf_inflate_kernel(BgzfInflateArgs a)
{
	__shared__ bgzf::InflateShared sh;
	for (int64_t i = blockIdx.x; i < a.n_members; i += gridDim.x) {
		const int64_t m0 = a.member_off[i], m1 = a.member_off[i + 1], t0 = a.text_off[i], t1 = a.text_off[i + 1];
		int status;
		if (m0 < 0 || m1 < m0 || m1 > a.src_bytes || m1 - m0 > kBgzfSlot) status = bgzf::kInflateHeader;
		else if (t0 < 0 || t1 < t0 || t1 > a.dst_capacity || t1 - t0 > kBgzfSlot) status = bgzf::kInflateSize;
		else status = bgzf::inflate_member(sh, a.src + m0, (int)(m1 - m0), a.dst + t0, (int)(t1 - t0));
		if (threadIdx.x == 0) a.status[i] = status;
	}
}

size_t bgzf_scan_temp_bytes(int64_t max_items)
{
	size_t b1 = 0, b2 = 0, b3 = 0;
	hipcub::TransformInputIterator<int64_t, hipcub::CastOp<int64_t>, const int32_t *> it((const int32_t *)nullptr, hipcub::CastOp<int64_t>());
	(void)hipcub::DeviceScan::ExclusiveSum(nullptr, b1, (const int64_t *)nullptr, (int64_t *)nullptr, (int)max_items);
	(void)hipcub::DeviceScan::ExclusiveSum(nullptr, b2, it, (int64_t *)nullptr, (int)max_items);
	(void)hipcub::DeviceScan::InclusiveScan(nullptr, b3, (const int64_t *)nullptr, (int64_t *)nullptr, MaxI64(), (int)max_items);
	return std::max(b1, std::max(b2, b3));
}

hipError_t launch_bgzf(const BgzfArgs &a, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream)
{
	if (a.n_cuts < 1 || a.max_blocks < 0) return hipErrorInvalidValue;
	kt_begin(KT_BGZF, stream);
	hipLaunchKernelGGL(bgzf_count_kernel, dim3(grid_of(a.n_cuts, 256, n_cu * 8)), dim3(256), 0, stream, a);
	size_t tb = scan_temp_bytes;
	hipError_t e = hipcub::DeviceScan::ExclusiveSum(scan_temp, tb, (const int64_t *)a.range_first, a.range_first, (int)a.n_cuts, stream);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(bgzf_table_kernel, dim3(grid_of(std::max(a.n_cuts, a.max_blocks + 1), 256, n_cu * 8)), dim3(256), 0, stream, a);
	hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(grid_of(a.max_blocks, 1, n_cu * 4)), dim3(bgzf::kThreads), 0, stream, a);
	hipcub::TransformInputIterator<int64_t, hipcub::CastOp<int64_t>, const int32_t *> it(a.block_bytes, hipcub::CastOp<int64_t>());
	tb = scan_temp_bytes;
	e = hipcub::DeviceScan::ExclusiveSum(scan_temp, tb, it, a.block_off, (int)(a.max_blocks + 1), stream);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(bgzf_pack_kernel, dim3(grid_of(a.max_blocks, 1, n_cu * 8)), dim3(256), 0, stream, a);
	kt_end(KT_BGZF, stream);
	return hipGetLastError();
}

hipError_t launch_bgzf_inflate(const BgzfInflateArgs &a, int n_cu, hipStream_t stream)
{
	if (a.n_members < 0) return hipErrorInvalidValue;
	if (a.n_members == 0) return hipSuccess;
	hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(grid_of(a.n_members, 1, n_cu * 16)), dim3(bgzf::kWave), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_bgzf_stream_cuts(const int64_t *sam_off, int64_t n_reads, int chunk_reads, int64_t *cuts, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(bgzf_stream_cuts_kernel, dim3(grid_of(n_reads + 1, 256, n_cu * 8)), dim3(256), 0, stream, sam_off, n_reads, chunk_reads, cuts);
	size_t tb = scan_temp_bytes;
	hipError_t e = hipcub::DeviceScan::InclusiveScan(scan_temp, tb, (const int64_t *)cuts, cuts, MaxI64(), (int)(n_reads + 1), stream);
	if (e != hipSuccess) return e;
	return hipGetLastError();
}

}  // namespace kg
