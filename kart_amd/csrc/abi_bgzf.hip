// abi_bgzf.hip -- kg_bgzf_deflate: bytes on the host in, BGZF blocks made on the device out (declared in include/kart_amd.h).
// The kernels alone (bgzf_kernels.hpp); a stream runs the same launch on its lanes' records (abi_stream.hip, KG_STREAM_FORMAT_BAM_BGZF).
#include "abi_internal.hpp"
#include "bgzf_kernels.hpp"

#include <algorithm>

#define fail kg_fail

namespace {

// the call's device buffers, freed on every way out
struct Buffers {
	std::vector<void *> all;
	template <class T> hipError_t get(T *&p, size_t bytes)
	{
		hipError_t e = hipMalloc((void **)&p, std::max<size_t>(bytes, 16));
		if (e == hipSuccess) all.push_back((void *)p);
		return e;
	}
	~Buffers()
	{
		for (void *p : all) (void)hipFree(p);
	}
};

}  // namespace

extern "C" int kg_bgzf_deflate(int device, const uint8_t *src, int64_t src_bytes, const int64_t *cuts, int64_t n_cuts, uint8_t *dst, int64_t dst_capacity,
                               int64_t *block_src, int64_t *block_off, int64_t max_blocks, int64_t *n_blocks)
{
	if (src_bytes < 0 || (!src && src_bytes > 0) || !cuts || n_cuts < 1 || (!dst && dst_capacity > 0) || dst_capacity < 0 || !block_src || !block_off || max_blocks < 0 || !n_blocks)
		return fail(KG_ERR_ARG, "kg_bgzf_deflate: bad argument");
	if (n_cuts > INT32_MAX - 1 || max_blocks > INT32_MAX - 2) return fail(KG_ERR_ARG, "kg_bgzf_deflate: %lld cuts / %lld blocks are more than one call takes", (long long)n_cuts, (long long)max_blocks);
	if (cuts[0] != 0 || cuts[n_cuts - 1] != src_bytes) return fail(KG_ERR_ARG, "kg_bgzf_deflate: the cuts run from %lld to %lld, not from 0 to src_bytes = %lld", (long long)cuts[0], (long long)cuts[n_cuts - 1], (long long)src_bytes);
	int64_t need_blocks = 0;
	for (int64_t i = 0; i + 1 < n_cuts; ++i) {
		if (cuts[i + 1] < cuts[i]) return fail(KG_ERR_ARG, "kg_bgzf_deflate: cut %lld (%lld) lies in front of cut %lld (%lld)", (long long)(i + 1), (long long)cuts[i + 1], (long long)i, (long long)cuts[i]);
		need_blocks += (cuts[i + 1] - cuts[i] + kBgzfPayload - 1) / kBgzfPayload;
	}
	*n_blocks = 0;
	if (need_blocks > max_blocks) return fail(KG_ERR_CAPACITY, "kg_bgzf_deflate: the cuts make %lld blocks, the tables hold %lld", (long long)need_blocks, (long long)max_blocks);
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return fail(KG_ERR_NO_DEVICE, "kg_bgzf_deflate: no HIP device %d", device);
	HIP_TRY(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	const int n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

	// the members are gathered into a device buffer that holds them whatever they come to (a stored member is its payload + 31 bytes), so that the
	// caller's capacity is checked against the size they did come to
	Buffers buf;
	BgzfArgs a{};
	uint8_t *d_src = nullptr;
	int64_t *d_cuts = nullptr;
	void *d_scan = nullptr;
	const int64_t table = need_blocks + 1, dst_room = src_bytes + 31 * need_blocks;
	const size_t scan_bytes = bgzf_scan_temp_bytes(std::max(n_cuts, table));
	HIP_TRY(buf.get(d_src, (size_t)src_bytes));
	HIP_TRY(buf.get(d_cuts, 8 * (size_t)n_cuts));
	HIP_TRY(buf.get(a.range_first, 8 * (size_t)n_cuts));
	HIP_TRY(buf.get(a.block_src, 8 * (size_t)table));
	HIP_TRY(buf.get(a.block_bytes, 4 * (size_t)table));
	HIP_TRY(buf.get(a.block_off, 8 * (size_t)table));
	HIP_TRY(buf.get(a.slots, (size_t)(need_blocks * kBgzfSlot)));
	HIP_TRY(buf.get(a.dst, (size_t)dst_room));
	HIP_TRY(buf.get(a.ctl, 8 * BGZ_WORDS));
	HIP_TRY(buf.get(d_scan, scan_bytes));
	if (src_bytes > 0) HIP_TRY(hipMemcpy(d_src, src, (size_t)src_bytes, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_cuts, cuts, 8 * (size_t)n_cuts, hipMemcpyHostToDevice));
	HIP_TRY(hipMemset(a.ctl, 0, 8 * BGZ_WORDS));
	a.src = d_src; a.src_bytes = src_bytes; a.cuts = d_cuts; a.n_cuts = n_cuts; a.max_blocks = need_blocks; a.dst_capacity = dst_room;
	HIP_TRY(launch_bgzf(a, d_scan, scan_bytes, n_cu, nullptr));
	unsigned long long ctl[BGZ_WORDS];
	HIP_TRY(hipMemcpy(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
	const int64_t made = (int64_t)ctl[BGZ_RUN], bytes = (int64_t)ctl[BGZ_BYTES];
	if ((int64_t)ctl[BGZ_BLOCKS] != need_blocks || made != need_blocks) return fail(KG_ERR_NO_DEVICE, "kg_bgzf_deflate: the device planned %lld blocks where the cuts make %lld", (long long)ctl[BGZ_BLOCKS], (long long)need_blocks);
	if (ctl[BGZ_ERRORS] != 0) return fail(KG_ERR_NO_DEVICE, "kg_bgzf_deflate: %lld members missed the size computed for them", (long long)ctl[BGZ_ERRORS]);
	if (bytes > dst_room) return fail(KG_ERR_NO_DEVICE, "kg_bgzf_deflate: %lld bytes of members where at most %lld can be", (long long)bytes, (long long)dst_room);
	if (bytes > dst_capacity) return fail(KG_ERR_CAPACITY, "kg_bgzf_deflate: the members take %lld bytes, dst holds %lld", (long long)bytes, (long long)dst_capacity);
	if (bytes > 0) HIP_TRY(hipMemcpy(dst, a.dst, (size_t)bytes, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(block_src, a.block_src, 8 * (size_t)(made + 1), hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(block_off, a.block_off, 8 * (size_t)(made + 1), hipMemcpyDeviceToHost));
	*n_blocks = made;
	return KG_OK;
}
