// abi_bgzf.hip -- kg_bgzf_deflate: bytes on the host in, BGZF blocks made on the device out; kg_bgzf_inflate / kg_inflater_*: BGZF members in,
// their text out (declared in include/kart_amd.h).
// The kernels alone (bgzf_kernels.hpp); a stream runs the same launch on its lanes' records (abi_stream.hip, KG_STREAM_FORMAT_BAM_BGZF).
#include "abi_internal.hpp"
#include "bgzf_kernels.hpp"

#include <algorithm>
#include <cstring>

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

// ---- kg_bgzf_inflate, kg_inflater_*: BGZF members in, their text out ------------------------------------------------------------
namespace {

// the two tables of a round against each other and against the buffers: 0, or the failure recorded
int check_members(const char *who, int64_t src_bytes, const int64_t *member_off, const int64_t *text_off, int64_t n, int64_t dst_capacity)
{
	if (src_bytes < 0 || n < 0 || !member_off || !text_off || dst_capacity < 0) return fail(KG_ERR_ARG, "%s: bad argument", who);
	if (n > INT32_MAX - 1) return fail(KG_ERR_ARG, "%s: %lld members are more than one call takes", who, (long long)n);
	if (member_off[0] != 0 || member_off[n] != src_bytes)
		return fail(KG_ERR_ARG, "%s: the members run from %lld to %lld, not from 0 to src_bytes = %lld", who, (long long)member_off[0], (long long)member_off[n], (long long)src_bytes);
	if (text_off[0] != 0) return fail(KG_ERR_ARG, "%s: the text begins at %lld, not at 0", who, (long long)text_off[0]);
	for (int64_t i = 0; i < n; ++i) {
		if (member_off[i + 1] < member_off[i] || text_off[i + 1] < text_off[i])
			return fail(KG_ERR_ARG, "%s: the offsets of member %lld lie in front of those of member %lld", who, (long long)(i + 1), (long long)i);
		if (member_off[i + 1] - member_off[i] > kBgzfSlot || text_off[i + 1] - text_off[i] > kBgzfSlot)
			return fail(KG_ERR_ARG, "%s: member %lld has %lld bytes and %lld bytes of text, a BGZF member has at most %lld of either", who, (long long)i,
			            (long long)(member_off[i + 1] - member_off[i]), (long long)(text_off[i + 1] - text_off[i]), (long long)kBgzfSlot);
	}
	if (text_off[n] > dst_capacity) return fail(KG_ERR_CAPACITY, "%s: the text takes %lld bytes, dst holds %lld", who, (long long)text_off[n], (long long)dst_capacity);
	return KG_OK;
}

int device_cus(const char *who, int device, int &n_cu)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return fail(KG_ERR_NO_DEVICE, "%s: no HIP device %d", who, device);
	HIP_TRY(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	return KG_OK;
}

}  // namespace

extern "C" int kg_bgzf_inflate(int device, const uint8_t *src, int64_t src_bytes, const int64_t *member_off, const int64_t *text_off, int64_t n_members,
                               uint8_t *dst, int64_t dst_capacity, int32_t *status)
{
	if ((!src && src_bytes > 0) || (!dst && dst_capacity > 0) || (!status && n_members > 0)) return fail(KG_ERR_ARG, "kg_bgzf_inflate: bad argument");
	if (int rc = check_members("kg_bgzf_inflate", src_bytes, member_off, text_off, n_members, dst_capacity)) return rc;
	int n_cu = 0;
	if (int rc = device_cus("kg_bgzf_inflate", device, n_cu)) return rc;
	if (n_members == 0) return KG_OK;
	const int64_t text_bytes = text_off[n_members];
	Buffers buf;
	BgzfInflateArgs a{};
	uint8_t *d_src = nullptr;
	int64_t *d_member = nullptr, *d_text = nullptr;
	HIP_TRY(buf.get(d_src, (size_t)src_bytes));
	HIP_TRY(buf.get(d_member, 8 * (size_t)(n_members + 1)));
	HIP_TRY(buf.get(d_text, 8 * (size_t)(n_members + 1)));
	HIP_TRY(buf.get(a.dst, (size_t)text_bytes));
	HIP_TRY(buf.get(a.status, 4 * (size_t)n_members));
	if (src_bytes > 0) HIP_TRY(hipMemcpy(d_src, src, (size_t)src_bytes, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_member, member_off, 8 * (size_t)(n_members + 1), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_text, text_off, 8 * (size_t)(n_members + 1), hipMemcpyHostToDevice));
	if (text_bytes > 0) HIP_TRY(hipMemset(a.dst, 0, (size_t)text_bytes));      // (a refused member's piece: zeros, not what the memory held)
	a.src = d_src; a.src_bytes = src_bytes; a.member_off = d_member; a.text_off = d_text; a.n_members = n_members; a.dst_capacity = text_bytes;
	HIP_TRY(launch_bgzf_inflate(a, n_cu, nullptr));
	if (text_bytes > 0) HIP_TRY(hipMemcpy(dst, a.dst, (size_t)text_bytes, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(status, a.status, 4 * (size_t)n_members, hipMemcpyDeviceToHost));
	return KG_OK;
}

struct kg_inflater {
	int device = 0, n_cu = 256;
	hipStream_t stream = nullptr;
	hipEvent_t ev[2] = {nullptr, nullptr};
	int64_t src_cap = 0, text_cap = 0, member_cap = 0;
	uint8_t *h_src = nullptr, *d_src = nullptr, *h_text = nullptr, *d_text = nullptr;
	int64_t *h_off = nullptr, *d_off = nullptr;      // member_off [member_cap + 1], text_off behind it
	int32_t *h_status = nullptr, *d_status = nullptr;
};

namespace {

void inflater_release(kg_inflater *k, bool src, bool text, bool members)
{
	if (src) { (void)hipHostFree(k->h_src); (void)hipFree(k->d_src); k->h_src = k->d_src = nullptr; k->src_cap = 0; }
	if (text) { (void)hipHostFree(k->h_text); (void)hipFree(k->d_text); k->h_text = k->d_text = nullptr; k->text_cap = 0; }
	if (members) {
		(void)hipHostFree(k->h_off); (void)hipFree(k->d_off); (void)hipHostFree(k->h_status); (void)hipFree(k->d_status);
		k->h_off = k->d_off = nullptr; k->h_status = k->d_status = nullptr; k->member_cap = 0;
	}
}

}  // namespace

extern "C" int kg_inflater_reserve(kg_inflater *k, int64_t src_bytes, int64_t text_bytes, int64_t members)
{
	if (!k || src_bytes < 0 || text_bytes < 0 || members < 0 || members > INT32_MAX - 1) return fail(KG_ERR_ARG, "kg_inflater_reserve: bad argument");
	HIP_TRY(hipSetDevice(k->device));
	if (src_bytes > k->src_cap || text_bytes > k->text_cap || members > k->member_cap) HIP_TRY(hipStreamSynchronize(k->stream));
	if (src_bytes > k->src_cap) {
		// (the caller may be in the middle of reading a round into it: what it holds moves along, and a failure leaves it as it was)
		const int64_t cap = src_bytes + src_bytes / 4;
		uint8_t *h = nullptr, *d = nullptr;
		HIP_TRY(hipHostMalloc((void **)&h, (size_t)std::max<int64_t>(cap, 16), hipHostMallocDefault));
		hipError_t e = hipMalloc((void **)&d, (size_t)std::max<int64_t>(cap, 16));
		if (e != hipSuccess) { (void)hipHostFree(h); HIP_TRY(e); }
		if (k->src_cap > 0) memcpy(h, k->h_src, (size_t)k->src_cap);
		inflater_release(k, true, false, false);
		k->h_src = h; k->d_src = d; k->src_cap = cap;
	}
	if (text_bytes > k->text_cap) {
		inflater_release(k, false, true, false);
		const int64_t cap = text_bytes + text_bytes / 4;
		HIP_TRY(hipHostMalloc((void **)&k->h_text, (size_t)std::max<int64_t>(cap, 16), hipHostMallocDefault));
		HIP_TRY(hipMalloc((void **)&k->d_text, (size_t)std::max<int64_t>(cap, 16)));
		k->text_cap = cap;
	}
	if (members > k->member_cap) {
		inflater_release(k, false, false, true);
		const int64_t cap = members + members / 4;
		HIP_TRY(hipHostMalloc((void **)&k->h_off, 16 * (size_t)(cap + 1), hipHostMallocDefault));
		HIP_TRY(hipMalloc((void **)&k->d_off, 16 * (size_t)(cap + 1)));
		HIP_TRY(hipHostMalloc((void **)&k->h_status, 4 * (size_t)(cap + 1), hipHostMallocDefault));
		HIP_TRY(hipMalloc((void **)&k->d_status, 4 * (size_t)(cap + 1)));
		k->member_cap = cap;
	}
	return KG_OK;
}

extern "C" int kg_inflater_create(int device, int64_t max_src_bytes, int64_t max_text_bytes, int64_t max_members, kg_inflater **out)
{
	if (!out || max_src_bytes < 0 || max_text_bytes < 0 || max_members < 0) return fail(KG_ERR_ARG, "kg_inflater_create: bad argument");
	*out = nullptr;
	int n_cu = 0;
	if (int rc = device_cus("kg_inflater_create", device, n_cu)) return rc;
	kg_inflater *k = new kg_inflater;
	k->device = device; k->n_cu = n_cu;
	int rc = KG_OK;
	auto make = [&]() -> int {
		HIP_TRY(hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreate(&k->ev[0]));
		HIP_TRY(hipEventCreate(&k->ev[1]));
		return kg_inflater_reserve(k, max_src_bytes, max_text_bytes, max_members);
	};
	if ((rc = make()) != KG_OK) { kg_inflater_destroy(k); return rc; }
	*out = k;
	return KG_OK;
}

extern "C" uint8_t *kg_inflater_src(kg_inflater *k) { return k ? k->h_src : nullptr; }

extern "C" int kg_inflater_run(kg_inflater *k, int64_t src_bytes, const int64_t *member_off, const int64_t *text_off, int64_t n_members,
                               const uint8_t **text, const int32_t **status, double *device_ms)
{
	if (!k || !text || !status) return fail(KG_ERR_ARG, "kg_inflater_run: bad argument");
	if (int rc = check_members("kg_inflater_run", src_bytes, member_off, text_off, n_members, k->text_cap)) return rc;
	if (src_bytes > k->src_cap) return fail(KG_ERR_CAPACITY, "kg_inflater_run: the members take %lld bytes, the inflater holds %lld", (long long)src_bytes, (long long)k->src_cap);
	if (n_members > k->member_cap) return fail(KG_ERR_CAPACITY, "kg_inflater_run: %lld members, the inflater holds %lld", (long long)n_members, (long long)k->member_cap);
	*text = k->h_text; *status = k->h_status;
	if (device_ms) *device_ms = 0;
	if (n_members == 0) return KG_OK;
	HIP_TRY(hipSetDevice(k->device));
	const int64_t text_bytes = text_off[n_members];
	const size_t table = (size_t)(n_members + 1);
	memcpy(k->h_off, member_off, 8 * table);
	memcpy(k->h_off + table, text_off, 8 * table);
	if (src_bytes > 0) HIP_TRY(hipMemcpyAsync(k->d_src, k->h_src, (size_t)src_bytes, hipMemcpyHostToDevice, k->stream));
	HIP_TRY(hipMemcpyAsync(k->d_off, k->h_off, 16 * table, hipMemcpyHostToDevice, k->stream));
	BgzfInflateArgs a{};
	a.src = k->d_src; a.src_bytes = src_bytes; a.member_off = k->d_off; a.text_off = k->d_off + table; a.n_members = n_members;
	a.dst = k->d_text; a.dst_capacity = text_bytes; a.status = k->d_status;
	HIP_TRY(hipEventRecord(k->ev[0], k->stream));
	HIP_TRY(launch_bgzf_inflate(a, k->n_cu, k->stream));
	HIP_TRY(hipEventRecord(k->ev[1], k->stream));
	if (text_bytes > 0) HIP_TRY(hipMemcpyAsync(k->h_text, k->d_text, (size_t)text_bytes, hipMemcpyDeviceToHost, k->stream));
	HIP_TRY(hipMemcpyAsync(k->h_status, k->d_status, 4 * (size_t)n_members, hipMemcpyDeviceToHost, k->stream));
	HIP_TRY(hipStreamSynchronize(k->stream));
	float ms = 0;
	if (device_ms && hipEventElapsedTime(&ms, k->ev[0], k->ev[1]) == hipSuccess) *device_ms = (double)ms;
	return KG_OK;
}

extern "C" void kg_inflater_destroy(kg_inflater *k)
{
	if (!k) return;
	(void)hipSetDevice(k->device);
	if (k->stream) (void)hipStreamSynchronize(k->stream);
	inflater_release(k, true, true, true);
	for (hipEvent_t e : k->ev)
		if (e) (void)hipEventDestroy(e);
	if (k->stream) (void)hipStreamDestroy(k->stream);
	delete k;
}
