// un_kernels.hip -- the unmapped reads of a batch, written back as the FASTQ / FASTA text they came as, on the device (gfx950; kg_stream_set_unmapped).
//
//   un_size_kernel      one lane per unit (a read, or a pair): is it selected -- every read of it has the unmapped record with FLAG & 4; a pair the device
//                       handed back (KG_ALN_HOST) is the caller's to decide -- and how many bytes its records take in either file -> scan -> offsets
//   un_copy_kernel      one wave per 64 units and file: the selected spans as ONE list of 16-byte chunks, lane l taking chunks l, l + 64, ... (text_device.hpp,
//                       as sam_format_kernel's phase 2b): consecutive lanes move consecutive chunks, whole memory lines per instruction on either side.  In an
//                       ordinary run almost nothing is selected: a group whose offsets do not move leaves after two loads.
// Byte work, HBM-bound: a selected byte is read once and written once.  Plain C++, vector loads and stores only.
#include "un_kernels.hpp"
#include "text_device.hpp"

namespace kg {

namespace {

// where the records of unit u lie in file f: text[from, to), and whether the file's last line ends there without a line feed
struct UnSpan {
	uint32_t from, to;
	int add_lf;
};

// the end of record j of window w: one past the last line GetNextEntry took for it
__device__ __forceinline__ uint32_t record_end(const FqWindow &w, bool fasta, int64_t j)
{
	// (FASTA: the line in front of the next record's header line, or the window's last line -- fa_head_kernel's rec_line[recs] is the number of lines)
	const int64_t last = fasta ? (int64_t)w.rec_line[j + 1] - 1 : 4 * j + 3;
	return last >= 0 && last < w.line_capacity ? w.line_end[last] : 0u;       // (0: no span, which the caller counts as an error)
}

__device__ __forceinline__ UnSpan unit_span(const UnArgs &a, int f, int64_t u)
{
	const FqWindow &w = a.w[f];
	// two files: record u of either; one file: records 2u and 2u + 1 of a pair follow each other, else record u
	const int64_t j0 = a.two_files || !a.paired ? u : 2 * u, j1 = a.two_files || !a.paired ? u : 2 * u + 1;
	UnSpan s;
	s.from = w.rec_hdr[j0];
	s.to = record_end(w, a.fasta != 0, j1);
	s.add_lf = (w.eof && (int64_t)s.to == w.end && s.to > s.from && w.text[s.to - 1] != '\n') ? 1 : 0;
	return s;
}

__device__ __forceinline__ bool read_unmapped(const kg_aln_record &rec) { return rec.kind == KG_ALN_UNMAPPED && (rec.flag & 4) != 0; }

}  // namespace

__global__ __launch_bounds__(256) void un_size_kernel(UnArgs a)
{
	const int nf = a.two_files ? 2 : 1;
	for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += (int64_t)gridDim.x * blockDim.x) {
		bool take;
		if (a.paired) {
			const kg_aln_record &r1 = a.records[2 * u], &r2 = a.records[2 * u + 1];
			take = read_unmapped(r1) && read_unmapped(r2);          // (a pair handed back is KG_ALN_HOST on both reads: not taken here)
		} else take = read_unmapped(a.records[u]);
		for (int f = 0; f < nf; ++f) {
			int n = 0;
			if (take) {
				const UnSpan s = unit_span(a, f, u);
				// (a span is a few lines of a window of less than 4 GB: anything else is a table this kernel does not understand, and nothing is taken)
				const bool sound = s.to > s.from && (int64_t)s.from >= a.w[f].begin && (int64_t)s.to <= a.w[f].end && s.to - s.from < (1u << 30);
				if (sound) n = (int)(s.to - s.from) + s.add_lf;
				else atomicAdd(&a.ctl[2], 1ull);
			}
			a.un_len[f][u] = n;
		}
	}
	if (blockIdx.x == 0 && threadIdx.x == 0)
		for (int f = 0; f < nf; ++f) a.un_len[f][a.n_units] = 0;
}

__global__ void un_reset_kernel(UnArgs a)
{
	if (threadIdx.x < 4) a.ctl[threadIdx.x] = 0;
}

// grid.y = file.  One wave per 64 consecutive units
__global__ __launch_bounds__(64) void un_copy_kernel(UnArgs a)
{
	__shared__ uint32_t src_at[64];       // where unit i's span starts in the window
	__shared__ int64_t dst_at[64];        // ... and where it goes
	__shared__ int span_n[64];            // bytes to move (the added line feed not among them)
	__shared__ int chunk_pre[65];         // chunks of the units before unit i
	const int f = blockIdx.y;
	const int lane = threadIdx.x;
	const FqWindow &w = a.w[f];
	const int64_t *off = a.un_off[f];
	uint8_t *const out = a.un[f];
	const int64_t n_groups = (a.n_units + 63) >> 6;
	unsigned long long moved = 0;
	for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
		const int64_t u0 = g << 6, u1 = u0 + 64 < a.n_units ? u0 + 64 : a.n_units;
		// nothing selected among the 64: two loads, the same for every lane
		if (off[u0] == off[u1]) continue;
		// ---- lane = unit: its span -------------------------------------------------------------------------------------------------
		{
			const int64_t u = u0 + lane;
			int n = 0;
			if (u < u1) {
				const int64_t o0 = off[u], o1 = off[u + 1];
				if (o1 > o0) {
					const UnSpan s = unit_span(a, f, u);
					// (what un_size_kernel counted, and within the buffer: anything else is an error, and nothing is written for the unit)
					if ((int64_t)(s.to - s.from) + s.add_lf == o1 - o0 && o1 <= a.un_capacity[f]) {
						n = (int)(s.to - s.from);
						src_at[lane] = s.from;
						dst_at[lane] = o0;
						if (s.add_lf) { out[o1 - 1] = '\n'; moved += 1; }
					} else atomicAdd(&a.ctl[2], 1ull);
				}
			}
			span_n[lane] = n;
			chunk_list(chunk_pre, lane, (n + 15) >> 4);
		}
		__syncthreads();
		// ---- lane = chunk: sixteen bytes at a time, a span's last bytes one by one (the byte behind a span is another lane's) ---------------------
		for_each_chunk(chunk_pre, lane, [&](int unit, int c) {
			const int at = c << 4, n = span_n[unit];
			const uint8_t *src = w.text + src_at[unit] + at;
			uint8_t *dst = out + dst_at[unit] + at;
			if (at + 16 <= n) {
				*reinterpret_cast<U128 *>(dst) = *reinterpret_cast<const U128 *>(src);
				moved += 16;
			} else {
				for (int k = 0; k < n - at; ++k) dst[k] = src[k];
				moved += (unsigned long long)(n - at);
			}
		});
		__syncthreads();
	}
	// the bytes this wave wrote: the caller holds the sum against the scan's total
	for (int d = 32; d > 0; d >>= 1) moved += __shfl_down(moved, d);
	if (lane == 0 && moved) atomicAdd(&a.ctl[f], moved);
}

hipError_t launch_un_size(const UnArgs &a, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream)
{
	kt_begin(KT_UN_SIZE, stream);
	hipLaunchKernelGGL(un_reset_kernel, dim3(1), dim3(64), 0, stream, a);
	if (a.n_units > 0) hipLaunchKernelGGL(un_size_kernel, dim3(grid_of(a.n_units, 256, n_cu * 16)), dim3(256), 0, stream, a);
	for (int f = 0; f < (a.two_files ? 2 : 1); ++f) {
		const hipError_t e = scan_lengths(a.un_len[f], a.un_off[f], a.n_units + 1, scan_temp, scan_temp_bytes, stream);
		if (e != hipSuccess) return e;
	}
	kt_end(KT_UN_SIZE, stream);
	return hipGetLastError();
}

hipError_t launch_un_copy(const UnArgs &a, int n_cu, hipStream_t stream)
{
	if (a.n_units <= 0) return hipSuccess;
	kt_begin(KT_UN_COPY, stream);
	hipLaunchKernelGGL(un_copy_kernel, dim3(grid_of(a.n_units, 64, n_cu * 32), a.two_files ? 2 : 1), dim3(64), 0, stream, a);
	kt_end(KT_UN_COPY, stream);
	return hipGetLastError();
}

}  // namespace kg
