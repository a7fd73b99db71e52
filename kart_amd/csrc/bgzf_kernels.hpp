// bgzf_kernels.hpp -- a device byte buffer as BGZF blocks (SAMv1 4.1), compressed on the device (bgzf_kernels.hip).
//
// htslib -- and bgzf_append on the host (host/detail/bam.inc) -- cut the BAM stream into payloads of at most 0xff00 bytes and make an
// independent gzip member of each.  Here the same happens on the device: the caller names CUTS, byte offsets no block may straddle,
// every non-empty range between two neighbouring cuts is split into such payloads (plan), one workgroup deflates each
// (kernels/bgzf_block.inc) into a slot of its own, and the members are gathered back to back behind a scan of their sizes (pack).
// No reader needs the bytes zlib would have made, only the inflated stream; two calls on the same bytes give the same members.
#pragma once
#include "seed_kernels.hpp"

namespace kg {

constexpr int64_t kBgzfPayload = 0xff00;     // bytes of payload per block
constexpr int64_t kBgzfSlot = 65536;         // bytes of a member at most (BSIZE is 16 bits): the stride of the members' slots

// words of BgzfArgs::ctl
enum { BGZ_BLOCKS = 0, BGZ_BYTES = 1, BGZ_ERRORS = 2, BGZ_RUN = 3, BGZ_WORDS = 4 };

struct BgzfArgs {
	const uint8_t *src;
	int64_t src_bytes;
	const int64_t *cuts;           // [n_cuts] ascending, cuts[0] = 0, cuts[n_cuts - 1] = src_bytes; equal neighbours are an empty range: no block
	int64_t n_cuts;
	int64_t max_blocks;            // what the tables and `slots` hold
	int64_t *range_first;          // [n_cuts] blocks in front of every range (scratch)
	int64_t *block_src;            // [max_blocks + 1] block i holds src[block_src[i], block_src[i + 1])
	int32_t *block_bytes;          // [max_blocks + 1] size of member i (scratch)
	int64_t *block_off;            // [max_blocks + 1] member i lies at dst[block_off[i], block_off[i + 1])
	uint8_t *slots;                // [max_blocks * kBgzfSlot] the members before they are gathered (scratch)
	uint8_t *dst;
	int64_t dst_capacity;          // a member that would end behind it is not written
	unsigned long long *ctl;       // [BGZ_WORDS] BGZ_BLOCKS: blocks the cuts make (more than max_blocks: none was made), BGZ_BYTES: bytes of all
	                               // members, BGZ_ERRORS: members that missed the size computed for them (never seen), BGZ_RUN: blocks made
};

// blocks that `bytes` of payload with `ranges` non-empty ranges make at most
inline int64_t bgzf_max_blocks(int64_t bytes, int64_t ranges) { return bytes / kBgzfPayload + ranges + 1; }
size_t bgzf_scan_temp_bytes(int64_t max_items);      // the scans over n_cuts and max_blocks + 1 items
// plan, deflate, pack: everything on `stream`, no synchronisation.  Timed as KT_BGZF.
hipError_t launch_bgzf(const BgzfArgs &a, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream);
// The cuts of a stream batch (kg_stream_map, KG_STREAM_FORMAT_BAM_BGZF) from its record offsets: cuts[r], r = 0 .. n_reads, is the offset of the
// last read at or in front of r that begins a chunk of chunk_reads reads or was handed back (sam_off[r] == sam_off[r + 1]); cuts[n_reads] = the end
hipError_t launch_bgzf_stream_cuts(const int64_t *sam_off, int64_t n_reads, int chunk_reads, int64_t *cuts, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream);

// ---- the other way: BGZF members inflated on the device (kernels/bgzf_inflate.inc) ---------------------------------------------
// Member i is src[member_off[i], member_off[i + 1]) and becomes dst[text_off[i], text_off[i + 1]): one wave per member, which finds the deflate
// stream behind the member's gzip header itself and checks the trailer's CRC-32 and ISIZE.  status[i] is KG_INFLATE_* (include/kart_amd.h); a member
// whose ranges do not lie inside src / dst, or are longer than 64 KiB, is refused without a byte of it being read.
struct BgzfInflateArgs {
	const uint8_t *src;
	int64_t src_bytes;
	const int64_t *member_off;     // [n_members + 1]
	const int64_t *text_off;       // [n_members + 1]
	int64_t n_members;
	uint8_t *dst;
	int64_t dst_capacity;
	int32_t *status;               // [n_members]
};
// everything on `stream`, no synchronisation
hipError_t launch_bgzf_inflate(const BgzfInflateArgs &a, int n_cu, hipStream_t stream);

}  // namespace kg
