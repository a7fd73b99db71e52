// abi_stream.hip -- kg_stream_*: FASTQ or FASTA text in, SAM text (or BAM records, kg_stream_set_format) out (declared in include/kart_amd.h).
//
// One call chain per batch replaces what the reference's worker loop does for a chunk from GetNextChunk to the fprintf of its SAM
// lines (src/Mapping.cpp:488-637; src/GetData.cpp:109-143): the caller uploads the bytes of the input files as they lie there,
// and receives the text of the records.  A stream owns `lanes` independent lanes -- workspace, device text windows, page-locked
// staging and result buffers, one HIP stream each -- so that several batches are in flight on the device at once (the analogue of
// the reference's N workers each on their own chunk, src/Mapping.cpp:716-717).
#include "abi_internal.hpp"
#include "stream_kernels.hpp"
#include "un_kernels.hpp"
#include "stats_kernels.hpp"
#include "bgzf_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>

#define fail kg_fail

namespace {

// the words of a lane's page-locked scratch behind the parser's (Lane::h_meta + FQM_WORDS)
enum LaneWord {
	LW_TEXT_BYTES = 0,                                 // kg_stream_map: bytes of the batch's text
	LW_HOST_READS = 1,                                 // reads handed back
	LW_FORMAT_ERRORS = 2,                              // records formatted to a size other than the one announced
	LW_EXTRA_RECORDS = 3,                              // extra records of -m
	LW_ALN_COUNTS = 8,                                 // [8, 16) kg_stream_timing_t::aln_counts of the batch: the alignment stage's seven list sizes, of which ...
	LW_ALN_TRIVIAL = 14,                               // ... the last (the piece count, which nobody reads) gives way to the pairs aln_trivial_kernel decided,
	LW_ALN_GENERAL = 15,                               // and the candidates its fast plan kernel left to the general one
	LW_CHECKSUM = 16,                                  // [16, 18) sam_checksum_kernel's sums (KG_STREAM_CHECKSUM)
	LW_FETCH_SEEDS = 18,                               // [18, 20) kg_stream_fetch: the candidate seeds' offsets at either end of the reads asked for
	LW_BGZF = 20,                                      // [20, 24) KG_STREAM_FORMAT_BAM_BGZF: the BGZF launch's control words (BgzfArgs::ctl)
	LW_UN_BYTES = 24,                                  // [24, 26) kg_stream_set_unmapped: bytes of the selected units in either file (the scans' totals)
	LW_UN_CTL = 26,                                    // [26, 29) ... and UnArgs::ctl: the bytes un_copy_kernel wrote per file, spans it did not understand
	LW_WORDS = 32
};

struct Lane {
	kg_workspace *ws = nullptr;
	// device
	uint8_t *d_text[2] = {nullptr, nullptr};
	int32_t *d_tile[2] = {nullptr, nullptr};
	uint32_t *d_line_end[2] = {nullptr, nullptr};
	uint32_t *d_rec[2] = {nullptr, nullptr};           // six arrays of rec_capacity words: hdr, name, seq, qual, rlen, qlen
	uint64_t *d_line_acc[2] = {nullptr, nullptr};      // FASTA (allocated by the first kg_stream_set_input(FASTA)): [line_capacity + 1] per-line record / character counts
	uint32_t *d_rec_line[2] = {nullptr, nullptr};      // ... and [rec_capacity + 1] the header line of every record
	int64_t *d_meta = nullptr;
	int32_t *d_read_len = nullptr;
	void *d_scan = nullptr;
	size_t scan_bytes = 0;
	int32_t *d_sam_len = nullptr, *d_host_list = nullptr;
	int64_t *d_sam_off = nullptr;
	unsigned long long *d_sam_ctl = nullptr;
	uint8_t *d_sam = nullptr;
	int64_t d_sam_capacity = 0;
	// KG_STREAM_FORMAT_BAM_BGZF (bgzf_room: allocated by the first kg_stream_set_format that asks for it, grown by a batch that needs more)
	int64_t *d_cuts = nullptr, *d_range_first = nullptr;       // [max_reads + 8]
	int64_t *d_block_src = nullptr, *d_block_off = nullptr;    // [bgzf_blocks + 1]
	int32_t *d_block_bytes = nullptr;
	uint8_t *d_slots = nullptr, *d_bgzf = nullptr;             // bgzf_blocks slots of 64 KiB; the members gathered
	int64_t bgzf_blocks = 0, d_bgzf_capacity = 0;
	unsigned long long *d_bgzf_ctl = nullptr;
	void *d_bgzf_scan = nullptr;
	size_t bgzf_scan_bytes = 0;
	// kg_stream_set_unmapped: the tables come with the lane's first kg_stream_map under the setting, the text buffers with the first batch that selects
	// something, and grow with a batch that needs more (map_un_size / map_un_room)
	int32_t *d_un_len[2] = {nullptr, nullptr};                 // [max_reads + 8]
	int64_t *d_un_off[2] = {nullptr, nullptr};
	uint8_t *d_un[2] = {nullptr, nullptr};
	int64_t d_un_capacity[2] = {0, 0};
	unsigned long long *d_un_ctl = nullptr;
	int64_t *h_un_off[2] = {nullptr, nullptr};                 // page-locked
	uint8_t *h_un[2] = {nullptr, nullptr};
	int64_t h_un_capacity[2] = {0, 0};
	// kg_stream_set_stats: one row per chunk, on the device and page-locked; both come with the lane's first kg_stream_map under the setting and grow with a
	// batch of more chunks (map_tally)
	uint32_t *d_tally = nullptr, *h_tally = nullptr;
	int64_t tally_capacity = 0, h_tally_capacity = 0;          // chunks
	uint8_t *h_bgzf = nullptr;                                 // page-locked, as are the tables
	int64_t h_bgzf_capacity = 0;
	int64_t *h_block_src = nullptr, *h_block_off = nullptr;
	// page-locked
	char *h_text[2] = {nullptr, nullptr};
	int64_t *h_meta = nullptr;                         // [FQM_WORDS] the parser's plan + [LW_WORDS] what the batch's small copies land in (LaneWord)
	char *h_sam = nullptr;
	int64_t h_sam_capacity = 0;
	int64_t *h_sam_off = nullptr, *h_cand_off = nullptr;
	int32_t *h_host_list = nullptr;
	uint32_t *h_rec_hdr[2] = {nullptr, nullptr};
	kg_aln_record *h_records = nullptr;
	int64_t record_capacity = 0;
	kg_chunk_stats *h_chunk_stats = nullptr;
	int64_t chunk_capacity = 0;
	kg_candidate *h_cands = nullptr;
	kg_seed *h_cand_seeds = nullptr;
	int64_t h_cand_capacity = 0;
	unsigned long long *h_ctl = nullptr;               // [kCtlWords] the search kernel's counters of the batch
	// the batch in the lane
	int64_t mapped_reads = 0;                          // reads of the batch the last kg_stream_map call mapped (still resident: kg_stream_fetch)
	const kg_aln_record *d_records = nullptr;          // ... and where its records lie
	kg_stream_window win{};
	kg_stream_parsed parsed{};
	bool have_batch = false;
	bool fasta = false;                                // the lane's parsed batch came from FASTA text (no qualities)
	hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	hipEvent_t ev_parsed = nullptr;                    // the batch is materialised and published to its group (recorded on the lane's stream)
};

// ONE seeding launch over the parsed batches of `size` lanes (kg_stream_config::seed_group).  The reference's analogue is simply N
// workers on N chunks (src/Mapping.cpp:716-717); on the device a search launch costs ~0.65 ms + 0.52 ms per M reads -- at 2.5 reads
// per persistent lane a launch lasts as long as its slowest lanes -- so four lanes' 1 M-read batches in one launch cost what 1.6 of
// them cost alone, while chaining, the report and the text keep the lanes' granularity.
// Lanes [first, first + size) share the group: its workspace holds `size` segments of `stride` read slots; lane j materialises its
// reads straight into segment j of the group's character array and publishes offsets / lengths of its slots (group_publish_kernel).
// A ROUND: every lane of the group either arrives with a parsed batch (kg_stream_map) or is absent (kg_stream_group_absent); the
// thread that completes the round launches the seeding of all segments on the group's stream, waits for it and wakes the others;
// each lane then cuts its seeds out of the group's arrays on its own stream.  A lane can only arrive again after it has finished
// with the group's arrays, so the next round never overwrites what a slow lane still reads.
struct SeedGroup {
	int first = 0, size = 0;
	int64_t stride = 0, seg_bases = 0;
	kg_workspace *ws = nullptr;                        // the group's workspace (hits, packed reads, seeds of all segments)
	unsigned long long *h_ctl = nullptr;               // page-locked: the search kernel's counters of the round
	std::mutex mu;
	std::condition_variable cv;
	int64_t round = 0;
	int arrived = 0;
	bool present[kMaxSeedSegments] = {false};
	int absent_rounds[kMaxSeedSegments] = {0};         // 0: the lane takes part; > 0: absent for that many rounds; < 0: until further notice
	int64_t n_reads[kMaxSeedSegments] = {0};
	// results of the last round
	int rc = KG_OK;
	int64_t seed_base[kMaxSeedSegments + 1] = {0};
	bool aborted = false;
	// After the round the lanes run their own stages (chaining .. text) ONE AFTER THE OTHER, in lane order: started all at once they
	// share the device, all finish late and together, and the caller's writer -- which takes the batches in order -- first starves and
	// is then handed four batches at once (measured, 100 M reads: 27.6-28.4 M reads/s against 29.0-29.9 M with independent lanes).
	// A lane keeps the turn until its batch is back on the host (kg_stream_map's last sync).
	int order[kMaxSeedSegments] = {0};
	int n_order = 0, turn = 0;
};

// the turn of lane j of a group at its own stages (see SeedGroup::order); released by hand once, or by the destructor on an error path
struct GroupTurn {
	SeedGroup *sg = nullptr;
	bool held = false;
	bool acquire(SeedGroup &g, int j)
	{
		sg = &g;
		std::unique_lock<std::mutex> lk(g.mu);
		g.cv.wait(lk, [&]() { return g.aborted || (g.turn < g.n_order && g.order[g.turn] == j); });
		held = !g.aborted;
		return held;
	}
	void release()
	{
		if (!held) return;
		held = false;
		std::lock_guard<std::mutex> lk(sg->mu);
		sg->turn++;
		sg->cv.notify_all();
	}
	~GroupTurn() { release(); }
};

}  // namespace

struct kg_stream {
	kg_index *ix = nullptr;
	kg_stream_config cfg{};
	int64_t text_capacity = 0, line_capacity = 0, rec_capacity = 0;
	std::vector<Lane> lanes;
	std::vector<std::unique_ptr<SeedGroup>> groups;    // empty: every lane seeds its own batch
	uint8_t *d_chr_names = nullptr;
	int32_t *d_chr_name_off = nullptr;
	int min_seed_len = 13;
	int format = KG_STREAM_FORMAT_SAM;                 // what kg_stream_map makes of the records (kg_stream_set_format)
	int input = KG_STREAM_INPUT_FASTQ;                 // what kg_stream_parse takes the text for (kg_stream_set_input)
	int tags = 0;                                      // KG_STREAM_TAG_*: the optional fields beyond NM / AS / XS (kg_stream_set_tags)
	bool unmapped = false;                             // kg_stream_map hands the unmapped units' input text back (kg_stream_set_unmapped)
	bool stats = false;                                // kg_stream_map tallies the batch's records per chunk (kg_stream_set_stats)
	// the read group every record carries (kg_stream_set_read_group), in the two forms the kernels copy: "\tRG:Z:<ID>" at d_rg (6 + rg_len bytes) and
	// 'R' 'G' 'Z' <ID> NUL at d_rg + kRgBamAt (4 + rg_len bytes); rg_len 0: none
	uint8_t *d_rg = nullptr;
	int rg_len = 0;
	bool fasta_sized = false;                          // the record tables hold line_capacity / 2 records (a FASTA record can be two lines) and the FASTA arrays exist
	std::mutex mu;
	kg_stream_timing_t total{};
};

namespace {

void free_lane(Lane &l)
{
	if (l.ws && l.ws->enc_borrowed) l.ws->d_enc = nullptr;        // (a part of its group's array)
	if (l.ev_parsed) (void)hipEventDestroy(l.ev_parsed);
	if (l.ws) kg_workspace_destroy(l.ws);
	for (int f = 0; f < 2; ++f) {
		if (l.d_text[f]) (void)hipFree(l.d_text[f]);
		if (l.d_tile[f]) (void)hipFree(l.d_tile[f]);
		if (l.d_line_end[f]) (void)hipFree(l.d_line_end[f]);
		if (l.d_rec[f]) (void)hipFree(l.d_rec[f]);
		if (l.d_line_acc[f]) (void)hipFree(l.d_line_acc[f]);
		if (l.d_rec_line[f]) (void)hipFree(l.d_rec_line[f]);
		if (l.h_text[f]) (void)hipHostFree(l.h_text[f]);
		if (l.h_rec_hdr[f]) (void)hipHostFree(l.h_rec_hdr[f]);
		for (void *p : {(void *)l.d_un_len[f], (void *)l.d_un_off[f], (void *)l.d_un[f]})
			if (p) (void)hipFree(p);
		for (void *p : {(void *)l.h_un_off[f], (void *)l.h_un[f]})
			if (p) (void)hipHostFree(p);
	}
	if (l.d_un_ctl) (void)hipFree(l.d_un_ctl);
	if (l.d_tally) (void)hipFree(l.d_tally);
	if (l.h_tally) (void)hipHostFree(l.h_tally);
	for (void *p : {(void *)l.d_meta, (void *)l.d_read_len, l.d_scan, (void *)l.d_sam_len, (void *)l.d_host_list, (void *)l.d_sam_off, (void *)l.d_sam_ctl, (void *)l.d_sam,
	                (void *)l.d_cuts, (void *)l.d_range_first, (void *)l.d_block_src, (void *)l.d_block_off, (void *)l.d_block_bytes, (void *)l.d_slots, (void *)l.d_bgzf,
	                (void *)l.d_bgzf_ctl, l.d_bgzf_scan})
		if (p) (void)hipFree(p);
	for (void *p : {(void *)l.h_meta, (void *)l.h_sam, (void *)l.h_sam_off, (void *)l.h_cand_off, (void *)l.h_host_list, (void *)l.h_records, (void *)l.h_chunk_stats,
	                (void *)l.h_cands, (void *)l.h_cand_seeds, (void *)l.h_ctl, (void *)l.h_bgzf, (void *)l.h_block_src, (void *)l.h_block_off})
		if (p) (void)hipHostFree(p);
	for (hipEvent_t e : l.ev)
		if (e) (void)hipEventDestroy(e);
	l = Lane();
}

FqWindow window_of(const kg_stream *s, const Lane &l, int f)
{
	FqWindow w;
	w.text = l.d_text[f];
	w.begin = l.win.begin[f]; w.end = l.win.end[f]; w.eof = l.win.eof[f];
	w.tile_lines = l.d_tile[f];
	w.line_end = l.d_line_end[f];
	w.line_capacity = s->line_capacity;
	uint32_t *r = l.d_rec[f];
	const size_t c = (size_t)s->rec_capacity;
	w.rec_hdr = r; w.rec_name = r + c; w.rec_seq = r + 2 * c; w.rec_qual = r + 3 * c;
	w.rec_rlen = (int32_t *)(r + 4 * c); w.rec_qlen = (int32_t *)(r + 5 * c);
	w.rec_capacity = s->rec_capacity;
	w.line_acc = l.d_line_acc[f]; w.rec_line = l.d_rec_line[f];
	return w;
}

// bytes of a lane's output buffer.  SAM: a batch's input bytes and a little more per read (FLAG .. TLEN and the tags against '+' and the mate
// suffix).  BAM: a record of a very short read is larger than its line -- 36 bytes of core, four per CIGAR operation and up to 21 of tags against a
// few characters of text; over its FASTQ record (name + 2 L + 6 bytes) a record of L bases gains 52 + min(96, 4 L) - L / 2 <= 136 bytes.
int64_t out_capacity(const kg_stream_config &cfg, int format)
{
	return 2 * cfg.max_window + (format != KG_STREAM_FORMAT_SAM ? 144 : 64) * cfg.max_reads + 4096;
}

// kg_stream::d_rg: the BAM form lies at this offset; behind either form there are 16 readable bytes (the kernels copy 16 bytes at a time)
constexpr int kRgMaxId = 255, kRgBamAt = 512, kRgBytes = 1024;
static_assert(6 + kRgMaxId + 16 <= kRgBamAt && kRgBamAt + 4 + kRgMaxId + 16 <= kRgBytes, "both forms of the longest ID and their slack must fit");

// ... with the optional fields: MD:Z of an ordinary record is a number or a few ("\tMD:Z:150": 10 bytes); a batch whose records need more grows the
// buffers in kg_stream_map.  The read group reserves nothing here: see kg_stream_set_read_group
int64_t out_capacity(const kg_stream_config &cfg, int format, int tags)
{
	return out_capacity(cfg, format) + ((tags & KG_STREAM_TAG_MD) ? 32 : 0) * cfg.max_reads;
}

// A buffer that has to hold more: a new one of `bytes` in its place (nobody needs what the old one holds).  The caller synchronises the lane's
// stream first where the device may still use the old one, and keeps the capacity beside it.  kAllocFirst: the old buffer stays until the new one
// exists, so that a failure leaves it usable.
enum GrowOrder { kFreeFirst, kAllocFirst };
template <class T> hipError_t grow_device(T *&p, size_t bytes, GrowOrder order = kFreeFirst)
{
	T *old = p;
	if (order == kFreeFirst) {
		if (old) { hipError_t e = hipFree(old); if (e != hipSuccess) return e; }
		p = old = nullptr;
	}
	T *fresh = nullptr;
	hipError_t e = hipMalloc((void **)&fresh, bytes);
	if (e != hipSuccess) return e;
	if (old) (void)hipFree(old);
	p = fresh;
	return hipSuccess;
}
template <class T> hipError_t grow_pinned(T *&p, size_t bytes)
{
	if (p) { hipError_t e = hipHostFree(p); if (e != hipSuccess) return e; }
	p = nullptr;
	return hipHostMalloc((void **)&p, bytes, hipHostMallocDefault);
}

// what a search launch over `reads` reads fetched, from the kernel's own counters `c` (those kg_workspace_traffic exports)
double search_useful_bytes(const kg_index *ix, const unsigned long long *c, int64_t reads)
{
	const double sa_bytes = ix->view.fsa32 ? 4.0 : 8.0;
	return 8.0 * (double)c[17] + 32.0 * (double)c[18] + (double)c[25] + sa_bytes * (double)c[8] + 48.0 * (double)c[20] + 8.0 * (double)c[21] + 20.0 * (double)reads + 32.0 * (double)c[1];
}

// ... with the capacity kept beside the buffer: unchanged while the old buffer is still there, zero while there is none
template <class T, class C> hipError_t grow_device(T *&p, C &capacity, C want, size_t bytes)
{
	hipError_t e = grow_device(p, bytes);
	capacity = e == hipSuccess ? want : p ? capacity : 0;
	return e;
}
template <class T, class C> hipError_t grow_pinned(T *&p, C &capacity, C want, size_t bytes)
{
	hipError_t e = grow_pinned(p, bytes);
	capacity = e == hipSuccess ? want : p ? capacity : 0;
	return e;
}

// (sg.mu held) every lane of the group has arrived with a batch or sits the round out
bool round_complete(const SeedGroup &sg)
{
	int accounted = sg.arrived;
	for (int i = 0; i < sg.size; ++i) accounted += (!sg.present[i] && sg.absent_rounds[i] != 0) ? 1 : 0;
	return accounted >= sg.size;
}

float elapsed(hipEvent_t a, hipEvent_t b)
{
	float ms = 0;
	if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return ms;
}

}  // namespace

extern "C" {

int kg_stream_open(kg_index *ix, const kg_stream_config *cfg, kg_stream **out)
{
	if (!ix || !cfg || !out) return fail(KG_ERR_ARG, "kg_stream_open: null argument");
	*out = nullptr;
	if (cfg->lanes < 1 || cfg->lanes > 16 || cfg->max_reads < 2 || cfg->max_window < 4096 || cfg->max_window > 0xF0000000ll)
		return fail(KG_ERR_ARG, "kg_stream_open: bad configuration (%d lanes, %lld reads, %lld bytes per window)", cfg->lanes, (long long)cfg->max_reads, (long long)cfg->max_window);
	const int group = cfg->seed_group > 1 ? cfg->seed_group : 0;
	if (group && (group > kMaxSeedSegments || cfg->lanes % group != 0))
		return fail(KG_ERR_ARG, "kg_stream_open: seed_group %d must divide the %d lanes and be at most %d", group, cfg->lanes, kMaxSeedSegments);
	if (!ix->d_text) return fail(KG_ERR_ARG, "kg_stream_open: the index holds no text");
	HIP_TRY(hipSetDevice(ix->device));
	std::unique_ptr<kg_stream, void (*)(kg_stream *)> s(new kg_stream(), kg_stream_close);
	s->ix = ix;
	s->cfg = *cfg;
	s->text_capacity = (cfg->max_window + 4096 + 255) & ~255ll;
	// a line of FASTQ text is rarely shorter than 16 bytes on average (header, sequence, '+', qualities); a window with more lines
	// than this goes back to the caller's reader (FQ_STOP_IRREGULAR)
	s->line_capacity = cfg->max_window / 16 + 4096;
	s->rec_capacity = s->line_capacity / 4 + 1;
	{
		kg_index_info_t info;
		kg_index_info(ix, &info);
		s->min_seed_len = info.min_seed_len;
		std::vector<int32_t> off{0};
		std::string names;
		for (const ContigRec &c : ix->contigs) { names += c.name; off.push_back((int32_t)names.size()); }
		HIP_TRY(hipMalloc((void **)&s->d_chr_names, names.size() + 16));
		HIP_TRY(hipMalloc((void **)&s->d_chr_name_off, 4 * off.size()));
		HIP_TRY(hipMemcpy(s->d_chr_names, names.data(), names.size(), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(s->d_chr_name_off, off.data(), 4 * off.size(), hipMemcpyHostToDevice));
		HIP_TRY(hipMalloc((void **)&s->d_rg, kRgBytes));
		HIP_TRY(hipMemset(s->d_rg, 0, kRgBytes));
	}
	s->lanes.resize((size_t)cfg->lanes);
	const int64_t n = cfg->max_reads;
	const int64_t seg_bases = (cfg->max_window + 4096 + 64 + 255) & ~255ll;      // a lane's part of its group's character array
	for (int g = 0; group && g < cfg->lanes / group; ++g) {
		// (in the stream's list at once: whatever fails below, kg_stream_close frees what the group holds -- ADVICE r4: a group that failed half-way
		//  used to keep its multi-GB arrays, and the host path the caller falls back to then ran out of device memory)
		s->groups.push_back(std::unique_ptr<SeedGroup>(new SeedGroup()));
		SeedGroup *sg = s->groups.back().get();
		sg->first = g * group; sg->size = group;
		sg->stride = n + 8; sg->seg_bases = seg_bases;
		int rc = kg_workspace_create(ix, sg->stride * group, seg_bases * group, &sg->ws);
		if (rc != KG_OK) return rc;
		kg_workspace *gw = sg->ws;
		HIP_TRY(hipMalloc((void **)&gw->d_enc, (size_t)gw->max_bases + 64));
		HIP_TRY(hipMalloc((void **)&gw->d_read_off, 8 * (size_t)(gw->max_reads + 1)));
		HIP_TRY(hipMalloc((void **)&gw->d_seed_off, 8 * (size_t)(gw->max_reads + 1)));
		HIP_TRY(hipMalloc((void **)&gw->group_read_len, 4 * (size_t)(gw->max_reads + 1)));
		HIP_TRY(hipMemsetAsync(gw->d_enc, 'N', (size_t)gw->max_bases + 64, gw->stream));
		HIP_TRY(hipMemsetAsync(gw->d_read_off, 0, 8 * (size_t)(gw->max_reads + 1), gw->stream));
		HIP_TRY(hipMemsetAsync(gw->group_read_len, 0, 4 * (size_t)(gw->max_reads + 1), gw->stream));
		HIP_TRY(hipStreamSynchronize(gw->stream));          // (the lanes write these arrays from their own streams)
		HIP_TRY(hipHostMalloc((void **)&sg->h_ctl, 8 * kCtlWords, hipHostMallocDefault));
		(void)kg_workspace_set_profiling(gw, 1);
	}
	for (size_t li = 0; li < s->lanes.size(); ++li) {
		Lane &l = s->lanes[li];
		// bases of a batch: what two windows can hold (every read costs its characters twice plus a header)
		int rc = kg_workspace_create(ix, n + 8, cfg->max_window + 4096, &l.ws);
		if (rc != KG_OK) return rc;
		kg_workspace *ws = l.ws;
		if (group) {
			SeedGroup &sg = *s->groups[li / (size_t)group];
			ws->d_enc = sg.ws->d_enc + (int64_t)(li % (size_t)group) * sg.seg_bases;
			ws->enc_borrowed = true;
			HIP_TRY(hipEventCreateWithFlags(&l.ev_parsed, hipEventDisableTiming));
		} else
		HIP_TRY(hipMalloc((void **)&ws->d_enc, (size_t)ws->max_bases + 64));
		HIP_TRY(hipMalloc((void **)&ws->d_read_off, 8 * (size_t)(ws->max_reads + 1)));
		HIP_TRY(hipMalloc((void **)&ws->d_seed_off, 8 * (size_t)(ws->max_reads + 1)));
		(void)kg_workspace_set_profiling(ws, 1);
		const int64_t n_tiles = s->text_capacity / kFqTile + 2;
		for (int f = 0; f < 2; ++f) {
			HIP_TRY(hipMalloc((void **)&l.d_text[f], (size_t)s->text_capacity));
			HIP_TRY(hipMalloc((void **)&l.d_tile[f], 4 * (size_t)(n_tiles + 1)));
			HIP_TRY(hipMalloc((void **)&l.d_line_end[f], 4 * (size_t)s->line_capacity));
			HIP_TRY(hipMalloc((void **)&l.d_rec[f], 4 * 6 * (size_t)s->rec_capacity));
			HIP_TRY(hipHostMalloc((void **)&l.h_text[f], (size_t)s->text_capacity, hipHostMallocDefault));
			HIP_TRY(hipHostMalloc((void **)&l.h_rec_hdr[f], 4 * (size_t)(n + 8), hipHostMallocDefault));
		}
		HIP_TRY(hipMalloc((void **)&l.d_meta, 8 * FQM_WORDS));
		HIP_TRY(hipMalloc((void **)&l.d_read_len, 4 * (size_t)(n + 8)));
		l.scan_bytes = fq_scan_temp_bytes(std::max<int64_t>(n + 8, n_tiles + 1));
		HIP_TRY(hipMalloc(&l.d_scan, l.scan_bytes ? l.scan_bytes : 256));
		HIP_TRY(hipMalloc((void **)&l.d_sam_len, 4 * (size_t)(n + 8)));
		HIP_TRY(hipMalloc((void **)&l.d_host_list, 4 * (size_t)(n + 8)));
		HIP_TRY(hipMalloc((void **)&l.d_sam_off, 8 * (size_t)(n + 8)));
		HIP_TRY(hipMalloc((void **)&l.d_sam_ctl, 8 * 4));
		HIP_TRY(hipHostMalloc((void **)&l.h_meta, 8 * (FQM_WORDS + LW_WORDS), hipHostMallocDefault));
		HIP_TRY(hipHostMalloc((void **)&l.h_sam_off, 8 * (size_t)(n + 8), hipHostMallocDefault));
		HIP_TRY(hipHostMalloc((void **)&l.h_cand_off, 8 * (size_t)(n + 8), hipHostMallocDefault));
		HIP_TRY(hipHostMalloc((void **)&l.h_host_list, 4 * (size_t)(n + 8), hipHostMallocDefault));
		HIP_TRY(hipHostMalloc((void **)&l.h_ctl, 8 * kCtlWords, hipHostMallocDefault));
		l.d_sam_capacity = out_capacity(*cfg, KG_STREAM_FORMAT_SAM);
		HIP_TRY(hipMalloc((void **)&l.d_sam, (size_t)l.d_sam_capacity));
		l.h_sam_capacity = l.d_sam_capacity;
		HIP_TRY(hipHostMalloc((void **)&l.h_sam, (size_t)l.h_sam_capacity, hipHostMallocDefault));
		l.record_capacity = n + n / 4 + 4096;
		HIP_TRY(hipHostMalloc((void **)&l.h_records, sizeof(kg_aln_record) * (size_t)l.record_capacity, hipHostMallocDefault));
		for (hipEvent_t &e : l.ev) HIP_TRY(hipEventCreate(&e));
	}
	HIP_TRY(hipDeviceSynchronize());                     // everything above has landed before a lane's first batch
	*out = s.release();
	return KG_OK;
}

void kg_stream_close(kg_stream *s)
{
	if (!s) return;
	(void)hipSetDevice(s->ix->device);
	for (Lane &l : s->lanes) free_lane(l);
	for (std::unique_ptr<SeedGroup> &sg : s->groups) {
		if (sg->ws && sg->ws->group_read_len) { (void)hipFree(sg->ws->group_read_len); sg->ws->group_read_len = nullptr; }
		if (sg->ws) kg_workspace_destroy(sg->ws);
		if (sg->h_ctl) (void)hipHostFree(sg->h_ctl);
	}
	if (s->d_chr_names) (void)hipFree(s->d_chr_names);
	if (s->d_chr_name_off) (void)hipFree(s->d_chr_name_off);
	if (s->d_rg) (void)hipFree(s->d_rg);
	delete s;
}

// KG_STREAM_FORMAT_BAM_BGZF: room in the lane for `blocks` BGZF blocks that hold `bytes` of records -- a slot per block, the gathered members (a stored
// member is its payload + 31 bytes) on the device, the tables, and a first page-locked buffer for the members.  Nothing of the lane's is in flight (the caller has synchronised).
static int bgzf_room(kg_stream *s, Lane &l, int64_t blocks, int64_t bytes)
{
	if (!l.d_cuts) {
		const size_t n = (size_t)s->cfg.max_reads + 8;
		HIP_TRY(hipMalloc((void **)&l.d_cuts, 8 * n));
		HIP_TRY(hipMalloc((void **)&l.d_range_first, 8 * n));
		HIP_TRY(hipMalloc((void **)&l.d_bgzf_ctl, 8 * BGZ_WORDS));
	}
	if (blocks > l.bgzf_blocks) {
		const int64_t want = blocks + blocks / 4 + 64;
		const size_t scan_bytes = bgzf_scan_temp_bytes(std::max<int64_t>(s->cfg.max_reads + 8, want + 1));
		l.bgzf_blocks = 0;
		HIP_TRY(grow_device(l.d_block_src, 8 * (size_t)(want + 1)));
		HIP_TRY(grow_device(l.d_block_off, 8 * (size_t)(want + 1)));
		HIP_TRY(grow_device(l.d_block_bytes, 4 * (size_t)(want + 1)));
		HIP_TRY(grow_device(l.d_slots, (size_t)(want * kBgzfSlot)));
		HIP_TRY(grow_device(l.d_bgzf_scan, scan_bytes ? scan_bytes : 256));
		HIP_TRY(grow_pinned(l.h_block_src, 8 * (size_t)(want + 1)));
		HIP_TRY(grow_pinned(l.h_block_off, 8 * (size_t)(want + 1)));
		l.bgzf_scan_bytes = scan_bytes;
		l.bgzf_blocks = want;
	}
	const int64_t room = bytes + 31 * blocks;
	if (room > l.d_bgzf_capacity) HIP_TRY(grow_device(l.d_bgzf, l.d_bgzf_capacity, room + room / 8, (size_t)(room + room / 8)));
	// (page-locked memory is the dearer kind: half of that to begin with -- BAM records deflate to a quarter -- and map_copy_out grows it for a batch whose
	//  blocks take more)
	if (!l.h_bgzf) HIP_TRY(grow_pinned(l.h_bgzf, l.h_bgzf_capacity, room / 2 + 4096, (size_t)(room / 2 + 4096)));
	return KG_OK;
}

// the lanes' output buffers, device and page-locked, hold `want` bytes (they only ever grow); nothing of a lane's is in flight afterwards
static int grow_output(kg_stream *s, int64_t want)
{
	for (Lane &l : s->lanes) {
		if (l.d_sam_capacity < want) {
			HIP_TRY(hipStreamSynchronize(l.ws->stream));
			HIP_TRY(grow_device(l.d_sam, l.d_sam_capacity, want, (size_t)want));
		}
		if (l.h_sam_capacity < want) {
			HIP_TRY(hipStreamSynchronize(l.ws->stream));
			HIP_TRY(grow_pinned(l.h_sam, l.h_sam_capacity, want, (size_t)want));
		}
	}
	return KG_OK;
}

int kg_stream_set_format(kg_stream *s, int format)
{
	if (!s) return fail(KG_ERR_ARG, "kg_stream_set_format: null stream");
	if (format != KG_STREAM_FORMAT_SAM && format != KG_STREAM_FORMAT_BAM && format != KG_STREAM_FORMAT_BAM_BGZF)
		return fail(KG_ERR_ARG, "kg_stream_set_format: unknown format %d (KG_STREAM_FORMAT_SAM, KG_STREAM_FORMAT_BAM or KG_STREAM_FORMAT_BAM_BGZF)", format);
	HIP_TRY(hipSetDevice(s->ix->device));
	// the lanes' output buffers hold a batch in the larger of the two formats from the first BAM run on
	const int64_t want = out_capacity(s->cfg, format, s->tags);
	{
		int rc = grow_output(s, want);
		if (rc != KG_OK) return rc;
	}
	for (Lane &l : s->lanes) {
		if (format == KG_STREAM_FORMAT_BAM_BGZF) {
			// (chunks of ReadChunkSize = 4000 reads and a read in a hundred handed back: a batch that cuts its records finer grows the tables)
			HIP_TRY(hipStreamSynchronize(l.ws->stream));
			int rc = bgzf_room(s, l, bgzf_max_blocks(want, s->cfg.max_reads / 4000 + s->cfg.max_reads / 100 + 1), want);
			if (rc != KG_OK) return rc;
		}
	}
	s->format = format;
	return KG_OK;
}

int kg_stream_set_tags(kg_stream *s, int tags)
{
	if (!s) return fail(KG_ERR_ARG, "kg_stream_set_tags: null stream");
	if (tags & ~KG_STREAM_TAG_MD) return fail(KG_ERR_ARG, "kg_stream_set_tags: unknown tags 0x%x (KG_STREAM_TAG_MD)", tags);
	HIP_TRY(hipSetDevice(s->ix->device));
	int rc = grow_output(s, out_capacity(s->cfg, s->format, tags));
	if (rc != KG_OK) return rc;
	s->tags = tags;
	return KG_OK;
}

int kg_stream_set_read_group(kg_stream *s, const char *id, int len)
{
	if (!s) return fail(KG_ERR_ARG, "kg_stream_set_read_group: null stream");
	if (!id && len != 0) return fail(KG_ERR_ARG, "kg_stream_set_read_group: no ID but a length of %d", len);
	if (id && (len < 1 || len > kRgMaxId)) return fail(KG_ERR_ARG, "kg_stream_set_read_group: an ID has 1 to %d bytes, not %d (NULL clears the read group)", kRgMaxId, len);
	for (int i = 0; id && i < len; ++i)
		if (id[i] < '!' || id[i] > '~') return fail(KG_ERR_ARG, "kg_stream_set_read_group: byte %d of the ID (0x%02x) is outside '!'..'~'", i, (unsigned)(unsigned char)id[i]);
	HIP_TRY(hipSetDevice(s->ix->device));
	if (id) {
		// The lanes' output buffers stay as they are.  They are sized for the worst batch two full windows can hold, which an ordinary batch fills by half,
		// and giving every lane a new device and page-locked buffer for 6 + len bytes more per read cost a run more than the field itself (0.8 s of a
		// 1.5 s run).  kg_stream_map knows each batch's true size before its text is made and grows the buffers of a batch that needs it.
		// no lane is inside a call, so no kernel reads the old forms: both new ones, each with zeros behind it
		uint8_t form[kRgBytes] = {0};
		memcpy(form, "\tRG:Z:", 6); memcpy(form + 6, id, (size_t)len);
		memcpy(form + kRgBamAt, "RGZ", 3); memcpy(form + kRgBamAt + 3, id, (size_t)len);
		HIP_TRY(hipMemcpy(s->d_rg, form, kRgBytes, hipMemcpyHostToDevice));
	}
	s->rg_len = id ? len : 0;
	return KG_OK;
}

int kg_stream_set_unmapped(kg_stream *s, int on)
{
	if (!s) return fail(KG_ERR_ARG, "kg_stream_set_unmapped: null stream");
	// (nothing is allocated here: a lane's tables and buffers come, and grow, inside the kg_stream_map calls that need them -- giving every lane new device
	//  and page-locked buffers in a setter cost a run more than the feature it switched on)
	s->unmapped = on != 0;
	return KG_OK;
}

int kg_stream_set_stats(kg_stream *s, int on)
{
	if (!s) return fail(KG_ERR_ARG, "kg_stream_set_stats: null stream");
	// (nothing is allocated here, as in kg_stream_set_unmapped: a lane's rows come, and grow, inside the kg_stream_map calls that need them)
	s->stats = on != 0;
	return KG_OK;
}

int kg_stream_set_input(kg_stream *s, int input)
{
	if (!s) return fail(KG_ERR_ARG, "kg_stream_set_input: null stream");
	if (input != KG_STREAM_INPUT_FASTQ && input != KG_STREAM_INPUT_FASTA) return fail(KG_ERR_ARG, "kg_stream_set_input: unknown input %d (KG_STREAM_INPUT_FASTQ or KG_STREAM_INPUT_FASTA)", input);
	HIP_TRY(hipSetDevice(s->ix->device));
	if (input == KG_STREAM_INPUT_FASTA) {
		// the per-line arrays of the FASTA record kernels, and room for their scan, from the first FASTA run on
		// The record tables were sized for four-line records (line_capacity / 4); a FASTA record can be two lines.  A window with more records than
		// that -- a header with nothing behind it is a record of ONE line -- goes back to the caller's reader (FQ_STOP_IRREGULAR), as one with too many lines
		const size_t want_scan = fa_scan_temp_bytes(s->line_capacity);
		const int64_t rec_capacity = s->line_capacity / 2 + 1;
		for (Lane &l : s->lanes) {
			if (s->fasta_sized) break;
			HIP_TRY(hipStreamSynchronize(l.ws->stream));
			for (int f = 0; f < 2; ++f) {
				HIP_TRY(grow_device(l.d_rec[f], 4 * 6 * (size_t)rec_capacity, kAllocFirst));     // (a failure leaves the stream usable for FASTQ)
				if (!l.d_line_acc[f]) HIP_TRY(hipMalloc((void **)&l.d_line_acc[f], 8 * (size_t)(s->line_capacity + 1)));
				if (!l.d_rec_line[f]) HIP_TRY(hipMalloc((void **)&l.d_rec_line[f], 4 * (size_t)(rec_capacity + 1)));
				HIP_TRY(hipMemset(l.d_line_acc[f], 0, 8 * (size_t)(s->line_capacity + 1)));
				HIP_TRY(hipMemset(l.d_rec_line[f], 0, 4 * (size_t)(rec_capacity + 1)));
			}
			if (l.scan_bytes < want_scan) {
				HIP_TRY(hipStreamSynchronize(l.ws->stream));
				HIP_TRY(grow_device(l.d_scan, l.scan_bytes, want_scan, want_scan));
			}
		}
	}
	if (input == KG_STREAM_INPUT_FASTA && !s->fasta_sized) { s->rec_capacity = s->line_capacity / 2 + 1; s->fasta_sized = true; }
	s->input = input;
	return KG_OK;
}

char *kg_stream_staging(kg_stream *s, int lane, int file, int64_t *capacity)
{
	if (!s || lane < 0 || lane >= (int)s->lanes.size() || file < 0 || file > 1) return nullptr;
	if (capacity) *capacity = s->cfg.max_window;
	return s->lanes[(size_t)lane].h_text[file];
}

int kg_stream_upload(kg_stream *s, int lane, int file, int64_t from, int64_t to)
{
	if (!s || lane < 0 || lane >= (int)s->lanes.size() || file < 0 || file > 1) return fail(KG_ERR_ARG, "kg_stream_upload: bad argument");
	if (from < 0 || to < from || to > s->cfg.max_window) return fail(KG_ERR_ARG, "kg_stream_upload: range [%lld, %lld) outside the staging buffer", (long long)from, (long long)to);
	if (to == from) return KG_OK;
	Lane &l = s->lanes[(size_t)lane];
	HIP_TRY(hipSetDevice(s->ix->device));
	HIP_TRY(hipMemcpyAsync(l.d_text[file] + from, l.h_text[file] + from, (size_t)(to - from), hipMemcpyHostToDevice, l.ws->stream));
	return KG_OK;
}

int kg_stream_parse(kg_stream *s, int lane, const kg_stream_window *w, kg_stream_parsed *out)
{
	if (!s || !w || !out || lane < 0 || lane >= (int)s->lanes.size()) return fail(KG_ERR_ARG, "kg_stream_parse: bad argument");
	Lane &l = s->lanes[(size_t)lane];
	const int nf = w->two_files ? 2 : 1;
	for (int f = 0; f < nf; ++f)
		if (w->begin[f] < 0 || w->end[f] < w->begin[f] || w->end[f] > s->cfg.max_window) return fail(KG_ERR_ARG, "kg_stream_parse: window %d outside the staging buffer", f);
	if (w->chunk_reads < 2 || (w->chunk_reads & 1) || w->want_reads < w->chunk_reads || w->want_reads > s->cfg.max_reads || w->want_reads % w->chunk_reads)
		return fail(KG_ERR_ARG, "kg_stream_parse: want_reads must be a multiple of chunk_reads (an even number) within the stream's batch size");
	HIP_TRY(hipSetDevice(s->ix->device));
	l.win = *w;
	l.have_batch = false;
	l.fasta = s->input == KG_STREAM_INPUT_FASTA;
	kg_workspace *ws = l.ws;
	FqArgs a;
	a.w[0] = window_of(s, l, 0);
	a.w[1] = window_of(s, l, 1);
	if (!w->two_files) { a.w[1].begin = a.w[1].end = 0; a.w[1].eof = 1; }
	a.two_files = w->two_files ? 1 : 0;
	a.paired = w->paired ? 1 : 0;
	a.chunk_reads = w->chunk_reads;
	a.fasta = s->input == KG_STREAM_INPUT_FASTA ? 1 : 0;
	a.gz_lines = w->gz_lines ? 1 : 0;
	a.max_reads = s->cfg.max_reads;
	a.want_reads = w->want_reads;
	a.meta = l.d_meta;
	a.read_len = l.d_read_len;
	a.read_off = ws->d_read_off;
	a.enc = ws->d_enc;
	a.n_reads = 0;
	hipStream_t st = ws->stream;
	KtUse kt_use(ws->profiling ? &ws->kt : nullptr);
	HIP_TRY(hipEventRecord(l.ev[0], st));
	HIP_TRY(launch_fq_parse(a, l.d_scan, l.scan_bytes, s->ix->n_cu, st));
	HIP_TRY(hipMemcpyAsync(l.h_meta, l.d_meta, 8 * FQM_WORDS, hipMemcpyDeviceToHost, st));
	HIP_TRY(kgi_sync(ws));
	kg_stream_parsed &p = l.parsed;
	p.n_reads = l.h_meta[FQM_READS]; p.n_chunks = l.h_meta[FQM_CHUNKS]; p.n_bases = l.h_meta[FQM_BASES];
	p.used[0] = l.h_meta[FQM_USED0]; p.used[1] = w->two_files ? l.h_meta[FQM_USED1] : 0;
	p.stop = (int32_t)l.h_meta[FQM_STOP]; p.done = (int32_t)l.h_meta[FQM_DONE];
	if (p.n_bases > ws->max_bases) return fail(KG_ERR_CAPACITY, "kg_stream_parse: %lld bases exceed the lane's workspace (%lld)", (long long)p.n_bases, (long long)ws->max_bases);
	if (p.n_reads > 0) {
		a.n_reads = p.n_reads;
		HIP_TRY(launch_fq_materialise(a, s->ix->n_cu, st));
		// where every record of the batch starts in its window: the caller re-reads the few reads that come back as KG_ALN_HOST
		const int64_t r0 = w->two_files ? p.n_reads / 2 : p.n_reads;
		HIP_TRY(hipMemcpyAsync(l.h_rec_hdr[0], a.w[0].rec_hdr, 4 * (size_t)r0, hipMemcpyDeviceToHost, st));
		if (w->two_files) HIP_TRY(hipMemcpyAsync(l.h_rec_hdr[1], a.w[1].rec_hdr, 4 * (size_t)r0, hipMemcpyDeviceToHost, st));
	}
	if (!s->groups.empty() && p.n_reads > 0) {
		// the batch as a segment of its group's batch: every slot's offset in the group's character array and its length
		SeedGroup &sg = *s->groups[(size_t)lane / (size_t)s->cfg.seed_group];
		const int j = lane - sg.first;
		HIP_TRY(launch_group_publish(ws->d_read_off, p.n_reads, sg.stride, (int64_t)j * sg.seg_bases, sg.ws->d_read_off + (int64_t)j * sg.stride,
		                             sg.ws->group_read_len + (int64_t)j * sg.stride, s->ix->n_cu, st));
		HIP_TRY(hipEventRecord(l.ev_parsed, st));
	}
	HIP_TRY(hipEventRecord(l.ev[1], st));
	l.have_batch = p.n_reads > 0;
	*out = p;
	return KG_OK;
}

// the lane's part in a round of its group (see SeedGroup): returns when the round's seeding is done and the lane's seeds lie in its
// own workspace; *was_leader: this call launched the round (its search kernel counts once in the statistics)
static int group_seed(kg_stream *s, int lane, int64_t n, int64_t n_bases, int64_t *n_seeds, bool *was_leader, float *search_ms, double *useful_bytes)
{
	SeedGroup &sg = *s->groups[(size_t)lane / (size_t)s->cfg.seed_group];
	Lane &l = s->lanes[(size_t)lane];
	const int j = lane - sg.first;
	*was_leader = false;
	std::unique_lock<std::mutex> lk(sg.mu);
	if (sg.aborted) return fail(KG_ERR_ARG, "kg_stream_map: the stream's seeding groups were aborted");
	if (sg.absent_rounds[j] < 0) return fail(KG_ERR_ARG, "kg_stream_map: lane %d was declared absent until further notice (kg_stream_group_absent) and arrives with a batch", lane);
	// (a lane that sits out a round and is back with a batch before that round has run waits for it)
	if (!sg.cv.wait_for(lk, std::chrono::seconds(600), [&]() { return sg.absent_rounds[j] == 0 || sg.aborted; })) {
		sg.aborted = true;
		sg.cv.notify_all();
		return fail(KG_ERR_ARG, "kg_stream_map: lane %d waited 600 s for the round it declared itself absent from", lane);
	}
	if (sg.aborted) return fail(KG_ERR_ARG, "kg_stream_map: the stream's seeding groups were aborted");
	const int64_t my_round = sg.round;
	sg.present[j] = true;
	sg.n_reads[j] = n;
	sg.arrived++;
	auto run_round = [&]() {           // (sg.mu held by the caller; every other lane of the group waits or is absent)
		kg_workspace *gw = sg.ws;
		int64_t counts[kMaxSeedSegments];
		int rc = KG_OK;
		for (int i = 0; i < sg.size && rc == KG_OK; ++i) {
			counts[i] = sg.present[i] ? sg.n_reads[i] : 0;
			// every lane publishes its slots ON ITS OWN STREAM -- a batch in kg_stream_parse, an absence (all slots empty) in kg_stream_group_absent --
			// and records ev_parsed behind it: the round waits for all of them.  (Round 4 zeroed an absent lane's slots here, on the group's
			// stream: nothing ordered that against the lane's publish of its NEXT batch, which it may parse before this round has run --
			// the memset could then wipe the lengths and the whole batch came out unmapped.)
			if (hipStreamWaitEvent(gw->stream, s->lanes[(size_t)(sg.first + i)].ev_parsed, 0) != hipSuccess) rc = fail(KG_ERR_NO_DEVICE, "kg_stream_map: hipStreamWaitEvent");
		}
		if (rc == KG_OK) rc = kgi_seed_group(gw, KG_MODE_FAST | KG_INPUT_ASCII, s->min_seed_len, KG_OCC_THR_DEFAULT, sg.size, sg.stride, counts, sg.seed_base);
		if (rc == KG_OK && (hipMemcpyAsync(sg.h_ctl, gw->d_ctl, 8 * kCtlWords, hipMemcpyDeviceToHost, gw->stream) != hipSuccess || kgi_sync(gw) != hipSuccess))
			rc = fail(KG_ERR_NO_DEVICE, "kg_stream_map: reading the group's counters back");
		sg.rc = rc;
		sg.n_order = 0; sg.turn = 0;
		for (int i = 0; i < sg.size; ++i)
			if (sg.present[i]) sg.order[sg.n_order++] = i;
		for (int i = 0; i < sg.size; ++i) {
			sg.present[i] = false;
			if (sg.absent_rounds[i] > 0) sg.absent_rounds[i]--;
		}
		sg.arrived = 0;
		sg.round++;
		sg.cv.notify_all();
	};
	// whoever finds the round complete runs it: the lane that arrives last, or -- when an absence completed it -- the first waiting
	// lane to look (kg_stream_group_absent wakes them).  The wait is bounded: a caller that lets a lane neither arrive nor declare
	// itself absent would hang the others for ever.
	const std::chrono::steady_clock::time_point give_up = std::chrono::steady_clock::now() + std::chrono::seconds(600);
	auto leave = [&]() {                // (an aborted round: this lane is no longer part of it)
		if (sg.round == my_round && sg.present[j]) { sg.present[j] = false; sg.arrived--; }
	};
	for (;;) {
		if (sg.aborted) { leave(); return fail(KG_ERR_ARG, "kg_stream_map: the stream's seeding groups were aborted"); }
		if (sg.round != my_round) break;
		if (round_complete(sg)) {
			run_round();
			*was_leader = true;
			if (sg.rc == KG_OK) {
				kg_workspace *gw = sg.ws;
				*search_ms = gw->profiling && gw->ev[0] ? elapsed(gw->ev[0], gw->ev[1]) : 0;
				*useful_bytes = search_useful_bytes(s->ix, sg.h_ctl, gw->group_prefix[sg.size]);
			}
			break;
		}
		if (sg.cv.wait_until(lk, give_up) == std::cv_status::timeout) {
			sg.aborted = true;
			sg.cv.notify_all();
			leave();
			return fail(KG_ERR_ARG, "kg_stream_map: lane %d waited 600 s for the other lanes of its seeding group (a lane without a batch must call kg_stream_group_absent)", lane);
		}
	}
	if (sg.rc != KG_OK) return sg.rc;
	const int64_t first = sg.seed_base[j], count = (j + 1 < sg.size ? sg.seed_base[j + 1] : sg.seed_base[sg.size]) - first;
	lk.unlock();
	// ---- the lane's slice: offsets rebased, seeds copied into its own workspace (the group's arrays belong to the next round) ----
	kg_workspace *ws = l.ws, *gw = sg.ws;
	if (count > ws->seed_capacity) {
		if (ws->d_seeds) HIP_TRY(hipFree(ws->d_seeds));
		ws->d_seeds = nullptr;
		const int64_t want = std::max<int64_t>(count + count / 4, 8 * ws->max_reads + 1024);
		HIP_TRY(hipMalloc((void **)&ws->d_seeds, sizeof(kg_seed) * (size_t)want));
		ws->seed_capacity = want;
	}
	HIP_TRY(launch_group_rebase(gw->d_seed_off + (int64_t)j * sg.stride, n, first, ws->d_seed_off, s->ix->n_cu, ws->stream));
	if (count > 0) HIP_TRY(hipMemcpyAsync(ws->d_seeds, gw->d_seeds + first, sizeof(kg_seed) * (size_t)count, hipMemcpyDeviceToDevice, ws->stream));
	ws->last_reads = n; ws->last_seeds = count; ws->last_cands = -1; ws->last_ascii = true;
	(void)n_bases;
	*n_seeds = count;
	return KG_OK;
}

// ---- kg_stream_map, piece by piece: all on the lane's stream, in this order --------------------------------------------------------

// what one kg_stream_map call carries from piece to piece
struct MapCall {
	const kg_stream_params *prm = nullptr;
	int64_t n = 0;                                     // reads of the batch
	int n_chunks = 0;
	bool grouped = false, group_leader = false;        // group_leader: this call launched its group's round (the launch counts once in the statistics)
	float group_search_ms = 0;
	double group_useful = 0;
	int64_t n_seeds = 0, totals[2] = {0, 0};           // candidates and their seeds
	AlnArgs a;
	SamArgs q;
	MdRef mdref{};                                     // what MD:Z needs of the index
	bool md = false;                                   // the batch's records carry MD:Z (the stream's tags when its text was sized)
	bool checksum = false;
	bool bgzf = false;                                 // the BGZF launch of the batch is on the lane's stream (KG_STREAM_FORMAT_BAM_BGZF)
	bool un = false;                                   // the batch's unmapped units are handed back (the stream's setting when its text was sized)
	UnArgs u{};
	int64_t un_bytes[2] = {0, 0};
	bool tally = false;                                // the batch's records are tallied (the stream's setting when the kernel was launched)
	int64_t sam_bytes = 0, n_host = 0, extra = 0;      // bytes of text, reads handed back, extra records of -m
};

// seeding (IdentifySeedPairs_FastMode) on the resident characters: in the lane's group's round, after which the lane takes its turn, or alone
static int map_seed(kg_stream *s, int lane, MapCall &m, GroupTurn &turn)
{
	Lane &l = s->lanes[(size_t)lane];
	kg_workspace *ws = l.ws;
	int rc;
	if (m.grouped) {
		rc = group_seed(s, lane, m.n, l.parsed.n_bases, &m.n_seeds, &m.group_leader, &m.group_search_ms, &m.group_useful);
		static const bool no_turns = getenv("KG_GROUP_NO_TURNS") != nullptr;          // A/B aid: the lanes of a group start their stages at once
		SeedGroup &sg = *s->groups[(size_t)lane / (size_t)s->cfg.seed_group];
		if (rc == KG_OK && !no_turns && !turn.acquire(sg, lane - sg.first)) rc = fail(KG_ERR_ARG, "kg_stream_map: the stream's seeding groups were aborted");
		if (rc != KG_OK) {                  // (this lane will never take its turn: nobody may wait for it)
			std::lock_guard<std::mutex> lk(sg.mu);
			sg.aborted = true;
			sg.cv.notify_all();
		}
	} else rc = kgi_seed_resident(ws, KG_MODE_FAST | KG_INPUT_ASCII, s->min_seed_len, KG_OCC_THR_DEFAULT, m.n, l.parsed.n_bases, &m.n_seeds);
	if (rc != KG_OK) return rc;
	if (!m.grouped) HIP_TRY(hipMemcpyAsync(l.h_ctl, ws->d_ctl, 8 * kCtlWords, hipMemcpyDeviceToHost, ws->stream));
	HIP_TRY(hipEventRecord(l.ev[2], ws->stream));
	return KG_OK;
}

static int map_chain(Lane &l, MapCall &m)
{
	int rc = kgi_chain_resident(l.ws, 0, m.prm->max_gaps, m.totals);
	if (rc != KG_OK) return rc;
	HIP_TRY(hipEventRecord(l.ev[3], l.ws->stream));
	return KG_OK;
}

// the per-read report
static int map_report(Lane &l, MapCall &m)
{
	const int n_chunks = m.n_chunks;
	std::vector<int64_t> chunk_off((size_t)n_chunks + 1);
	std::vector<uint8_t> chunk_paired((size_t)n_chunks, (uint8_t)(l.win.paired ? 1 : 0));
	for (int c = 0; c <= n_chunks; ++c) chunk_off[(size_t)c] = std::min<int64_t>(m.n, (int64_t)c * l.win.chunk_reads);
	if (n_chunks > l.chunk_capacity) {
		const int64_t want = n_chunks + n_chunks / 2 + 64;
		HIP_TRY(grow_pinned(l.h_chunk_stats, l.chunk_capacity, want, sizeof(kg_chunk_stats) * (size_t)want));
	}
	int rc = kgi_align_resident(l.ws, chunk_off.data(), chunk_paired.data(), n_chunks, m.prm->est_distance, m.prm->max_insert, m.prm->max_gaps, m.prm->multi_hit,
	                            m.prm->unset_flag, l.record_capacity, m.a);
	if (rc != KG_OK) return rc;
	HIP_TRY(hipEventRecord(l.ev[4], l.ws->stream));
	return KG_OK;
}

// kg_stream_set_unmapped: which units are handed back and how many bytes each takes in either file; the totals are on their way to the lane's words when
// this returns (map_size_text's sync brings them over).  The lane's tables are allocated by its first call
static int map_un_size(kg_stream *s, Lane &l, MapCall &m)
{
	hipStream_t st = l.ws->stream;
	const int nf = l.win.two_files ? 2 : 1;
	if (l.win.two_files && !l.win.paired) return fail(KG_ERR_ARG, "kg_stream_map: the unmapped reads of two files are handed back as pairs (kg_stream_window::paired)");
	const size_t slots = (size_t)s->cfg.max_reads + 8;
	if (!l.d_un_ctl) HIP_TRY(hipMalloc((void **)&l.d_un_ctl, 8 * 4));
	for (int f = 0; f < nf; ++f) {
		if (l.d_un_len[f]) continue;
		HIP_TRY(hipMalloc((void **)&l.d_un_len[f], 4 * slots));
		HIP_TRY(hipMalloc((void **)&l.d_un_off[f], 8 * slots));
		HIP_TRY(hipHostMalloc((void **)&l.h_un_off[f], 8 * slots, hipHostMallocDefault));
	}
	UnArgs &u = m.u;
	u.w[0] = m.q.w[0]; u.w[1] = m.q.w[1];
	u.two_files = m.q.two_files; u.paired = m.q.paired; u.fasta = m.q.fasta;
	u.n_units = l.win.paired ? m.n / 2 : m.n;
	u.records = m.a.records;
	for (int f = 0; f < 2; ++f) { u.un_len[f] = l.d_un_len[f]; u.un_off[f] = l.d_un_off[f]; u.un[f] = l.d_un[f]; u.un_capacity[f] = l.d_un_capacity[f]; }
	u.ctl = l.d_un_ctl;
	HIP_TRY(launch_un_size(u, l.d_scan, l.scan_bytes, s->ix->n_cu, st));
	int64_t *word = l.h_meta + FQM_WORDS;
	word[LW_UN_BYTES] = word[LW_UN_BYTES + 1] = 0;
	for (int f = 0; f < nf; ++f) HIP_TRY(hipMemcpyAsync(&word[LW_UN_BYTES + f], l.d_un_off[f] + u.n_units, 8, hipMemcpyDeviceToHost, st));
	m.un = true;
	return KG_OK;
}

// ... and, once the totals are here (the lane's stream is synchronised), room for the bytes: device and page-locked buffers that hold them
static int map_un_room(Lane &l, MapCall &m)
{
	const int64_t *word = l.h_meta + FQM_WORDS;
	for (int f = 0; f < (l.win.two_files ? 2 : 1); ++f) {
		const int64_t bytes = m.un_bytes[f] = word[LW_UN_BYTES + f];
		// (the bytes are a part of the window's: a total beyond it is a table gone wrong, not a size to allocate)
		if (bytes < 0 || bytes > (l.win.end[f] - l.win.begin[f]) + 1) return fail(KG_ERR_NO_DEVICE, "kg_stream_map: %lld bytes of unmapped reads in a window of %lld", (long long)bytes, (long long)(l.win.end[f] - l.win.begin[f]));
		const int64_t want = std::max<int64_t>(bytes + bytes / 8, 1 << 16);
		if (bytes > l.d_un_capacity[f]) HIP_TRY(grow_device(l.d_un[f], l.d_un_capacity[f], want, (size_t)want));
		if (bytes > l.h_un_capacity[f]) HIP_TRY(grow_pinned(l.h_un[f], l.h_un_capacity[f], want, (size_t)want));
		m.u.un[f] = l.d_un[f]; m.u.un_capacity[f] = l.d_un_capacity[f];
	}
	return KG_OK;
}

// the size of every read's text (one sync: the totals come over), and buffers that hold the text and, on the host, the batch's candidates
static int map_size_text(kg_stream *s, Lane &l, MapCall &m)
{
	kg_workspace *ws = l.ws;
	hipStream_t st = ws->stream;
	const int64_t n = m.n;
	SamArgs &q = m.q;
	q.w[0] = window_of(s, l, 0); q.w[1] = window_of(s, l, 1);
	q.two_files = l.win.two_files ? 1 : 0; q.paired = l.win.paired ? 1 : 0;
	q.fasta = l.fasta ? 1 : 0;
	q.enc = ws->d_enc; q.read_off = ws->d_read_off; q.n_reads = n;
	q.records = m.a.records;
	q.chr_names = s->d_chr_names; q.chr_name_off = s->d_chr_name_off;
	q.sam_len = l.d_sam_len; q.sam_off = l.d_sam_off; q.sam = l.d_sam; q.sam_capacity = l.d_sam_capacity;
	q.host_list = l.d_host_list; q.ctl = l.d_sam_ctl;
	// (the size kernel and the format kernel of a batch see the same read group: both take it from here)
	const bool bam = s->format != KG_STREAM_FORMAT_SAM;
	q.rg = s->rg_len > 0 ? s->d_rg + (bam ? kRgBamAt : 0) : nullptr;
	q.rg_len = s->rg_len > 0 ? (bam ? 4 : 6) + s->rg_len : 0;
	{
		const kg_index *ix = s->ix;
		const int n_chr = (int)ix->contigs.size();
		m.mdref.text = ix->d_text; m.mdref.genome_size = ix->l_pac;
		m.mdref.chr_fwd_start = ix->d_chr_tab; m.mdref.chr_len = ix->d_chr_tab + 2 * n_chr;
		m.mdref.n_chr = n_chr; m.mdref.n_holes = ix->n_holes;
		m.mdref.hole_start = ix->d_hole_start; m.mdref.hole_len = ix->d_hole_len; m.mdref.hole_char = ix->d_hole_char;
	}
	m.md = (s->tags & KG_STREAM_TAG_MD) != 0;
	HIP_TRY(launch_text_size(q, s->format != KG_STREAM_FORMAT_SAM, m.md ? &m.mdref : nullptr, l.d_scan, l.scan_bytes, s->ix->n_cu, st));
	int64_t *word = l.h_meta + FQM_WORDS;
	HIP_TRY(hipMemcpyAsync(&word[LW_TEXT_BYTES], l.d_sam_off + n, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&word[LW_HOST_READS], l.d_sam_ctl, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&word[LW_EXTRA_RECORDS], ws->d_aln_ctl + 7, 8, hipMemcpyDeviceToHost, st));
	if (s->unmapped) {
		int rc = map_un_size(s, l, m);
		if (rc != KG_OK) return rc;
	}
	HIP_TRY(kgi_sync(ws));
	if (m.un) {
		int rc = map_un_room(l, m);
		if (rc != KG_OK) return rc;
	}
	const int64_t sam_bytes = m.sam_bytes = word[LW_TEXT_BYTES];
	m.n_host = word[LW_HOST_READS];
	m.extra = m.prm->multi_hit ? std::min<int64_t>(word[LW_EXTRA_RECORDS], m.a.extra_capacity) : 0;
	if (sam_bytes > l.d_sam_capacity) {
		// (never seen: the estimate in kg_stream_open is generous; -m on a repeat-rich genome could get here)
		HIP_TRY(grow_device(l.d_sam, l.d_sam_capacity, sam_bytes + sam_bytes / 4, (size_t)(sam_bytes + sam_bytes / 4)));
		q.sam = l.d_sam; q.sam_capacity = l.d_sam_capacity;
	}
	if (sam_bytes > l.h_sam_capacity) {
		HIP_TRY(grow_pinned(l.h_sam, l.h_sam_capacity, sam_bytes + sam_bytes / 4, (size_t)(sam_bytes + sam_bytes / 4)));
	}
	const int64_t cand_need = std::max(m.totals[0], m.totals[1]);
	if (cand_need > l.h_cand_capacity) {
		// (two buffers under one capacity: both are freed before either is allocated)
		const int64_t want = std::max<int64_t>(cand_need + cand_need / 4 + 1024, 3 * s->cfg.max_reads);
		if (l.h_cands) HIP_TRY(hipHostFree(l.h_cands));
		if (l.h_cand_seeds) HIP_TRY(hipHostFree(l.h_cand_seeds));
		l.h_cands = nullptr; l.h_cand_seeds = nullptr;
		l.h_cand_capacity = 0;
		HIP_TRY(grow_pinned(l.h_cands, sizeof(kg_candidate) * (size_t)want));
		HIP_TRY(grow_pinned(l.h_cand_seeds, sizeof(kg_seed) * (size_t)want));
		l.h_cand_capacity = want;
	}
	return KG_OK;
}

// KG_STREAM_FORMAT_BAM_BGZF: the records as BGZF blocks, cut where a chunk begins and where a read was handed back; the totals are on their way
// to the lane's words when this returns (map_copy_out waits for them: the mode's one more sync)
static int map_bgzf(kg_stream *s, Lane &l, MapCall &m)
{
	hipStream_t st = l.ws->stream;
	const int64_t blocks = bgzf_max_blocks(m.sam_bytes, (int64_t)m.n_chunks + m.n_host + 1);
	if (blocks > l.bgzf_blocks || m.sam_bytes + 31 * blocks > l.d_bgzf_capacity) {
		HIP_TRY(kgi_sync(l.ws));
		int rc = bgzf_room(s, l, blocks, m.sam_bytes);
		if (rc != KG_OK) return rc;
	}
	BgzfArgs z{};
	z.src = l.d_sam; z.src_bytes = m.sam_bytes;
	z.cuts = l.d_cuts; z.n_cuts = m.n + 1;
	z.max_blocks = l.bgzf_blocks;
	z.range_first = l.d_range_first; z.block_src = l.d_block_src; z.block_bytes = l.d_block_bytes; z.block_off = l.d_block_off;
	z.slots = l.d_slots; z.dst = l.d_bgzf; z.dst_capacity = l.d_bgzf_capacity; z.ctl = l.d_bgzf_ctl;
	HIP_TRY(hipMemsetAsync(l.d_bgzf_ctl, 0, 8 * BGZ_WORDS, st));
	HIP_TRY(launch_bgzf_stream_cuts(l.d_sam_off, m.n, l.win.chunk_reads > 0 ? l.win.chunk_reads : 1, l.d_cuts, l.d_bgzf_scan, l.bgzf_scan_bytes, s->ix->n_cu, st));
	HIP_TRY(launch_bgzf(z, l.d_bgzf_scan, l.bgzf_scan_bytes, s->ix->n_cu, st));
	HIP_TRY(hipMemcpyAsync(l.h_meta + FQM_WORDS + LW_BGZF, l.d_bgzf_ctl, 8 * BGZ_WORDS, hipMemcpyDeviceToHost, st));
	m.bgzf = true;
	return KG_OK;
}

// kg_stream_set_stats: the tally of the batch's final records, a row per chunk (the records are final once the report stage is through: the text
// kernels only read them).  The lane's rows are allocated by its first call and grow with a batch of more chunks
static int map_tally(Lane &l, MapCall &m)
{
	if (m.n_chunks > l.tally_capacity) {
		const int64_t want = m.n_chunks + m.n_chunks / 2 + 64;
		HIP_TRY(grow_device(l.d_tally, l.tally_capacity, want, 4 * (size_t)KG_STATS_WORDS * (size_t)want));
	}
	if (m.n_chunks > l.h_tally_capacity) {
		const int64_t want = m.n_chunks + m.n_chunks / 2 + 64;
		HIP_TRY(grow_pinned(l.h_tally, l.h_tally_capacity, want, 4 * (size_t)KG_STATS_WORDS * (size_t)want));
	}
	StatsArgs t{};
	t.records = m.a.records;
	t.n_reads = m.n; t.n_records = m.n + m.extra;
	t.chunk_off = m.a.chunk_off; t.n_chunks = m.n_chunks;
	t.rows = l.d_tally;
	HIP_TRY(launch_stats_tally(t, l.ws->stream));
	m.tally = true;
	return KG_OK;
}

static int map_format(kg_stream *s, Lane &l, MapCall &m)
{
	hipStream_t st = l.ws->stream;
	HIP_TRY(launch_text_format(m.q, s->format != KG_STREAM_FORMAT_SAM, m.md ? &m.mdref : nullptr, s->ix->n_cu, st));
	// measurement aid (bench.py's gpu_pipeline leg): the text summed on the device, for runs that never copy it into file pages (read per call: a session switches it on and off)
	m.checksum = getenv("KG_STREAM_CHECKSUM") != nullptr;
	if (m.checksum) HIP_TRY(launch_sam_checksum(m.q, s->ix->n_cu, st));
	if (m.un && m.un_bytes[0] + m.un_bytes[1] > 0) HIP_TRY(launch_un_copy(m.u, s->ix->n_cu, st));
	if (s->stats) {
		int rc = map_tally(l, m);
		if (rc != KG_OK) return rc;
	}
	if (s->format == KG_STREAM_FORMAT_BAM_BGZF) {
		int rc = map_bgzf(s, l, m);
		if (rc != KG_OK) return rc;
	}
	HIP_TRY(hipEventRecord(l.ev[5], st));
	return KG_OK;
}

// the batch back on the host (the second sync) and described in *out
static int map_copy_out(Lane &l, MapCall &m, kg_stream_result *out)
{
	kg_workspace *ws = l.ws;
	hipStream_t st = ws->stream;
	const int64_t n = m.n, n_host = m.n_host, extra = m.extra, *totals = m.totals;
	const AlnArgs &a = m.a;
	int64_t *word = l.h_meta + FQM_WORDS;
	int64_t n_blocks = 0, bgzf_bytes = 0;
	if (m.bgzf) {
		// how many blocks and bytes the device made of the records: known once its kernels are through
		HIP_TRY(kgi_sync(ws));
		const int64_t *z = word + LW_BGZF;
		n_blocks = z[BGZ_RUN]; bgzf_bytes = z[BGZ_BYTES];
		if (z[BGZ_BLOCKS] != n_blocks || n_blocks > l.bgzf_blocks) return fail(KG_ERR_NO_DEVICE, "kg_stream_map: the records make %lld BGZF blocks, the lane was sized for %lld", (long long)z[BGZ_BLOCKS], (long long)l.bgzf_blocks);
		if (z[BGZ_ERRORS] != 0) return fail(KG_ERR_NO_DEVICE, "kg_stream_map: %lld BGZF members missed the size computed for them", (long long)z[BGZ_ERRORS]);
		if (bgzf_bytes > l.d_bgzf_capacity) return fail(KG_ERR_NO_DEVICE, "kg_stream_map: %lld bytes of BGZF blocks where at most %lld can be", (long long)bgzf_bytes, (long long)l.d_bgzf_capacity);
		if (bgzf_bytes > l.h_bgzf_capacity) HIP_TRY(grow_pinned(l.h_bgzf, l.h_bgzf_capacity, bgzf_bytes + bgzf_bytes / 4, (size_t)(bgzf_bytes + bgzf_bytes / 4)));
		if (bgzf_bytes > 0) HIP_TRY(hipMemcpyAsync(l.h_bgzf, l.d_bgzf, (size_t)bgzf_bytes, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(l.h_block_src, l.d_block_src, 8 * (size_t)(n_blocks + 1), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(l.h_block_off, l.d_block_off, 8 * (size_t)(n_blocks + 1), hipMemcpyDeviceToHost, st));
	}
	if (m.sam_bytes > 0) HIP_TRY(hipMemcpyAsync(l.h_sam, l.d_sam, (size_t)m.sam_bytes, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(l.h_sam_off, l.d_sam_off, 8 * (size_t)(n + 1), hipMemcpyDeviceToHost, st));
	if (m.un) {
		// only the selected bytes cross the link; the offsets come whole, as sam_off does
		for (int f = 0; f < (l.win.two_files ? 2 : 1); ++f) {
			if (m.un_bytes[f] > 0) HIP_TRY(hipMemcpyAsync(l.h_un[f], l.d_un[f], (size_t)m.un_bytes[f], hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(l.h_un_off[f], l.d_un_off[f], 8 * (size_t)(m.u.n_units + 1), hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(hipMemcpyAsync(&word[LW_UN_CTL], l.d_un_ctl, 8 * 3, hipMemcpyDeviceToHost, st));
	}
	// the records, candidate offsets, candidates and their seeds stay on the device unless the caller wants them all: it asks for the chunks it needs
	// (kg_stream_fetch) -- 207 of the 605 bytes per read that used to cross the link
	const bool all = m.prm->fetch_all != 0;
	l.mapped_reads = n; l.d_records = a.records;
	if (all) HIP_TRY(hipMemcpyAsync(l.h_records, a.records, sizeof(kg_aln_record) * (size_t)(n + extra), hipMemcpyDeviceToHost, st));
	else if (extra > 0) HIP_TRY(hipMemcpyAsync(l.h_records + n, a.records + n, sizeof(kg_aln_record) * (size_t)extra, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(l.h_chunk_stats, ws->d_chunk_stats, sizeof(kg_chunk_stats) * (size_t)m.n_chunks, hipMemcpyDeviceToHost, st));
	if (m.tally) HIP_TRY(hipMemcpyAsync(l.h_tally, l.d_tally, 4 * (size_t)KG_STATS_WORDS * (size_t)m.n_chunks, hipMemcpyDeviceToHost, st));
	if (all) HIP_TRY(hipMemcpyAsync(l.h_cand_off, ws->d_cand_off, 8 * (size_t)(n + 1), hipMemcpyDeviceToHost, st));
	// the candidates travel with every batch: the reads handed back need them, and so does a pair the caller maps again because its
	// speculated EstDistance did not hold
	if (n_host > 0) HIP_TRY(hipMemcpyAsync(l.h_host_list, l.d_host_list, 4 * (size_t)n_host, hipMemcpyDeviceToHost, st));
	if (all && totals[0] > 0) HIP_TRY(hipMemcpyAsync(l.h_cands, ws->d_dense_cands, sizeof(kg_candidate) * (size_t)totals[0], hipMemcpyDeviceToHost, st));
	if (all && totals[1] > 0) HIP_TRY(hipMemcpyAsync(l.h_cand_seeds, ws->d_dense_seeds, sizeof(kg_seed) * (size_t)totals[1], hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&word[LW_FORMAT_ERRORS], l.d_sam_ctl + 1, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&word[LW_ALN_COUNTS], ws->d_aln_ctl, 8 * 7, hipMemcpyDeviceToHost, st));          // the alignment stage's list sizes of this batch ...
	HIP_TRY(hipMemcpyAsync(&word[LW_ALN_GENERAL], ws->d_aln_ctl + 32, 8, hipMemcpyDeviceToHost, st));        // ... and the candidates its fast plan kernel left to the general one
	word[LW_CHECKSUM] = word[LW_CHECKSUM + 1] = 0;
	if (m.checksum) HIP_TRY(hipMemcpyAsync(&word[LW_CHECKSUM], l.d_sam_ctl + 2, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&word[LW_ALN_TRIVIAL], ws->d_aln_ctl + 36, 8, hipMemcpyDeviceToHost, st));        // ... and the pairs aln_trivial_kernel decided (in the place of the piece count, which nobody reads)
	HIP_TRY(hipEventRecord(l.ev[6], st));
	HIP_TRY(kgi_sync(ws));
	if (word[LW_FORMAT_ERRORS] != 0) return fail(KG_ERR_NO_DEVICE, "kg_stream_map: %lld records were formatted to a size other than the one announced", (long long)word[LW_FORMAT_ERRORS]);
	if (m.un) {
		const bool copied = m.un_bytes[0] + m.un_bytes[1] > 0;       // (nothing selected: un_copy_kernel was not launched and its counters stand at zero)
		for (int f = 0; f < 2; ++f)
			if (word[LW_UN_CTL + f] != (copied ? m.un_bytes[f] : 0)) return fail(KG_ERR_NO_DEVICE, "kg_stream_map: %lld bytes of unmapped reads were written for file %d, %lld announced", (long long)word[LW_UN_CTL + f], f, (long long)m.un_bytes[f]);
		if (word[LW_UN_CTL + 2] != 0) return fail(KG_ERR_NO_DEVICE, "kg_stream_map: %lld spans of unmapped reads lie outside their window or buffer", (long long)word[LW_UN_CTL + 2]);
	}
	std::sort(l.h_host_list, l.h_host_list + n_host);
	out->n_reads = n; out->n_chunks = m.n_chunks;
	out->sam = l.h_sam; out->sam_bytes = m.sam_bytes; out->sam_off = l.h_sam_off;
	out->records = l.h_records; out->n_records = n + extra;
	out->chunk_stats = l.h_chunk_stats;
	out->host_reads = l.h_host_list; out->n_host_reads = n_host;
	out->cand_off = l.h_cand_off; out->cands = l.h_cands; out->cand_seeds = l.h_cand_seeds;
	out->rec_start[0] = l.h_rec_hdr[0]; out->rec_start[1] = l.win.two_files ? l.h_rec_hdr[1] : nullptr;
	if (m.bgzf) {
		out->bgzf = l.h_bgzf; out->bgzf_bytes = bgzf_bytes; out->n_blocks = n_blocks;
		out->block_src = l.h_block_src; out->block_off = l.h_block_off;
	}
	if (m.un) {
		for (int f = 0; f < (l.win.two_files ? 2 : 1); ++f) { out->un[f] = l.h_un[f]; out->un_bytes[f] = m.un_bytes[f]; out->un_off[f] = l.h_un_off[f]; }
		out->n_units = m.u.n_units;
	}
	if (m.tally) out->chunk_tally = l.h_tally;
	l.have_batch = false;
	return KG_OK;
}

// what the batch cost on the device, stage by stage, and what its search kernel fetched
static void map_account(kg_stream *s, Lane &l, const MapCall &m)
{
	kg_workspace *ws = l.ws;
	const int64_t *word = l.h_meta + FQM_WORDS;
	float sk = 0;
	if (!m.grouped && ws->profiling && ws->ev[0]) sk = elapsed(ws->ev[0], ws->ev[1]);
	double useful = m.grouped ? 0.0 : search_useful_bytes(s->ix, l.h_ctl, m.n);
	// (a group's launch counts once, with the lane that launched it)
	if (m.grouped && m.group_leader) { sk = m.group_search_ms; useful = m.group_useful; }
	std::lock_guard<std::mutex> lk(s->mu);
	kg_stream_timing_t &t = s->total;
	t.batches += 1; t.reads += m.n;
	t.parse_ms += elapsed(l.ev[0], l.ev[1]); t.seed_ms += elapsed(l.ev[1], l.ev[2]); t.chain_ms += elapsed(l.ev[2], l.ev[3]);
	t.align_ms += elapsed(l.ev[3], l.ev[4]); t.format_ms += elapsed(l.ev[4], l.ev[5]); t.copy_ms += elapsed(l.ev[5], l.ev[6]);
	t.search_kernel_ms += sk; t.search_kernel_launches += (!m.grouped || m.group_leader) ? 1 : 0; t.search_useful_bytes += useful;
	t.text_in_bytes += (double)((l.parsed.used[0] - l.win.begin[0]) + (l.win.two_files ? l.parsed.used[1] - l.win.begin[1] : 0));
	t.text_out_bytes += (double)m.sam_bytes;
	t.un_bytes += (double)(m.un_bytes[0] + m.un_bytes[1]);
	if (m.tally) t.stats_bytes += 4.0 * KG_STATS_WORDS * (double)m.n_chunks;
	t.candidates += (double)m.totals[0]; t.candidate_seeds += (double)m.totals[1];
	for (int i = 0; i < 8; ++i) t.aln_counts[i] += (double)word[LW_ALN_COUNTS + i];
	t.text_checksum[0] += (double)(uint64_t)word[LW_CHECKSUM]; t.text_checksum[1] += (double)(uint64_t)word[LW_CHECKSUM + 1];
	// the kernels' own launches of this batch (events around each, the lane's stream is synchronised)
	for (int i = 0; i < KT_SLOTS; ++i) {
		const int used = ws->kt.used[i];
		if (!used) continue;
		ws->kt.used[i] = 0;
		// (the sixteen slots of kernel_ms, then un_kernel_ms, then stats_kernel_ms)
		double &ms = i < 16 ? t.kernel_ms[i] : i == KT_STATS ? t.stats_kernel_ms : t.un_kernel_ms[i - 16];
		for (int j = 0; j < used; ++j) ms += elapsed(ws->kt.b[i][j], ws->kt.e[i][j]);
		(i < 16 ? t.kernel_launches[i] : i == KT_STATS ? t.stats_kernel_launches : t.un_kernel_launches[i - 16]) += used;
	}
}

int kg_stream_map(kg_stream *s, int lane, const kg_stream_params *prm, kg_stream_result *out)
{
	if (!s || !prm || !out || lane < 0 || lane >= (int)s->lanes.size()) return fail(KG_ERR_ARG, "kg_stream_map: bad argument");
	Lane &l = s->lanes[(size_t)lane];
	if (!l.have_batch) return fail(KG_ERR_ARG, "kg_stream_map: no parsed batch in lane %d (kg_stream_parse first)", lane);
	memset(out, 0, sizeof(*out));
	HIP_TRY(hipSetDevice(s->ix->device));
	KtUse kt_use(l.ws->profiling ? &l.ws->kt : nullptr);
	MapCall m;
	m.prm = prm;
	m.n = l.parsed.n_reads;
	m.n_chunks = (int)l.parsed.n_chunks;
	m.grouped = !s->groups.empty();
	GroupTurn turn;                                    // (released on every way out of this function)
	int rc;
	if ((rc = map_seed(s, lane, m, turn)) != KG_OK) return rc;
	if ((rc = map_chain(l, m)) != KG_OK) return rc;
	if ((rc = map_report(l, m)) != KG_OK) return rc;
	if ((rc = map_size_text(s, l, m)) != KG_OK) return rc;
	if ((rc = map_format(s, l, m)) != KG_OK) return rc;
	// (grouped seeding) the turn is kept until the batch is back on the host.  Passing it on here -- so that this lane's copies overlap the
	// next lane's kernels, KG_GROUP_TURN_EARLY=1 -- gives the same FASTQ -> SAM rate at 100 M reads (29.4-29.9 M against 29.8-30.4 M
	// mapped reads/s) while the next lane's first kernel then waits behind this one's copies: chain_kernel 5.0 ms per launch instead of 0.35,
	// the stage sums twice as long (profiles/r04u_trace_chain.log, r04v_ab_turn_late.log); the other group's lanes overlap either way.
	static const bool turn_early = getenv("KG_GROUP_TURN_EARLY") != nullptr;
	if (turn_early) turn.release();
	if ((rc = map_copy_out(l, m, out)) != KG_OK) return rc;
	map_account(s, l, m);
	return KG_OK;
}

int kg_stream_group_absent(kg_stream *s, int lane, int rounds)
{
	if (!s || lane < 0 || lane >= (int)s->lanes.size()) return fail(KG_ERR_ARG, "kg_stream_group_absent: bad argument");
	if (s->groups.empty()) return KG_OK;
	SeedGroup &sg = *s->groups[(size_t)lane / (size_t)s->cfg.seed_group];
	const int j = lane - sg.first;
	std::unique_lock<std::mutex> lk(sg.mu);
	if (sg.present[j]) return fail(KG_ERR_ARG, "kg_stream_group_absent: lane %d is inside a round", lane);
	if (rounds != 0) {
		// the lane's slots of the group's batch are empty from here on (until its next kg_stream_parse publishes a batch): on the lane's own stream
		Lane &l = s->lanes[(size_t)lane];
		HIP_TRY(hipSetDevice(s->ix->device));
		HIP_TRY(launch_group_publish(l.ws->d_read_off, 0, sg.stride, (int64_t)j * sg.seg_bases, sg.ws->d_read_off + (int64_t)j * sg.stride, sg.ws->group_read_len + (int64_t)j * sg.stride,
		                             s->ix->n_cu, l.ws->stream));
		HIP_TRY(hipEventRecord(l.ev_parsed, l.ws->stream));
	}
	sg.absent_rounds[j] = rounds;
	if (rounds == 0) sg.aborted = false;               // (a new run: the lanes take part again; an aborted run's half-finished round is forgotten)
	// the round may be complete now: everybody else has arrived and waits
	const bool complete = round_complete(sg);
	if (rounds != 0 && sg.arrived > 0 && complete) sg.cv.notify_all();     // a waiting lane runs the round (group_seed's loop)
	if (rounds > 0 && sg.arrived == 0 && complete) {
		// every lane of the group sits this round out: nobody will run it, so it is over here (the lanes would wait for it for ever)
		for (int i = 0; i < sg.size; ++i)
			if (sg.absent_rounds[i] > 0) sg.absent_rounds[i]--;
		sg.round++;
		sg.cv.notify_all();
	}
	return KG_OK;
}

int kg_stream_group_abort(kg_stream *s)
{
	if (!s) return fail(KG_ERR_ARG, "kg_stream_group_abort: null stream");
	for (std::unique_ptr<SeedGroup> &sg : s->groups) {
		std::lock_guard<std::mutex> lk(sg->mu);
		sg->aborted = true;
		sg->cv.notify_all();
	}
	return KG_OK;
}

int kg_stream_fetch_reads(kg_stream *s, int lane, uint8_t *enc, int64_t *read_off)
{
	if (!s || lane < 0 || lane >= (int)s->lanes.size() || !read_off) return fail(KG_ERR_ARG, "kg_stream_fetch_reads: bad argument");
	Lane &l = s->lanes[(size_t)lane];
	if (!l.have_batch) return fail(KG_ERR_ARG, "kg_stream_fetch_reads: no parsed batch in lane %d", lane);
	HIP_TRY(hipSetDevice(s->ix->device));
	HIP_TRY(kgi_sync(l.ws));
	HIP_TRY(hipMemcpy(read_off, l.ws->d_read_off, 8 * (size_t)(l.parsed.n_reads + 1), hipMemcpyDeviceToHost));
	if (enc && l.parsed.n_bases > 0) HIP_TRY(hipMemcpy(enc, l.ws->d_enc, (size_t)l.parsed.n_bases, hipMemcpyDeviceToHost));
	return KG_OK;
}

int kg_stream_fetch(kg_stream *s, int lane, int64_t first, int64_t count)
{
	if (!s || lane < 0 || lane >= (int)s->lanes.size()) return fail(KG_ERR_ARG, "kg_stream_fetch: bad lane");
	Lane &l = s->lanes[(size_t)lane];
	if (first < 0 || count < 0 || first + count > l.mapped_reads || !l.d_records) return fail(KG_ERR_ARG, "kg_stream_fetch: reads [%lld, %lld) are not of the lane's mapped batch (%lld reads)", (long long)first, (long long)(first + count), (long long)l.mapped_reads);
	if (count == 0) return KG_OK;
	kg_workspace *ws = l.ws;
	HIP_TRY(hipSetDevice(ws->ix->device));
	hipStream_t st = ws->stream;
	int64_t *seeds_at = l.h_meta + FQM_WORDS + LW_FETCH_SEEDS;
	HIP_TRY(hipMemcpyAsync(l.h_records + first, l.d_records + first, sizeof(kg_aln_record) * (size_t)count, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(l.h_cand_off + first, ws->d_cand_off + first, 8 * (size_t)(count + 1), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&seeds_at[0], ws->d_cseed_off + first, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&seeds_at[1], ws->d_cseed_off + first + count, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(kgi_sync(ws));
	const int64_t c0 = l.h_cand_off[first], c1 = l.h_cand_off[first + count], s0 = seeds_at[0], s1 = seeds_at[1];
	if (c0 < 0 || c1 < c0 || c1 > l.h_cand_capacity || s0 < 0 || s1 < s0 || s1 > l.h_cand_capacity) return fail(KG_ERR_NO_DEVICE, "kg_stream_fetch: the batch's candidate offsets are not what kg_stream_map left");
	if (c1 > c0) HIP_TRY(hipMemcpyAsync(l.h_cands + c0, ws->d_dense_cands + c0, sizeof(kg_candidate) * (size_t)(c1 - c0), hipMemcpyDeviceToHost, st));
	if (s1 > s0) HIP_TRY(hipMemcpyAsync(l.h_cand_seeds + s0, ws->d_dense_seeds + s0, sizeof(kg_seed) * (size_t)(s1 - s0), hipMemcpyDeviceToHost, st));
	HIP_TRY(kgi_sync(ws));
	return KG_OK;
}

int kg_tally_records(const kg_aln_record *records, int64_t n_records, int64_t n_reads, const int64_t *chunk_off, int n_chunks, uint32_t *rows)
{
	if (!chunk_off || !rows || n_chunks < 0 || n_reads < 0 || n_records < n_reads || (n_records > 0 && !records)) return fail(KG_ERR_ARG, "kg_tally_records: bad argument");
	for (int c = 0; c < n_chunks; ++c)
		if (chunk_off[c] < 0 || chunk_off[c + 1] < chunk_off[c] || chunk_off[c + 1] > n_reads)
			return fail(KG_ERR_ARG, "kg_tally_records: chunk %d is reads [%lld, %lld) of %lld", c, (long long)chunk_off[c], (long long)chunk_off[c + 1], (long long)n_reads);
	if (n_chunks == 0) return KG_OK;
	// (device buffers of this call alone, freed on every way out)
	struct Buffers {
		kg_aln_record *records = nullptr;
		int64_t *chunk_off = nullptr;
		uint32_t *rows = nullptr;
		~Buffers() { for (void *p : {(void *)records, (void *)chunk_off, (void *)rows}) if (p) (void)hipFree(p); }
	} d;
	const size_t row_bytes = 4 * (size_t)KG_STATS_WORDS * (size_t)n_chunks;
	HIP_TRY(hipMalloc((void **)&d.records, sizeof(kg_aln_record) * (size_t)std::max<int64_t>(n_records, 1)));
	HIP_TRY(hipMalloc((void **)&d.chunk_off, 8 * (size_t)(n_chunks + 1)));
	HIP_TRY(hipMalloc((void **)&d.rows, row_bytes));
	if (n_records > 0) HIP_TRY(hipMemcpy(d.records, records, sizeof(kg_aln_record) * (size_t)n_records, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d.chunk_off, chunk_off, 8 * (size_t)(n_chunks + 1), hipMemcpyHostToDevice));
	StatsArgs t{};
	t.records = d.records;
	t.n_reads = n_reads; t.n_records = n_records;
	t.chunk_off = d.chunk_off; t.n_chunks = n_chunks;
	t.rows = d.rows;
	HIP_TRY(launch_stats_tally(t, nullptr));
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(rows, d.rows, row_bytes, hipMemcpyDeviceToHost));
	return KG_OK;
}

int kg_stream_timing(kg_stream *s, kg_stream_timing_t *out, int reset)
{
	if (!s || !out) return fail(KG_ERR_ARG, "kg_stream_timing: null argument");
	std::lock_guard<std::mutex> lk(s->mu);
	*out = s->total;
	if (reset) s->total = kg_stream_timing_t{};
	return KG_OK;
}

}  // extern "C"
