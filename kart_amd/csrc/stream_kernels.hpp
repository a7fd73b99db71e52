// stream_kernels.hpp -- argument blocks and launchers of the FASTQ/FASTA-text-in / SAM-text-out kernels shared with the C ABI: the input side in
// read_kernels.hip, the output side in sam_kernels.hip (which launches its own kernels or those of bam_kernels.hip).
//
// The reference parses its input one record at a time on the host (GetNextEntry / GetNextChunk, src/GetData.cpp:51-143) and prints
// its output one record at a time (OutputPairedAlignments / OutputSingledAlignments, src/Mapping.cpp:177-315).  Here both ends run
// on the device, so that the host only moves bytes: the FASTQ text of a batch is uploaded as it lies in the file, the device finds
// the lines and the records, builds the read characters the seeding stage wants (mate 2 reverse-complemented), and after the
// alignment stage formats every kg_aln_record as the SAM line(s) the reference would print.
#pragma once
#include "seed_kernels.hpp"

namespace kg {

constexpr int kFqTile = 4096;            // bytes of text per block of the line-index kernels (256 threads x 16 bytes)

// why the parser stopped in front of the end of its window (kg_stream_parsed::stop)
enum { FQ_STOP_NONE = 0, FQ_STOP_IRREGULAR = 1, FQ_STOP_TAIL = 2 };

// words of the parser's control block (device, int64)
enum {
	FQM_LINES0 = 0, FQM_LINES1 = 1,      // lines found in window 0 / 1 (a last line without newline counts)
	FQM_BAD0 = 2, FQM_BAD1 = 3,          // first record of window f the device path does not take (empty read, overlong header), or INT64_MAX
	FQM_NUL = 4,                         // a NUL byte somewhere in a window (the reference treats lines as C strings)
	FQM_OVERFLOW = 5,                    // more lines than the line table holds
	FQM_READS = 6, FQM_CHUNKS = 7, FQM_BASES = 8, FQM_USED0 = 9, FQM_USED1 = 10, FQM_STOP = 11, FQM_DONE = 12,
	FQM_RECS0 = 13, FQM_RECS1 = 14,      // (FASTA) header lines = records begun in window 0 / 1
	FQM_WORDS = 16
};

struct FqWindow {
	const uint8_t *text;       // device buffer; the window is text[begin, end)
	int64_t begin, end;
	int eof;                   // the window ends where the file ends
	int32_t *tile_lines;       // [n_tiles + 1] newlines per tile, then (in place) their exclusive scan
	uint32_t *line_end;        // [line_capacity] offset (in `text`) one past each line
	int64_t line_capacity;
	// per record (four lines), capacity line_capacity / 4
	uint32_t *rec_hdr;         // offset of the header line
	uint32_t *rec_name;        // name: (offset from the header line's start) | (length << 16)   (IdentifyHeaderBegPos / EndPos)
	uint32_t *rec_seq;         // offset of the sequence line
	uint32_t *rec_qual;        // offset of the quality line
	int32_t *rec_rlen;         // sequence line length - 1
	int32_t *rec_qlen;         // min(quality line length, rlen)
	// FASTA (kg_stream_set_input): a record is a header line and every line up to the next one that starts with '>'.  There rec_seq is the
	// offset of the first sequence line, rec_qual that line's number, rec_qlen the number of sequence lines, rec_rlen the sum of (length - 1) over them
	int64_t rec_capacity;      // entries of the rec_* arrays
	uint64_t *line_acc;        // [line_capacity + 1] per line (header ? 1 : 0) << 32 | (header ? 0 : length - 1), then (in place) their exclusive scan:
	                           //   line i belongs to record (acc[i + 1] >> 32) - 1, and (uint32_t)acc[i] sequence characters lie in front of it
	uint32_t *rec_line;        // [rec_capacity + 1] the header line of every record, then the number of lines
};

struct FqArgs {
	FqWindow w[2];
	int two_files;             // mates alternate between the windows (else every read comes from window 0)
	int paired;                // the second read of every pair is held reverse-complemented (src/GetData.cpp:125-135)
	int chunk_reads;           // ReadChunkSize (4000)
	int fasta;                 // the text is FASTA (kg_stream_set_input): fa_* kernels make the record table
	int gz_lines;              // the text comes out of a gz file: records that gzgets() with its 1000-byte buffer reads differently end the batch (kg_stream_window)
	int64_t max_reads;         // capacity of the batch (a multiple of chunk_reads)
	int64_t want_reads;        // take at most this many (a multiple of chunk_reads, <= max_reads)
	int64_t *meta;             // [FQM_WORDS]
	int32_t *read_len;         // [max_reads + 1]
	int64_t *read_off;         // [max_reads + 1] exclusive scan of read_len
	uint8_t *enc;              // the reads' characters as the reference holds them
	int64_t n_reads;           // (materialise) reads of the batch, as the plan settled it
};

// what the MD:Z field needs of the index (kg_stream_set_tags; kernels/md_tag.inc): the 2-bit text, the contigs' places on its forward strand, and the holes of
// .amb (runs of one ambiguous character in the FASTA, random bases in the text), ascending
struct MdRef {
	const uint8_t *text;
	int64_t genome_size;             // bases of the forward strand
	const int64_t *chr_fwd_start;    // [n_chr]
	const int64_t *chr_len;          // [n_chr]
	int32_t n_chr, n_holes;
	const int64_t *hole_start;       // [n_holes] forward-strand coordinate of the hole's first base
	const int32_t *hole_len;         // [n_holes]
	const uint8_t *hole_char;        // [n_holes] the hole's character, upper case
};

// a kernel's last argument: the above where the kernel prints MD:Z, nothing where it does not (those kernels' arguments are what they were)
template <bool kMd> struct MdArg {};
template <> struct MdArg<true> { MdRef r; };

// the SAM text of a batch
struct SamArgs {
	FqWindow w[2];
	int two_files, paired;
	int fasta;                       // the reads have no qualities: the column is "*" (src/Mapping.cpp:186,218,234,259,280,303)
	const uint8_t *enc;
	const int64_t *read_off;
	int64_t n_reads;
	const kg_aln_record *records;    // [n_reads + extras]
	const uint8_t *chr_names;        // contig names, concatenated ...
	const int32_t *chr_name_off;     // ... [n_chr + 1]
	int32_t *sam_len;                // [n_reads + 1] bytes of text per read (0 for reads handed back)
	int64_t *sam_off;                // [n_reads + 1] exclusive scan
	uint8_t *sam;                    // the text
	int64_t sam_capacity;
	int32_t *host_list;              // reads handed back (KG_ALN_HOST), in no particular order
	unsigned long long *ctl;         // [0] entries of host_list, [1] format errors (a record whose text is not the size announced), [2] / [3] sam_checksum_kernel's sums
	// the read group of the batch (kg_stream_set_read_group), in the form the launch's format copies behind every record's last field: "\tRG:Z:<ID>" for SAM
	// lines, 'R' 'G' 'Z' <ID> NUL for BAM records; 16 readable bytes lie behind it (lane_copy).  rg_len: its bytes, 0 = none (the kRg = false kernels read neither)
	const uint8_t *rg;
	int32_t rg_len;
};

size_t fq_scan_temp_bytes(int64_t max_items);
size_t fa_scan_temp_bytes(int64_t max_lines);      // the scan over FqWindow::line_acc
// line index + record table of both windows, read lengths and their scan, the plan (meta)
hipError_t launch_fq_parse(const FqArgs &a, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream);
hipError_t launch_fq_materialise(const FqArgs &a, int n_cu, hipStream_t stream);
// the text of the batch: sizes and their scan, then the bytes; bam: BAM records in the place of the SAM lines (same arguments, same outputs:
// sam_len / sam_off / sam hold the records' bytes)
// md (may be null: none): every mapped record carries MD:Z behind XS; a.rg_len > 0: every record, unmapped ones too, carries RG:Z as its last field
hipError_t launch_text_size(const SamArgs &a, bool bam, const MdRef *md, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream);
hipError_t launch_text_format(const SamArgs &a, bool bam, const MdRef *md, int n_cu, hipStream_t stream);
hipError_t launch_sam_checksum(const SamArgs &a, int n_cu, hipStream_t stream);      // measurement aid: ctl[2] += byte sum, ctl[3] += line feeds of the text
// grouped seeding: a lane's parsed batch published as a segment of its group's batch; the lane's seed offsets cut out of the group's
hipError_t launch_group_publish(const int64_t *local_off, int64_t n, int64_t slots, int64_t enc_base, int64_t *g_off, int32_t *g_len, int n_cu, hipStream_t stream);
hipError_t launch_group_rebase(const int64_t *g_seed_off, int64_t n, int64_t first, int64_t *seed_off, int n_cu, hipStream_t stream);

}  // namespace kg
