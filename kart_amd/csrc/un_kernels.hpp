// un_kernels.hpp -- argument block of the kernels that hand a batch's unmapped reads back as the text they came as (un_kernels.hip; kg_stream_set_unmapped).
//
// What `samtools fastq -f 4` (single-end) / `-f 12` (pairs) makes of a mapper's output, without the output: after kg_stream_map's report the device holds the
// input text, the record tables of its windows and the final records, so the reads that did not map are a selection, a scan and a gather of byte ranges.
#pragma once
#include "stream_kernels.hpp"

namespace kg {

// A UNIT is one read (single-end) or one pair.  Its span in file f is the bytes of its record(s) there exactly as they lie in the window: from the first byte of
// the header line through the line feed of the record's last line (FASTQ: the fourth; FASTA: the last line in front of the next header, from the FASTA record
// tables), both records of an interleaved pair in file 0.  A file whose last line has no line feed gets one.
struct UnArgs {
	FqWindow w[2];
	int two_files, paired, fasta;
	int64_t n_units;                 // n_reads / 2 for pairs
	const kg_aln_record *records;    // [n_reads ..] the reads' own records come first
	int32_t *un_len[2];              // [n_units + 1] bytes of unit u in file f: 0 where the unit is not selected or was handed back (KG_ALN_HOST)
	int64_t *un_off[2];              // [n_units + 1] exclusive scan
	uint8_t *un[2];                  // the text
	int64_t un_capacity[2];
	unsigned long long *ctl;         // [f] bytes un_copy_kernel wrote to file f (the caller holds them against un_off[f][n_units]), [2] spans that do not fit un[f]
};

// sizes of both files and their scans (scan_temp: what fq_scan_temp_bytes(n_units + 1) asks for); ctl is cleared
hipError_t launch_un_size(const UnArgs &a, void *scan_temp, size_t scan_temp_bytes, int n_cu, hipStream_t stream);
hipError_t launch_un_copy(const UnArgs &a, int n_cu, hipStream_t stream);

}  // namespace kg
