// stats_kernels.hpp -- argument block of the kernel that tallies a batch's output records per chunk (stats_kernels.hip; kg_stream_set_stats, kg_tally_records).
//
// What `samtools flagstat` / `samtools stats` count over a mapper's output, without the output: after kg_stream_map's report the device holds the final
// records, so the run's summary is one more pass over ~112 bytes per record.
#pragma once
#include "seed_kernels.hpp"

namespace kg {

struct StatsArgs {
	const kg_aln_record *records;    // [n_records] the reads' own records come first, the records chained behind them (-m) follow
	int64_t n_reads, n_records;
	const int64_t *chunk_off;        // [n_chunks + 1] chunk c holds reads [chunk_off[c], chunk_off[c + 1])
	int n_chunks;
	uint32_t *rows;                  // [n_chunks][KG_STATS_WORDS], every word written
};

// one workgroup per chunk
hipError_t launch_stats_tally(const StatsArgs &a, hipStream_t stream);

}  // namespace kg
