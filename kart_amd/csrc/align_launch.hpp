// align_launch.hpp -- one host function per launch step of the alignment stage, each defined in the unit that holds its kernels;
// launch_align_front / launch_align_back (align_kernels.hip) call them in the stage's order.
#pragma once
#include "align_kernels.hpp"

namespace kg {

inline int grid_for_aln(int64_t items, int block, int max_blocks)
{
	int64_t g = (items + block - 1) / block;
	if (g < 1) g = 1;
	if (g > max_blocks) g = max_blocks;
	return (int)g;
}

// align_plan.hip
void launch_aln_trivial(const AlnArgs &a, int n_cu, hipStream_t stream);
void launch_aln_bin(const AlnArgs &a, int n_cu, hipStream_t stream);           // both passes
void launch_aln_plan_fast(const AlnArgs &a, int n_cu, hipStream_t stream);
void launch_aln_plan(const AlnArgs &a, int n_cu, hipStream_t stream);
void launch_aln_partition(const AlnArgs &a, int n_cu, hipStream_t stream);
// align_pair.hip
void launch_aln_reset(const AlnArgs &a, int n_cu, hipStream_t stream);
void launch_aln_pair(const AlnArgs &a, int n_cu, hipStream_t stream);
void launch_aln_rescue(const AlnArgs &a, int n_cu, hipStream_t stream);        // the windows, then the filters behind them
void launch_aln_final(const AlnArgs &a, int n_cu, hipStream_t stream);
// align_finish.hip
void launch_aln_finish(const AlnArgs &a, int n_cu, hipStream_t stream);

}  // namespace kg
