// align_kernels.hip -- the per-read report on the device (gfx950): pairing, normal pairs, gap closing, CIGAR, flags, MAPQ.
//
// Replaces, for the short-read configuration (neither -pacbio nor -m) and per batch, what ReadMapping() does for every read
// between chaining and the SAM text (reference src/Mapping.cpp:542-578):
//   aln_pair_kernel   CheckPairedAlignmentCandidates, RemoveUnMatedAlignmentCandidates, RemoveRedundantCandidates
//                     (src/Mapping.cpp:317-427); one read pair per lane.
//   aln_plan_kernel   GenMappingReport pass 1 (src/AlignmentCandidates.cpp:624-745), one candidate per lane: IdentifyNormalPairs
//                     with RemoveTandemRepeatSeeds / RemoveTranslocatedSeeds / CheckOverlappingSeeds (:226-490),
//                     CheckCoordinateValidity (:582-610), and for every normal pair the decisions of
//                     Process{Head,Normal,Tail}SequencePair that need no alignment (src/tools.cpp:225-253, 292-312, 344-363):
//                     pure insertion / deletion, the <= 2-mismatch shortcut against the 2-bit text, the long-end soft clip, the
//                     1 x 1 gap.  A pair that needs nw_alignment becomes a job descriptor for the NW kernels (nw_kernels.hip read
//                     the read characters and the 2-bit text in place); the candidate is then parked in a spill slot.  A
//                     candidate without jobs is reported right here (report_job_free_candidate).
//   aln_finish_group_kernel  pass 2 for the parked candidates, eight lanes per candidate: CheckLocalAlignmentQuality, the leading /
//                     trailing gap trimming of the head and tail pairs, AddNewCigarElements (src/tools.cpp:49-104, 255-290, 314-339,
//                     366-394) over the op strings.
//   aln_final_kernel  best / second best (src/AlignmentCandidates.cpp:724-740), CheckPairedFinalAlignments,
//                     Set{Paired,Single}AlignmentFlag, EvaluateMAPQ (src/Mapping.cpp:49-175, 429-480) and what
//                     Output{Paired,Singled}Alignments print (:177-315) as one kg_aln_record per read, plus the chunk's
//                     contribution to iPaired / iDistance and its EstDistance validity interval.
// Integer work throughout; MAPQ's one libm expression comes from a table the host fills with its own log().  No MFMA: there is
// no contraction here.  Anything outside the envelope (mate rescue, 8-mer partition of long fragments, > 12 seeds, > 47 CIGAR
// characters) marks the read pair for the host path instead.
// The kernels live in three units -- align_pair.hip (the kernels that take a pair per lane: the reset, pairing and rescue, the final pass), align_plan.hip, align_finish.hip, the helpers they share in
// align_device.hpp --; this unit holds the stage's two entry points.
#include "align_launch.hpp"

namespace kg {

hipError_t launch_align_front(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	launch_aln_reset(a, n_cu, stream);
	if (a.slow_pairs) {
		kt_begin(KT_ALN_TRIVIAL, stream);
		launch_aln_trivial(a, n_cu, stream);
		kt_end(KT_ALN_TRIVIAL, stream);
	}
	kt_begin(KT_ALN_PAIR, stream);
	launch_aln_pair(a, n_cu, stream);
	kt_end(KT_ALN_PAIR, stream);
	kt_begin(KT_ALN_RESCUE, stream);
	launch_aln_rescue(a, n_cu, stream);
	kt_end(KT_ALN_RESCUE, stream);
	if (a.n_cands > 0) {
		if (a.plan_order) launch_aln_bin(a, n_cu, stream);
		kt_begin(KT_ALN_PLAN_FAST, stream);
		if (a.plan_slow) launch_aln_plan_fast(a, n_cu, stream);
		kt_end(KT_ALN_PLAN_FAST, stream);
		kt_begin(KT_ALN_PLAN, stream);
		launch_aln_plan(a, n_cu, stream);
		kt_end(KT_ALN_PLAN, stream);
		kt_begin(KT_ALN_PARTITION, stream);
		launch_aln_partition(a, n_cu, stream);
		kt_end(KT_ALN_PARTITION, stream);
	}
	return hipGetLastError();
}

hipError_t launch_align_back(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	kt_begin(KT_ALN_FINISH, stream);
	launch_aln_finish(a, n_cu, stream);
	kt_end(KT_ALN_FINISH, stream);
	kt_begin(KT_ALN_FINAL, stream);
	launch_aln_final(a, n_cu, stream);
	kt_end(KT_ALN_FINAL, stream);
	return hipGetLastError();
}

}  // namespace kg
