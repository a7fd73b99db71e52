// align_pair.hip -- the alignment stage's kernels that take a read pair (or a single read) per lane, at both ends of the stage: aln_reset_kernel,
// aln_pair_kernel, aln_rescue_kernel, aln_post_rescue_kernel, and aln_final_kernel, which writes one record per read
// (the kernel <-> reference correspondence of the whole stage: align_kernels.hip).
#include "align_device.hpp"

namespace kg {

namespace {

// vector<AlignmentCandidate_t> of one read: the chained candidates (dense, [c0, c0 + nd)) followed by the slots of the pair's
// rescue windows ([r0, r0 + nr), mate 1 of a rescued pair only; a window that found nothing leaves a slot of score 0, which
// every consumer skips exactly like a candidate of score 0)
struct CandList {
	int64_t c0, r0;
	int nd, nr;
	__device__ __forceinline__ int n() const { return nd + nr; }
	__device__ __forceinline__ int64_t at(int i) const { return i < nd ? c0 + i : r0 + (i - nd); }
};
__device__ __forceinline__ CandList cand_list(const AlnArgs &a, int64_t r)
{
	CandList l;
	l.c0 = a.cand_off[r];
	l.nd = (int)(a.cand_off[r + 1] - l.c0);
	l.nr = a.resc_n[r];
	l.r0 = a.n_cands + (l.nr ? a.resc_off[r] : 0);
	return l;
}

// RemoveRedundantCandidates, src/Mapping.cpp:317-346 (non-PacBio)
__device__ void remove_redundant(const AlnArgs &a, const CandList &l)
{
	const int n = l.n();
	if (n <= 1) return;
	int s1 = 0, s2 = 0;
	for (int i = 0; i < n; ++i) {
		int s = a.c_score[l.at(i)];
		if (s > s2) {
			if (s >= s1) { s2 = s1; s1 = s; }
			else s2 = s;
		}
	}
	int thr = (s1 == s2 || s1 - s2 > 20) ? s1 : s2;
	for (int i = 0; i < n; ++i)
		if (a.c_score[l.at(i)] < thr) a.c_score[l.at(i)] = 0;
}

// RemoveUnMatedAlignmentCandidates, src/Mapping.cpp:402-427
__device__ void remove_unmated(const AlnArgs &a, const CandList &l1, const CandList &l2)
{
	for (int i = 0; i < l1.n(); ++i) {
		int j = a.c_mate[l1.at(i)];
		if (j == -1) a.c_score[l1.at(i)] = 0;
		else { int s = a.c_score[l1.at(i)] + a.c_score[l2.at(j)]; a.c_score[l1.at(i)] = s; a.c_score[l2.at(j)] = s; }
	}
	for (int j = 0; j < l2.n(); ++j)
		if (a.c_mate[l2.at(j)] == -1) a.c_score[l2.at(j)] = 0;
}

// ---- pairing ---------------------------------------------------------------------------------------------------------------
// one pair (or one single-end read): CheckPairedAlignmentCandidates and what follows it.  out_ck / out_lo / out_hi: the pair's
// contribution to its chunk's EstDistance validity interval (out_ck < 0: none) -- merged per wave by the kernel.
// In two halves: pair_front runs up to the point where the pair knows how many rescue windows it wants (st.nt; 0: it is done), the kernel
// reserves the task slots of the whole wave with one atomic (wave_reserve), pair_back writes the windows and finishes the pair.
struct PairState {
	int64_t a1;
	int ck, n1, n2, sc1, rl1, rl2, est_r, thr, nt;
};

// the windows of mate 1 next to the candidates of mate 2 (src/AlignmentRescue.cpp:127-165): counted (write false) or written from slot `base` on.
// Returns their number; host: a window beyond what the rescue kernel takes
__device__ __forceinline__ int rescue_windows(const AlnArgs &a, int64_t r, const PairState &st, bool write, unsigned long long base, bool &host, int &why)
{
	int k = 0;
	for (int j = 0; j < st.n2; ++j) {
		if (a.c_score[st.a1 + j] < st.thr) continue;
		int64_t pd = a.cands[st.a1 + j].posDiff;
		int64_t left = pd - st.est_r, right = pd + st.rl2;
		int it = end_lower_bound(a, right);
		if (it == a.n_ends) continue;
		int chr = a.end_chr[it];
		int64_t fs = a.chr_fwd_start[chr], rs = a.chr_rev_start[chr], cl = a.chr_len[chr];
		if (left < a.genome_size && left < (fs - cl)) left = fs - cl + 1;
		else if (right >= a.genome_size && left < (rs - cl)) left = rs - cl + 1;
		int slen = (int)(right - left);
		if (slen < st.rl1) continue;
		if (left < 0) { left = 0; slen = (int)(right - left); if (slen < st.rl1) continue; }
		if (right > a.two_genome_size) continue;
		if (slen > kRescueMaxWindow) { host = true; why = WHY_RESCUE_WINDOW; break; }
		if (write) {
			RescueTask t;
			t.left = left; t.read = (int32_t)r; t.j = j; t.slen = slen; t.score1 = st.sc1; t.ordinal = k;
			a.tasks[base + k] = t;
			int64_t slot = a.n_cands + (int64_t)(base + k);
			a.c_score[slot] = 0; a.c_mate[slot] = -1; a.c_read[slot] = (int32_t)r;
		}
		k++;
	}
	return k;
}

__device__ __forceinline__ void pair_front(const AlnArgs &a, const int64_t r, int &out_ck, long long &out_lo, long long &out_hi, PairState &st)
{
		st.nt = 0;
		const int ck = chunk_of(a, r);
		const bool paired = a.chunk_paired[ck] != 0;
		const int64_t in_chunk = r - a.chunk_off[ck];
		if (paired && (in_chunk & 1)) return;                        // the first mate's lane does the pair
		const CandList l1 = cand_list(a, r);                         // (no rescue slots yet: resc_n is zero)
		const int64_t a0 = l1.c0;
		const int n1 = l1.nd;
		for (int i = 0; i < n1; ++i) { a.c_score[a0 + i] = a.cands[a0 + i].score; a.c_mate[a0 + i] = -1; a.c_read[a0 + i] = (int32_t)r; }
		a.records[r].est_lo = -1; a.records[r].est_hi = 0x7fffffff; a.records[r].rescue = 0;
		if (!paired) {
			remove_redundant(a, l1);                                 // src/Mapping.cpp:589
			return;
		}
		a.records[r + 1].est_lo = -1; a.records[r + 1].est_hi = 0x7fffffff; a.records[r + 1].rescue = 0;
		const CandList l2 = cand_list(a, r + 1);
		const int64_t a1 = l2.c0;
		const int n2 = l2.nd;
		for (int j = 0; j < n2; ++j) { a.c_score[a1 + j] = a.cands[a1 + j].score; a.c_mate[a1 + j] = -1; a.c_read[a1 + j] = (int32_t)(r + 1); }
		if ((int64_t)n1 * n2 > kAlnPairProduct) { flag_host(a, r, WHY_PAIR_PRODUCT); return; }
		// CheckPairedAlignmentCandidates, src/Mapping.cpp:348-400
		if (n1 * n2 > 1000) { remove_redundant(a, l1); remove_redundant(a, l2); }
		bool pairing = false;
		long long lo = -1, hi = 0x7fffffffffffffffll;
		const long long est = a.est_distance;
		for (int i = 0; i < n1; ++i) {
			if (a.c_score[a0 + i] == 0) continue;
			const int64_t pd1 = a.cands[a0 + i].posDiff;
			int best = -1, s = 0;
			for (int j = 0; j < n2; ++j) {
				int sj = a.c_score[a1 + j];
				int64_t pd2 = a.cands[a1 + j].posDiff;
				if (sj == 0 || pd2 < pd1) continue;
				long long dist = pd2 - pd1;
				if (dist < est) {
					if (dist > lo) lo = dist;
					if (sj > s) { best = j; s = sj; }
					else if (sj == s) best = -1;
				} else if (dist < hi) hi = dist;
			}
			if (s > 0 && best != -1) {
				int j = best;
				int mj = a.c_mate[a1 + j];
				if (mj == -1) {
					pairing = true;
					a.c_mate[a0 + i] = j;
					a.c_mate[a1 + j] = i;
				} else if (a.c_score[a0 + i] > a.c_score[a0 + mj]) {
					a.c_mate[a0 + mj] = -1;
					a.c_mate[a0 + i] = j;
					a.c_mate[a1 + j] = i;
				}
			}
		}
		out_ck = ck; out_lo = lo; out_hi = hi;                       // (into the chunk's interval by the caller: one atomic pair per wave)
		{
			// the pair's own interval (every distance that matters is far below 2^31: EstDistance never exceeds 1.5 x 10000)
			int32_t plo = (int32_t)lo, phi = hi > 0x7fffffffll ? 0x7fffffff : (int32_t)hi;
			a.records[r].est_lo = plo; a.records[r].est_hi = phi;
			a.records[r + 1].est_lo = plo; a.records[r + 1].est_hi = phi;
		}
		if (pairing) remove_unmated(a, l1, l2);
		else {
			// RescueUnpairedAlignment is due (src/Mapping.cpp:559-560; src/AlignmentRescue.cpp:73-170)
			a.chunk_stats[ck].rescue_wanted = 1;
			a.records[r].rescue = 1; a.records[r + 1].rescue = 1;
			int sc1 = 0, sc2 = 0;
			for (int i = 0; i < n1; ++i) sc1 = max(sc1, a.c_score[a0 + i]);
			for (int j = 0; j < n2; ++j) sc2 = max(sc2, a.c_score[a1 + j]);
			const int rl1 = (int)(a.read_off[r + 1] - a.read_off[r]), rl2 = (int)(a.read_off[r + 2] - a.read_off[r + 1]);
			int strategy;
			if (sc1 == 0 && sc2 == 0) strategy = 0;                                            // :83 returns at once
			else if (sc1 < (int)(rl1 * 0.1) && sc2 < (int)(rl2 * 0.1)) strategy = 4;          // :84: neither direction is tried
			else if (sc1 > sc2 && sc1 - sc2 > 50) strategy = 1;
			else if (sc2 > sc1 && sc2 - sc1 > 50) strategy = 2;
			else strategy = 3;
			const int est_r = a.est_distance > a.max_insert ? a.max_insert : a.est_distance;   // :95
			bool host = false;
			int why = 0;
			if (strategy == 1 || strategy == 3) {
				// mate 2 next to the candidates of mate 1 (:97-125).  The right end of that window is clamped against the START
				// of the contig (:111-112), which collapses it: the "slen < rlen" test skips it.  Verified per window here; a
				// window that would be scanned after all goes to the host.
				int thr = sc1 - 30;
				if (thr < 50) thr = 50;
				for (int i = 0; i < n1 && !host; ++i) {
					if (a.c_score[a0 + i] < thr) continue;
					int64_t left = a.cands[a0 + i].posDiff, right = left + est_r + rl2;
					int it = end_lower_bound(a, left);
					if (it == a.n_ends) continue;
					int chr = a.end_chr[it];
					if (right < a.genome_size && right > a.chr_fwd_start[chr]) right = a.chr_fwd_start[chr] - 1;
					else if (right >= a.genome_size && right > a.chr_rev_start[chr]) right = a.chr_rev_start[chr] - 1;
					int slen = (int)(right - left);
					if (slen < rl2) continue;
					if (left < 0 || right > a.two_genome_size) continue;
					host = true; why = WHY_RESCUE_DIR1;
				}
			}
			int nt = 0;
			if (!host && (strategy == 2 || strategy == 3)) {
				// mate 1 next to the candidates of mate 2 (:127-165): one task per window -- counted here, written by pair_back
				st.a1 = a1; st.ck = ck; st.n1 = n1; st.n2 = n2; st.sc1 = sc1; st.rl1 = rl1; st.rl2 = rl2; st.est_r = est_r;
				st.thr = sc2 - 30;                        // (nothing was appended to mate 2's list above)
				if (st.thr < 50) st.thr = 50;
				nt = rescue_windows(a, r, st, false, 0, host, why);
				if (!host && nt > 200) { host = true; why = WHY_CAPACITY; }
			}
			if (host) { a.resc_n[r] = 0; flag_host(a, r, why); return; }
			if (nt > 0) { st.nt = nt; return; }                    // the windows are written once the wave has its task slots (pair_back)
		}
		remove_redundant(a, l1);                                     // src/Mapping.cpp:563
		remove_redundant(a, l2);
}

// a pair with st.nt rescue windows, task slots [base, base + nt) reserved
__device__ __forceinline__ void pair_back(const AlnArgs &a, const int64_t r, const PairState &st, unsigned long long base)
{
	bool host = false;
	int why = 0;
	if (base + (unsigned long long)st.nt > (unsigned long long)a.task_capacity) { host = true; why = WHY_CAPACITY; }
	else {
		(void)rescue_windows(a, r, st, true, base, host, why);
		a.resc_off[r] = (int32_t)base; a.resc_n[r] = (uint8_t)st.nt;
		// the 8-mer code skips 'N' and maps everything else through nst_nt4_table (src/KmerAnalysis.cpp:25-32, 56-102);
		// the kernel compares 2-bit codes, which is the same thing for reads made of A/C/G/T in either case
		if (st.rl1 > kRescueMaxRead || st.rl1 < 8) { host = true; why = WHY_RESCUE_READ; }
		const uint8_t *rd = a.enc + a.read_off[r];
		for (int i0 = 0; i0 < st.rl1 && !host; i0 += 8) {          // (eight characters per load: the character array has 64 bytes of slack)
			const uint64_t w = reinterpret_cast<const AlnU64u *>(rd + i0)->v;
			const int m = st.rl1 - i0 < 8 ? st.rl1 - i0 : 8;
			for (int i = 0; i < m; ++i) {
				unsigned u = (unsigned)((w >> (8 * i)) & 0xDFu);
				if (!(u == 'A' || u == 'C' || u == 'G' || u == 'T')) { host = true; why = WHY_RESCUE_READ; }
			}
		}
	}
	if (host) { a.resc_n[r] = 0; flag_host(a, r, why); return; }
	a.r_pending[r] = 1;                                              // filters follow once the windows are scanned (aln_post_rescue_kernel)
}

// ---- the same for a pair with MANY candidates, the whole wave on it ----------------------------------------------------------------
// A pair out of a repeat family comes with tens of candidates per mate: CheckPairedAlignmentCandidates is a loop over n1 x n2 of them, the
// filters and the rescue windows loops over each list, every step a dependent trip to the per-candidate arrays -- and a wave costs what its
// heaviest lane costs (64 consecutive pairs of the hg38-sized workload: the heaviest lane carries tens of times the wave's mean, tools/cand_histogram.py).
// Pairs above kPairHeavy candidate pairs are therefore taken out of the lanes' loop and done by the wave together, one after the other:
// lane j holds candidate j of a list (j + 64, ... where a list is longer), the inner loop of :362-391 is one step per candidate of mate 1 --
// the best score among the admissible candidates of mate 2 and whether a single one reaches it, by wave reductions; the order in which the
// reference walks mate 2's list does not matter for that --, the mate book-keeping stays sequential in the candidates of mate 1 as in
// the reference (a later candidate may take an earlier one's mate, :381-388).  Same arrays, same results as pair_front / pair_back.
constexpr int kPairHeavy = 32;

// RemoveRedundantCandidates (src/Mapping.cpp:317-346), the wave on one list
__device__ void remove_redundant_wave(const AlnArgs &a, const CandList &l)
{
	const int n = l.n(), lane = threadIdx.x & 63;
	if (n <= 1) return;
	int s1 = 0, s2 = 0;
	for (int i = lane; i < n; i += 64) {
		const int s = a.c_score[l.at(i)];
		if (s > s2) {
			if (s >= s1) { s2 = s1; s1 = s; }
			else s2 = s;
		}
	}
	for (int off = 32; off > 0; off >>= 1) {                // the two largest of the union (a value twice: both)
		const int b1 = __shfl_xor(s1, off), b2 = __shfl_xor(s2, off);
		const int hi = s1 > b1 ? s1 : b1, lo = s1 > b1 ? b1 : s1, rest = s2 > b2 ? s2 : b2;
		s1 = hi; s2 = lo > rest ? lo : rest;
	}
	const int thr = (s1 == s2 || s1 - s2 > 20) ? s1 : s2;
	for (int i = lane; i < n; i += 64)
		if (a.c_score[l.at(i)] < thr) a.c_score[l.at(i)] = 0;
	wave_sync_mem();
}

// rescue_windows, lanes over the candidates of mate 2 (ordinals in list order, as the loop of :127-165 hands them out)
__device__ int rescue_windows_wave(const AlnArgs &a, int64_t r, const PairState &st, bool write, unsigned long long base, bool &host, int &why)
{
	const int lane = threadIdx.x & 63;
	int k_total = 0;
	for (int j0 = 0; j0 < st.n2; j0 += 64) {
		const int j = j0 + lane;
		bool valid = false, too_big = false;
		int64_t left = 0;
		int slen = 0;
		if (j < st.n2 && a.c_score[st.a1 + j] >= st.thr) {
			const int64_t pd = a.cands[st.a1 + j].posDiff;
			left = pd - st.est_r;
			const int64_t right = pd + st.rl2;
			const int it = end_lower_bound(a, right);
			if (it != a.n_ends) {
				const int chr = a.end_chr[it];
				const int64_t fs = a.chr_fwd_start[chr], rs = a.chr_rev_start[chr], cl = a.chr_len[chr];
				if (left < a.genome_size && left < (fs - cl)) left = fs - cl + 1;
				else if (right >= a.genome_size && left < (rs - cl)) left = rs - cl + 1;
				slen = (int)(right - left);
				valid = slen >= st.rl1;
				if (valid && left < 0) { left = 0; slen = (int)(right - left); valid = slen >= st.rl1; }
				if (valid && right > a.two_genome_size) valid = false;
				if (valid && slen > kRescueMaxWindow) { too_big = true; valid = false; }
			}
		}
		// (the reference's loop stops at the first window beyond the kernel's reach; whatever it had counted before, the pair is the host's)
		if (__ballot(too_big)) { host = true; why = WHY_RESCUE_WINDOW; return k_total; }
		const uint64_t mask = __ballot(valid);
		if (write && valid) {
			const int k = k_total + __popcll(mask & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
			RescueTask t;
			t.left = left; t.read = (int32_t)r; t.j = j; t.slen = slen; t.score1 = st.sc1; t.ordinal = k;
			a.tasks[base + k] = t;
			const int64_t slot = a.n_cands + (int64_t)(base + k);
			a.c_score[slot] = 0; a.c_mate[slot] = -1; a.c_read[slot] = (int32_t)r;
		}
		k_total += __popcll(mask);
	}
	return k_total;
}

// pair_front for the pair of reads (r, r + 1) of an all-paired batch, every lane of the wave in it; the results are the same in all lanes
__device__ void pair_front_wave(const AlnArgs &a, const int64_t r, int &out_ck, long long &out_lo, long long &out_hi, PairState &st)
{
	const int lane = threadIdx.x & 63;
	st.nt = 0;
	const int ck = chunk_of(a, r);
	const CandList l1 = cand_list(a, r), l2 = cand_list(a, r + 1);          // (no rescue slots yet: resc_n is zero)
	const int64_t a0 = l1.c0, a1 = l2.c0;
	const int n1 = l1.nd, n2 = l2.nd;
	for (int i = lane; i < n1; i += 64) { a.c_score[a0 + i] = a.cands[a0 + i].score; a.c_mate[a0 + i] = -1; a.c_read[a0 + i] = (int32_t)r; }
	for (int j = lane; j < n2; j += 64) { a.c_score[a1 + j] = a.cands[a1 + j].score; a.c_mate[a1 + j] = -1; a.c_read[a1 + j] = (int32_t)(r + 1); }
	if (lane == 0) {
		a.records[r].est_lo = -1; a.records[r].est_hi = 0x7fffffff; a.records[r].rescue = 0;
		a.records[r + 1].est_lo = -1; a.records[r + 1].est_hi = 0x7fffffff; a.records[r + 1].rescue = 0;
	}
	wave_sync_mem();
	if ((int64_t)n1 * n2 > kAlnPairProduct) { if (lane == 0) flag_host(a, r, WHY_PAIR_PRODUCT); return; }
	// CheckPairedAlignmentCandidates, src/Mapping.cpp:348-400
	if (n1 * n2 > 1000) { remove_redundant_wave(a, l1); remove_redundant_wave(a, l2); }
	bool pairing = false;
	long long lo = -1, hi = 0x7fffffffffffffffll;            // (lane-local until the loop is through)
	const long long est = a.est_distance;
	for (int i = 0; i < n1; ++i) {
		const int si = a.c_score[a0 + i];
		if (si == 0) continue;
		const int64_t pd1 = a.cands[a0 + i].posDiff;
		int m = 0, cnt = 0, arg = -1;                        // of this lane's candidates of mate 2: the best admissible score, how many reach it, the first that does
		for (int j = lane; j < n2; j += 64) {
			const int sj = a.c_score[a1 + j];
			const int64_t pd2 = a.cands[a1 + j].posDiff;
			if (sj == 0 || pd2 < pd1) continue;
			const long long dist = pd2 - pd1;
			if (dist < est) {
				if (dist > lo) lo = dist;
				if (sj > m) { m = sj; cnt = 1; arg = j; }
				else if (sj == m) cnt++;
			} else if (dist < hi) hi = dist;
		}
		const int s = wave_max(m);
		if (s <= 0) continue;
		const int mine = m == s ? cnt : 0;
		if (wave_sum(mine) != 1) continue;                   // two candidates of the best score: no mate for this one (:374-375)
		const int best = __shfl(arg, __ffsll((unsigned long long)__ballot(mine == 1)) - 1);
		const int mj = a.c_mate[a1 + best];
		if (mj == -1) {
			pairing = true;
			if (lane == 0) { a.c_mate[a0 + i] = best; a.c_mate[a1 + best] = i; }
		} else if (si > a.c_score[a0 + mj]) {
			if (lane == 0) { a.c_mate[a0 + mj] = -1; a.c_mate[a0 + i] = best; a.c_mate[a1 + best] = i; }
		}
		wave_sync_mem();
	}
	for (int off = 32; off > 0; off >>= 1) {
		const long long l2_ = __shfl_xor(lo, off), h2_ = __shfl_xor(hi, off);
		lo = l2_ > lo ? l2_ : lo;
		hi = h2_ < hi ? h2_ : hi;
	}
	out_ck = ck; out_lo = lo; out_hi = hi;
	if (lane == 0) {
		int32_t plo = (int32_t)lo, phi = hi > 0x7fffffffll ? 0x7fffffff : (int32_t)hi;
		a.records[r].est_lo = plo; a.records[r].est_hi = phi;
		a.records[r + 1].est_lo = plo; a.records[r + 1].est_hi = phi;
	}
	if (pairing) {
		// RemoveUnMatedAlignmentCandidates, src/Mapping.cpp:402-427 (the mates are a matching: no two candidates of mate 1 share one of mate 2)
		for (int i = lane; i < n1; i += 64) {
			const int j = a.c_mate[a0 + i];
			if (j == -1) a.c_score[a0 + i] = 0;
			else { const int sum = a.c_score[a0 + i] + a.c_score[a1 + j]; a.c_score[a0 + i] = sum; a.c_score[a1 + j] = sum; }
		}
		wave_sync_mem();
		for (int j = lane; j < n2; j += 64)
			if (a.c_mate[a1 + j] == -1) a.c_score[a1 + j] = 0;
		wave_sync_mem();
	} else {
		// RescueUnpairedAlignment is due (src/Mapping.cpp:559-560; src/AlignmentRescue.cpp:73-170)
		if (lane == 0) { a.chunk_stats[ck].rescue_wanted = 1; a.records[r].rescue = 1; a.records[r + 1].rescue = 1; }
		int sc1 = 0, sc2 = 0;
		for (int i = lane; i < n1; i += 64) sc1 = max(sc1, a.c_score[a0 + i]);
		for (int j = lane; j < n2; j += 64) sc2 = max(sc2, a.c_score[a1 + j]);
		sc1 = wave_max(sc1); sc2 = wave_max(sc2);
		const int rl1 = (int)(a.read_off[r + 1] - a.read_off[r]), rl2 = (int)(a.read_off[r + 2] - a.read_off[r + 1]);
		int strategy;
		if (sc1 == 0 && sc2 == 0) strategy = 0;
		else if (sc1 < (int)(rl1 * 0.1) && sc2 < (int)(rl2 * 0.1)) strategy = 4;
		else if (sc1 > sc2 && sc1 - sc2 > 50) strategy = 1;
		else if (sc2 > sc1 && sc2 - sc1 > 50) strategy = 2;
		else strategy = 3;
		const int est_r = a.est_distance > a.max_insert ? a.max_insert : a.est_distance;
		bool host = false;
		int why = 0;
		if (strategy == 1 || strategy == 3) {
			// mate 2 next to the candidates of mate 1 (:97-125): a window that would be scanned after all goes to the host (pair_front)
			int thr = sc1 - 30;
			if (thr < 50) thr = 50;
			bool found = false;
			for (int i = lane; i < n1; i += 64) {
				if (a.c_score[a0 + i] < thr) continue;
				int64_t left = a.cands[a0 + i].posDiff, right = left + est_r + rl2;
				const int it = end_lower_bound(a, left);
				if (it == a.n_ends) continue;
				const int chr = a.end_chr[it];
				if (right < a.genome_size && right > a.chr_fwd_start[chr]) right = a.chr_fwd_start[chr] - 1;
				else if (right >= a.genome_size && right > a.chr_rev_start[chr]) right = a.chr_rev_start[chr] - 1;
				const int slen = (int)(right - left);
				if (slen < rl2) continue;
				if (left < 0 || right > a.two_genome_size) continue;
				found = true;
			}
			if (__ballot(found)) { host = true; why = WHY_RESCUE_DIR1; }
		}
		int nt = 0;
		if (!host && (strategy == 2 || strategy == 3)) {
			st.a1 = a1; st.ck = ck; st.n1 = n1; st.n2 = n2; st.sc1 = sc1; st.rl1 = rl1; st.rl2 = rl2; st.est_r = est_r;
			st.thr = sc2 - 30;
			if (st.thr < 50) st.thr = 50;
			nt = rescue_windows_wave(a, r, st, false, 0, host, why);
			if (!host && nt > 200) { host = true; why = WHY_CAPACITY; }
		}
		if (host) { if (lane == 0) { a.resc_n[r] = 0; flag_host(a, r, why); } return; }
		if (nt > 0) { st.nt = nt; return; }
	}
	remove_redundant_wave(a, l1);
	remove_redundant_wave(a, l2);
}

__device__ void pair_back_wave(const AlnArgs &a, const int64_t r, const PairState &st, unsigned long long base)
{
	const int lane = threadIdx.x & 63;
	bool host = false;
	int why = 0;
	if (base + (unsigned long long)st.nt > (unsigned long long)a.task_capacity) { host = true; why = WHY_CAPACITY; }
	else {
		(void)rescue_windows_wave(a, r, st, true, base, host, why);
		if (lane == 0) { a.resc_off[r] = (int32_t)base; a.resc_n[r] = (uint8_t)st.nt; }
		if (st.rl1 > kRescueMaxRead || st.rl1 < 8) { host = true; why = WHY_RESCUE_READ; }
		const uint8_t *rd = a.enc + a.read_off[r];
		bool bad = false;
		for (int i = lane; i < st.rl1 && !host; i += 64) {
			const unsigned u = rd[i] & 0xDFu;
			bad = bad || !(u == 'A' || u == 'C' || u == 'G' || u == 'T');
		}
		if (__ballot(bad)) { host = true; why = WHY_RESCUE_READ; }
	}
	if (lane != 0) return;
	if (host) { a.resc_n[r] = 0; flag_host(a, r, why); return; }
	a.r_pending[r] = 1;
}

}  // namespace

// One PAIR per lane (one read per lane where a chunk is not paired).  Rounds 2-3 ran one READ per lane and let the second mate's lane
// leave at once -- half of every wave idle -- and sent two same-address atomics per pair at the chunk's interval (2000 pairs per
// chunk: a wave's 64 lanes hit one address); now a wave whose pairs lie in one chunk sends one pair of atomics, the rescue
// windows of the wave's pairs take their task slots with one atomic, and the pairs with many candidates are the whole wave's.
__global__ __launch_bounds__(256) void aln_pair_kernel(AlnArgs a)
{
	// (a.slow_pairs: the pairs aln_trivial_kernel did not decide, ctl[35] of them; else every pair / read of the batch)
	const int64_t n_units = a.slow_pairs ? (int64_t)a.ctl[35] : a.all_paired ? a.n_reads >> 1 : a.n_reads;
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int lane = threadIdx.x & 63;
	const bool heavy_on = a.all_paired && !a.dbg_no_heavy;
	for (int64_t u0 = (int64_t)blockIdx.x * blockDim.x; u0 < n_units; u0 += stride) {
		const int64_t u = u0 + threadIdx.x;
		int ck = -1;
		long long lo = -1, hi = 0x7fffffffffffffffll;
		PairState st;
		st.nt = 0;
		const int64_t r = u < n_units ? (a.slow_pairs ? (int64_t)a.slow_pairs[u] << 1 : a.all_paired ? u << 1 : u) : 0;
		bool heavy = false;
		if (u < n_units && heavy_on) {
			const int64_t c0 = a.cand_off[r], c1 = a.cand_off[r + 1], c2 = a.cand_off[r + 2];
			heavy = (c1 - c0) * (c2 - c1) > (int64_t)a.pair_heavy;
		}
		if (u < n_units && !heavy) pair_front(a, r, ck, lo, hi, st);
		uint64_t hm = __ballot(heavy);
		while (hm) {
			const int src = __ffsll((unsigned long long)hm) - 1;
			hm &= hm - 1;
			const int64_t rh = ((int64_t)__shfl((int)(uint32_t)((uint64_t)r >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)(uint64_t)r, src);
			int ck_h = -1;
			long long lo_h = -1, hi_h = 0x7fffffffffffffffll;
			PairState st_h;
			pair_front_wave(a, rh, ck_h, lo_h, hi_h, st_h);
			if (lane == src) { ck = ck_h; lo = lo_h; hi = hi_h; st = st_h; }
		}
		const unsigned long long base = wave_reserve(&a.ctl[4], (unsigned long long)st.nt);
		if (st.nt > 0 && !heavy) pair_back(a, r, st, base);
		hm = __ballot(heavy && st.nt > 0);
		while (hm) {
			const int src = __ffsll((unsigned long long)hm) - 1;
			hm &= hm - 1;
			const int64_t rh = ((int64_t)__shfl((int)(uint32_t)((uint64_t)r >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)(uint64_t)r, src);
			PairState st_h;
			st_h.a1 = ((int64_t)__shfl((int)(uint32_t)((uint64_t)st.a1 >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)(uint64_t)st.a1, src);
			st_h.ck = __shfl(st.ck, src); st_h.n1 = __shfl(st.n1, src); st_h.n2 = __shfl(st.n2, src); st_h.sc1 = __shfl(st.sc1, src);
			st_h.rl1 = __shfl(st.rl1, src); st_h.rl2 = __shfl(st.rl2, src); st_h.est_r = __shfl(st.est_r, src); st_h.thr = __shfl(st.thr, src); st_h.nt = __shfl(st.nt, src);
			const unsigned long long bh = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)base, src);
			pair_back_wave(a, rh, st_h, bh);
		}
		// ---- the chunk's interval: lo = max over the pairs, hi = min ----
		const uint64_t have = __ballot(ck >= 0);
		if (have == 0) continue;
		const int ck0 = __shfl(ck, __ffsll((unsigned long long)have) - 1);
		if (__ballot(ck >= 0 && ck != ck0) == 0) {
			for (int off = 32; off > 0; off >>= 1) {
				const long long l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
				lo = l2 > lo ? l2 : lo;
				hi = h2 < hi ? h2 : hi;
			}
			if ((threadIdx.x & 63) == 0) {
				if (lo > -1) atomicMax((long long *)&a.chunk_stats[ck0].lo, lo);
				if (hi != 0x7fffffffffffffffll) atomicMin((long long *)&a.chunk_stats[ck0].hi, hi);
			}
		} else if (ck >= 0) {
			if (lo > -1) atomicMax((long long *)&a.chunk_stats[ck].lo, lo);
			if (hi != 0x7fffffffffffffffll) atomicMin((long long *)&a.chunk_stats[ck].hi, hi);
		}
	}
}

// ---- mate rescue: one wave per window ----------------------------------------------------------------------------------------
// IdentifyCommonKmers + GenerateSimplePairsFromCommonKmers(10) over a window (src/KmerAnalysis.cpp:104-162) produce, per diagonal,
// the maximal runs of consecutive common 8-mers = the maximal exact matches of at least 10 bases between the read and the window
// along that diagonal, sorted by (diagonal, read position).  The kernel finds those runs directly: every lane takes a block of
// consecutive diagonals and XORs 2-bit packed read words against the window shifted to that diagonal.
// IdnetifyRescueCandidate (src/AlignmentRescue.cpp:24-69) then groups consecutive runs whose diagonals lie within MaxGaps of
// the group's first one and keeps the first group of the largest total length.
__global__ __launch_bounds__(64) void aln_rescue_kernel(AlnArgs a)
{
	__shared__ uint64_t rd2[kRescueMaxRead / 32 + 2];          // read, 2 bits per base, base t in bits 2*(t&31) of word t>>5
	__shared__ uint64_t win2[kRescueMaxWindow / 32 + 4];       // window likewise
	__shared__ int raw_key[kRescueMaxRuns], raw_len[kRescueMaxRuns];      // runs as the lanes find them: (diagonal index << 8 | read position), length
	__shared__ int run_d[kRescueMaxRuns], run_t[kRescueMaxRuns], run_l[kRescueMaxRuns];   // ... sorted by (diagonal, read position)
	__shared__ int n_raw;
	__shared__ int kh_head[512], kh_next[kRescueMaxRead];           // the read's 10-mers: hash slot -> chain of read positions
	__shared__ uint32_t kh_key[kRescueMaxRead];
	const int lane = threadIdx.x;
	unsigned long long n_tasks = a.ctl[4];
	if (n_tasks > (unsigned long long)a.task_capacity) n_tasks = (unsigned long long)a.task_capacity;
	for (unsigned long long ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
		const RescueTask t = a.tasks[ti];
		const int64_t slot = a.n_cands + (int64_t)ti;
		if (a.r_host[t.read]) continue;                            // (uniform per block)
		const int rlen = (int)(a.read_off[t.read + 1] - a.read_off[t.read]);
		const uint8_t *rd = a.enc + a.read_off[t.read];
		const int slen = t.slen;
		const int rwords = (rlen + 31) >> 5, wwords = (slen + 31) >> 5;
		__syncthreads();
		// the read as 2-bit codes, 64 bases per step: every lane converts one character (A 00, C 01, G 11, T 10 in either case
		// is one Gray step from the codes 0..3), two ballots collect the bit planes, which are then interleaved
		for (int w2 = 0; (w2 << 6) < rlen + 32; ++w2) {
			int p = (w2 << 6) + lane;
			unsigned g = 0;
			if (p < rlen) { unsigned ch = rd[p]; g = (ch >> 1) & 3; g ^= g >> 1; }
			uint64_t m0 = __ballot(g & 1), m1 = __ballot(g & 2);
			if (lane < 2) {
				uint32_t lo0 = (uint32_t)(m0 >> (lane << 5)), lo1 = (uint32_t)(m1 >> (lane << 5));
				auto spread = [](uint32_t v) {
					uint64_t x = v;
					x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
					x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
					x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
					x = (x | (x << 2)) & 0x3333333333333333ull;
					x = (x | (x << 1)) & 0x5555555555555555ull;
					return x;
				};
				int w = (w2 << 1) + lane;
				if (w < rwords + 1) rd2[w] = spread(lo0) | (spread(lo1) << 1);
			}
		}
		// the window straight from the 2-bit text (same packing: base i in bits 2 (i & 3) of byte i >> 2): one unaligned 64-bit
		// load + the next byte per word
		for (int w = lane; w < wwords + 2; w += 64) {
			int64_t g0 = t.left + ((int64_t)w << 5);
			uint64_t x = 0;
			if ((w << 5) < slen) {
				const uint8_t *tp = a.ix.text + ((uint64_t)g0 >> 2);
				uint64_t lo_w = 0;
				for (int k = 0; k < 8; ++k) lo_w |= (uint64_t)tp[k] << (k << 3);
				uint64_t hi_b = tp[8];
				int sh = ((int)g0 & 3) << 1;
				x = sh ? (lo_w >> sh) | (hi_b << (64 - sh)) : lo_w;
				int valid = slen - (w << 5);
				if (valid < 32) x &= (1ull << (valid << 1)) - 1;
			}
			win2[w] = x;
		}
		if (lane == 0) n_raw = 0;
		__syncthreads();
		// diagonals d = gpos - rpos of k-mer pairs: -(rlen - 8) .. slen - 8
		const int d_lo = -(rlen - 8), nd = slen + rlen - 15;
		if (!a.dbg_rescue_scan) {
			// Round 4: the runs through the read's 10-mers.  Every maximal exact match of >= 10 bases starts with a common 10-mer whose
			// predecessor pair differs (or does not exist): the read's <= 247 10-mers go into a 512-slot LDS hash, every lane looks the
			// window's 10-mers up (26 positions per lane for a 1650-base window), and a hit that starts a run is extended 32 bases per
			// step.  The scan below walked all ~1800 diagonals of the window, 8 words each (87 G VALU wave-instructions per 80 M
			// reads, 54 % of the kernel's cycles waiting on its own issue, profiles/r03w); the same runs come out (rank-sorted afterwards).
			auto bits_at = [](const uint64_t *v, int pos) -> uint64_t {        // 32 bases from base `pos` (2 bits each)
				const int w = pos >> 5, sh = (pos & 31) << 1;
				return sh ? (v[w] >> sh) | (v[w + 1] << (64 - sh)) : v[w];
			};
			for (int i = lane; i < 512; i += 64) kh_head[i] = -1;
			__syncthreads();
			for (int q = lane; q + 10 <= rlen; q += 64) {
				const uint32_t key = (uint32_t)(bits_at(rd2, q) & 0xFFFFFull);
				kh_key[q] = key;
				kh_next[q] = atomicExch(&kh_head[(key * 0x9E3779B1u) >> 23], q);
			}
			__syncthreads();
			for (int w = lane; w + 10 <= slen; w += 64) {
				const uint32_t key = (uint32_t)(bits_at(win2, w) & 0xFFFFFull);
				for (int q = kh_head[(key * 0x9E3779B1u) >> 23]; q >= 0; q = kh_next[q]) {
					if (kh_key[q] != key) continue;
					if (q > 0 && w > 0 && ((((rd2[(q - 1) >> 5] >> (((q - 1) & 31) << 1)) ^ (win2[(w - 1) >> 5] >> (((w - 1) & 31) << 1))) & 3) == 0)) continue;   // not where the run starts
					const int room = rlen - q < slen - w ? rlen - q : slen - w;
					int e = 0;
					while (e < room) {
						const uint64_t diff = bits_at(rd2, q + e) ^ bits_at(win2, w + e);
						const uint64_t ne = (diff | (diff >> 1)) & 0x5555555555555555ull;
						if (ne) { e += (__ffsll((unsigned long long)ne) - 1) >> 1; break; }
						e += 32;
					}
					if (e > room) e = room;
					const int at_ = atomicAdd(&n_raw, 1);
					if (at_ < kRescueMaxRuns) { raw_key[at_] = ((w - q - d_lo) << 8) | q; raw_len[at_] = e; }
				}
			}
		} else {
		const int per = (nd + 63) >> 6;
		// per diagonal: the equality bit of every read position (one bit per base, up to 256), then the positions where ten
		// consecutive bits are set by shift-and doubling; almost every diagonal ends there with nothing set
		for (int q = 0; q < per; ++q) {
			int di = lane * per + q;
			if (di >= nd) break;
			int d = d_lo + di;
			int t_lo = d < 0 ? -d : 0;
			int t_hi = rlen < slen - d ? rlen : slen - d;               // read positions [t_lo, t_hi) face window positions t + d
			uint64_t E[4] = {0, 0, 0, 0};
#pragma unroll
			for (int w = 0; w < kRescueMaxRead / 32; ++w) {                // (fixed trip count: E[] stays in registers)
				int base = w << 5;
				if (base >= t_hi || base + 32 <= t_lo) continue;
				int wp = base + d;                                      // window position facing read position `base` (negative: masked below)
				int idx = wp >> 5;                                      // floor division (arithmetic shift)
				int sh = (wp & 31) << 1;
				uint64_t lo_w = idx >= 0 ? win2[idx] : 0, hi_w = idx + 1 >= 0 ? win2[idx + 1] : 0;
				uint64_t ww = sh ? (lo_w >> sh) | (hi_w << (64 - sh)) : lo_w;
				uint64_t diff = rd2[w] ^ ww;
				uint64_t eq = ~(diff | (diff >> 1)) & 0x5555555555555555ull;   // bit 2b set: base b equal
				int b0 = t_lo > base ? t_lo - base : 0, b1 = t_hi - base < 32 ? t_hi - base : 32;
				eq &= (b1 >= 32 ? ~0ull : ((1ull << (b1 << 1)) - 1)) & ~((1ull << (b0 << 1)) - 1);
				// 2 bits per base -> 1 bit per base
				uint64_t x = eq;
				x = (x | (x >> 1)) & 0x3333333333333333ull;
				x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
				x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
				x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
				x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
				E[w >> 1] |= x << ((w & 1) << 5);
			}
			// R[p]: positions p .. p+9 all equal
			auto shr = [](const uint64_t *v, int k, uint64_t *o) {     // o = v >> k over 256 bits, 0 < k < 64
				o[0] = (v[0] >> k) | (v[1] << (64 - k)); o[1] = (v[1] >> k) | (v[2] << (64 - k)); o[2] = (v[2] >> k) | (v[3] << (64 - k)); o[3] = v[3] >> k;
			};
			uint64_t T[4], R2[4], R[4];
			shr(E, 1, T);
			for (int i = 0; i < 4; ++i) R2[i] = E[i] & T[i];            // >= 2
			shr(R2, 2, T);
			for (int i = 0; i < 4; ++i) R[i] = R2[i] & T[i];            // >= 4
			shr(R, 4, T);
			for (int i = 0; i < 4; ++i) R[i] &= T[i];                   // >= 8
			shr(R2, 8, T);
			for (int i = 0; i < 4; ++i) R[i] &= T[i];                   // >= 10
			if ((R[0] | R[1] | R[2] | R[3]) == 0) continue;
			// the maximal runs of at least 10: each starts at the lowest remaining bit of R
			for (;;) {
				int p = -1;
				for (int i = 0; i < 4; ++i)
					if (R[i]) { p = (i << 6) + __ffsll((unsigned long long)R[i]) - 1; break; }
				if (p < 0) break;
				int e = p + 10;                                         // extend while the bases stay equal
				while (e < 256 && ((E[e >> 6] >> (e & 63)) & 1)) e++;
				int at_ = atomicAdd(&n_raw, 1);
				if (at_ < kRescueMaxRuns) { raw_key[at_] = (di << 8) | p; raw_len[at_] = e - p; }
				for (int c = p; c < e; ++c) R[c >> 6] &= ~(1ull << (c & 63));   // (positions of this run cannot start another)
			}
		}
		}
		// the runs in (diagonal, read position) order -- the order IdentifyCommonKmers' sort leaves the k-mer hits in: rank sort
		__syncthreads();
		const int total = n_raw;
		if (total > kRescueMaxRuns) {
			if (lane == 0) flag_host(a, t.read, WHY_RESCUE_RUNS);
			continue;
		}
		for (int i = lane; i < total; i += 64) {
			int key = raw_key[i], rank = 0;
			for (int j = 0; j < total; ++j) rank += raw_key[j] < key ? 1 : 0;
			run_d[rank] = d_lo + (key >> 8); run_t[rank] = key & 255; run_l[rank] = raw_len[i];
		}
		__syncthreads();
		if (lane == 0) {
			// IdnetifyRescueCandidate
			int best_s = 0, best_i = 0, best_j = 0;
			for (int i = 0; i < total;) {
				int s = run_l[i], j;
				for (j = i + 1; j < total; ++j) {
					if (run_d[j] - run_d[i] < a.max_gaps) s += run_l[j];
					else break;
				}
				if (s > best_s) { best_s = s; best_i = i; best_j = j; }
				i = j;
			}
			int cnt = best_j - best_i;
			if (best_s > t.score1) {
				if (cnt > kAlnMaxSeeds) flag_host(a, t.read, WHY_RESCUE_SEEDS);
				else {
					// the group's pairs by (gPos, rPos) (:61); text coordinates
					kg_seed *out = a.resc_seeds + (int64_t)ti * kAlnMaxSeeds;
					for (int k = 0; k < cnt; ++k) {
						kg_seed sd;
						sd.rPos = run_t[best_i + k]; sd.len = run_l[best_i + k]; sd.gPos = t.left + run_t[best_i + k] + run_d[best_i + k];
						int p = k;
						while (p > 0 && (out[p - 1].gPos > sd.gPos || (out[p - 1].gPos == sd.gPos && out[p - 1].rPos > sd.rPos))) { out[p] = out[p - 1]; --p; }
						out[p] = sd;
					}
					a.resc_count[ti] = cnt;
					a.resc_posdiff[ti] = (int64_t)run_d[best_i] + t.left;
					// the new candidate of mate 1 is mated with candidate j of mate 2 (:158-164)
					const CandList l1 = cand_list(a, t.read);
					a.c_score[slot] = best_s;
					a.c_mate[slot] = t.j;
					a.c_mate[a.cand_off[t.read + 1] + t.j] = l1.nd + t.ordinal;
				}
			}
		}
	}
}

// what follows RescueUnpairedAlignment for the pairs that had windows (src/Mapping.cpp:561-563)
__global__ __launch_bounds__(256) void aln_post_rescue_kernel(AlnArgs a)
{
	int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int64_t n = a.slow_pairs ? (int64_t)a.ctl[35] : a.n_reads;          // (only the first mate of a pair is ever pending)
	for (; x < n; x += stride) {
		const int64_t r = a.slow_pairs ? (int64_t)a.slow_pairs[x] << 1 : x;
		if (!a.r_pending[r] || a.r_host[r]) continue;
		const CandList l1 = cand_list(a, r), l2 = cand_list(a, r + 1);
		bool mated = false;
		for (int i = l1.nd; i < l1.n(); ++i) mated = mated || a.c_score[l1.at(i)] > 0;
		if (mated) remove_unmated(a, l1, l2);
		remove_redundant(a, l1);
		remove_redundant(a, l2);
	}
}

// ---- per read: best / second best, final pair check, flags, MAPQ, records ----------------------------------------------------
namespace {

struct ReadSum {                    // the ReadItem_t fields the output depends on
	int score, sub_score, best, can_num, mapq, rlen;
	CandList l;
};

// the tail of GenMappingReport's loop, src/AlignmentCandidates.cpp:724-740 (bMultiHit false)
__device__ void summarise(const AlnArgs &a, int64_t r, ReadSum &s)
{
	s.l = cand_list(a, r);
	s.can_num = s.l.n();
	s.rlen = (int)(a.read_off[r + 1] - a.read_off[r]);
	s.score = s.sub_score = s.best = 0;
	s.mapq = 0;
	for (int i = 0; i < s.can_num; ++i) {
		int cs = a.c_score[s.l.at(i)];
		if (cs == 0 || cs == -1) continue;                          // skipped before the comparison (Score == 0, invalid coordinates, gap penalty)
		int sc = a.rep_score[s.l.at(i)];
		if (sc > s.score) { s.best = i; s.sub_score = s.score; s.score = sc; }
		else if (sc == s.score) {
			s.sub_score = s.score;
			if (!a.multi_hit && a.chr_len[a.rep_chr[s.l.at(i)]] > a.chr_len[a.rep_chr[s.l.at(s.best)]]) s.best = i;
		}
	}
}

__device__ __forceinline__ int eval_mapq(const AlnArgs &a, const ReadSum &s)   // EvaluateMAPQ, src/Mapping.cpp:160-175
{
	if (s.score == 0 || s.score == s.sub_score) return 0;
	int q;
	const int d = s.score - s.sub_score;
	if (s.sub_score == 0 || d > 5) q = 60;
	else if (d > 0) q = a.mapq_tab[s.score * 6 + d];
	// score < sub_score happens (CheckPairedFinalAlignments can settle on a mated candidate below the read's second best): the
	// expression then exceeds 60 for every score >= 8 (30 ln 8 = 62.4); the few smaller scores are tabulated as well
	else if (s.score >= 8) q = 60;
	else q = a.mapq_tab[(kAlnMaxScore + 1) * 6 + s.score * (kAlnMaxScore + 1) + (-d)];
	return q > 60 ? 60 : q;
}

// rep[i] of a read; a read without candidates holds one empty report (score 0, mate -1, forward; :627-634)
__device__ __forceinline__ int rep_score_at(const AlnArgs &a, const ReadSum &s, int i) { return (s.can_num == 0) ? 0 : a.rep_score[s.l.at(i)]; }
__device__ __forceinline__ int rep_mate_at(const AlnArgs &a, const ReadSum &s, int i) { return (s.can_num == 0) ? -1 : a.c_mate[s.l.at(i)]; }
__device__ __forceinline__ bool rep_fwd_at(const AlnArgs &a, const ReadSum &s, int i) { return (s.can_num == 0) ? true : a.rep_fwd[s.l.at(i)] != 0; }

// the per-mate halves of SetPairedAlignmentFlag, src/Mapping.cpp:96-156: the flag of the record that can be printed for `me`
// (its best candidate), or of the unmapped record
__device__ int one_mate_flag(const AlnArgs &a, const ReadSum &me, const ReadSum &other, int base)
{
	if (me.score > 0) {                                            // (score > sub_score and score == sub_score > 0 set the best candidate's flag alike)
		if (me.score <= me.sub_score && rep_score_at(a, me, me.best) <= 0) return 0;   // not assigned; such a record is never printed
		int f = base | (rep_fwd_at(a, me, me.best) ? 0x20 : 0x10);
		int j = rep_mate_at(a, me, me.best);
		if (j != -1 && rep_score_at(a, other, j) > 0) f |= 0x2;
		else f |= 0x8;
		return f;
	}
	int f = base | 0x4;
	if (other.score == 0) f |= 0x8;
	else f |= (rep_fwd_at(a, other, other.best) ? 0x10 : 0x20);
	return f;
}

// record slot `at` (the read's own slot, or one of the extra slots of -m) for candidate `cand_i` of the read
__device__ void write_record_at(const AlnArgs &a, int64_t at, const ReadSum &s, int cand_i, int kind, int flag, bool has_mate, int64_t mate_pos, int tlen, bool flip)
{
	kg_aln_record &o = a.records[at];
	o.kind = kind; o.flag = flag; o.mapq = s.mapq; o.score = s.score; o.sub_score = s.sub_score;
	o.has_mate = has_mate ? 1 : 0; o.mate_pos = mate_pos; o.tlen = tlen; o.flip = flip ? 1 : 0;      // (est_lo / est_hi / rescue: aln_pair_kernel)
	o.chr = -1; o.pos = 0; o.cigar_len = 0;
	o.next = -1; o.primary = cand_i == s.best ? 1 : 0; o.pad[0] = o.pad[1] = o.pad[2] = 0;
	if (kind == KG_ALN_MAPPED) {
		int64_t c = s.l.at(cand_i);
		o.chr = a.rep_chr[c]; o.pos = a.rep_pos[c];
		int n = a.rep_cigar_len[c];
		o.cigar_len = (uint8_t)n;
		// (eight characters per load and store: both sides are 8-byte aligned and KG_ALN_CIGAR_MAX long; what lies behind cigar_len is nobody's)
		const uint64_t *src = reinterpret_cast<const uint64_t *>(a.rep_cigar + c * KG_ALN_CIGAR_MAX);
		uint64_t *dst = reinterpret_cast<uint64_t *>(o.cigar);
		for (int i = 0; 8 * i < n; ++i) dst[i] = src[i];
	}
}

__device__ __forceinline__ void write_record(const AlnArgs &a, int64_t r, const ReadSum &s, int kind, int flag, bool has_mate, int64_t mate_pos, int tlen, bool flip)
{
	write_record_at(a, r, s, s.best, kind, flag, has_mate, mate_pos, tlen, flip);
}

// -m: the next record of read r goes into its own slot when that is still free, else into an extra slot chained behind `last`
// (the slot written before).  false: the extra slots are used up.
__device__ bool next_slot(const AlnArgs &a, int64_t r, int64_t &last, int64_t &at)
{
	if (last < 0) { at = r; last = r; return true; }
	unsigned long long k = atomicAdd(&a.ctl[7], 1ull);
	if (k >= (unsigned long long)a.extra_capacity) return false;
	at = a.n_reads + (int64_t)k;
	a.records[last].next = (int32_t)at;
	last = at;
	return true;
}

// SetPairedAlignmentFlag for candidate i of `me` when the run prints more than the best candidate (-m): assigned exactly where the
// reference assigns it (src/Mapping.cpp:78-93, 96-156), the unset value elsewhere
__device__ int multi_flag(const AlnArgs &a, const ReadSum &me, const ReadSum &other, int i, int base, bool both_unique, int best_flag)
{
	if (both_unique || me.score > me.sub_score) return i == me.best ? best_flag : a.unset_flag;
	// me.score == me.sub_score > 0: every candidate with a positive score is assigned
	int f = base | (rep_fwd_at(a, me, i) ? 0x20 : 0x10);
	int j = rep_mate_at(a, me, i);
	if (j != -1 && rep_score_at(a, other, j) > 0) f |= 0x2; else f |= 0x8;
	return f;
}

}  // namespace

__global__ __launch_bounds__(256) void aln_final_kernel(AlnArgs a)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int64_t n_units = a.slow_pairs ? (int64_t)a.ctl[35] : a.n_reads;          // (the pairs aln_trivial_kernel left, or every read)
	// (the wave's lanes stay together: what they add to their chunk's statistics is summed across the wave -- 64 lanes, mostly one chunk, one address)
	for (int64_t x0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); x0 < n_units; x0 += stride) {
		const int64_t x = x0 + (threadIdx.x & 63);
		int ck = -1;
		long long add_paired = 0, add_dist = 0;
		int add_unmapped = 0, add_unique = 0, add_host = 0;
		do {
		if (x >= n_units) break;
		const int64_t r = a.slow_pairs ? (int64_t)a.slow_pairs[x] << 1 : x;
		const int ck_r = chunk_of(a, r);
		const bool paired = a.chunk_paired[ck_r] != 0;
		if (paired && ((r - a.chunk_off[ck_r]) & 1)) break;
		ck = ck_r;
		if (a.r_host[r]) {
			a.records[r].kind = KG_ALN_HOST;
			if (paired) a.records[r + 1].kind = KG_ALN_HOST;
			add_host = paired ? 2 : 1;
			break;
		}
		ReadSum s1;
		summarise(a, r, s1);
		if (s1.score > kAlnMaxScore || s1.sub_score > kAlnMaxScore) {             // beyond the MAPQ table (reads longer than 2047 bases)
			atomicAdd(&a.ctl[8 + WHY_SCORE], 1ull);
			a.records[r].kind = KG_ALN_HOST;
			if (paired) a.records[r + 1].kind = KG_ALN_HOST;
			break;
		}
		if (!paired) {
			// SetSingleAlignmentFlag + EvaluateMAPQ + OutputSingledAlignments, src/Mapping.cpp:49-71, 160-175, 272-315
			s1.mapq = eval_mapq(a, s1);
			if (s1.score == 0) {
				add_unmapped = 1;
				write_record(a, r, s1, KG_ALN_UNMAPPED, 0x4, false, 0, 0, false);
			} else {
				// the candidates from `best` on whose score is the read's: the first one, or with -m all of them (:291-304); every
				// one of them carries an assigned flag (a second candidate of the read's score makes score == sub_score, :58-66)
				int64_t last = -1, at = r;
				bool full = false;
				for (int i = s1.best; i < s1.can_num && !full; ++i) {
					if (a.rep_score[s1.l.at(i)] != s1.score) continue;
					if (!next_slot(a, r, last, at)) { full = true; break; }
					bool fwd = a.rep_fwd[s1.l.at(i)] != 0;
					write_record_at(a, at, s1, i, KG_ALN_MAPPED, fwd ? 0 : 0x10, false, 0, 0, !fwd);
					if (!a.multi_hit) break;
				}
				if (full) { atomicAdd(&a.ctl[8 + WHY_CAPACITY], 1ull); a.records[r].kind = KG_ALN_HOST; break; }
				if (last < 0) write_record(a, r, s1, KG_ALN_NONE, 0, false, 0, 0, false);
				if (s1.mapq == 60) add_unique = 1;
			}
			break;
		}
		ReadSum s2;
		summarise(a, r + 1, s2);
		if (s2.score > kAlnMaxScore || s2.sub_score > kAlnMaxScore) {
			atomicAdd(&a.ctl[8 + WHY_SCORE], 1ull);
			a.records[r].kind = KG_ALN_HOST; a.records[r + 1].kind = KG_ALN_HOST;
			break;
		}
		// CheckPairedFinalAlignments, src/Mapping.cpp:429-480 (bMultiHit false)
		{
			bool mated = false;
			if (s1.can_num > 0 && s2.can_num > 0) mated = a.c_mate[s1.l.at(s1.best)] == s2.best;
			else if (s1.can_num == 0 && s2.can_num > 0) mated = -1 == s2.best;       // (a report of an empty read: mate -1)
			else if (s1.can_num > 0 && s2.can_num == 0) mated = a.c_mate[s1.l.at(s1.best)] == 0;
			else mated = false;                                                      // -1 == 0
			if (!mated || a.multi_hit) {                                             // (!bMultiHit && bMated returns, :438)
				if (!mated && s1.score > 0 && s2.score > 0) {
					int s = 0;
					for (int i = 0; i < s1.can_num; ++i) {
						int j;
						if (a.rep_score[s1.l.at(i)] > 0 && (j = a.c_mate[s1.l.at(i)]) != -1 && a.rep_score[s2.l.at(j)] > 0) {
							mated = true;
							int t = a.rep_score[s1.l.at(i)] + a.rep_score[s2.l.at(j)];
							if (s < t) {
								s = t;
								s1.best = i; s1.score = a.rep_score[s1.l.at(i)];
								s2.best = j; s2.score = a.rep_score[s2.l.at(j)];
							}
						}
					}
				}
				if (mated) {
					for (int i = 0; i < s1.can_num; ++i) {
						int j;
						if (a.rep_score[s1.l.at(i)] != s1.score || ((j = a.c_mate[s1.l.at(i)]) != -1 && a.rep_score[s2.l.at(j)] != s2.score)) {
							a.rep_score[s1.l.at(i)] = 0;
							a.c_mate[s1.l.at(i)] = -1;
						}
					}
				} else {
					for (int i = 0; i < s1.can_num; ++i) {
						a.c_mate[s1.l.at(i)] = -1;
						if (a.rep_score[s1.l.at(i)] > 0 && a.rep_score[s1.l.at(i)] != s1.score) a.rep_score[s1.l.at(i)] = 0;
					}
					for (int j = 0; j < s2.can_num; ++j) {
						a.c_mate[s2.l.at(j)] = -1;
						if (a.rep_score[s2.l.at(j)] > 0 && a.rep_score[s2.l.at(j)] != s2.score) a.rep_score[s2.l.at(j)] = 0;
					}
				}
			}
		}
		// SetPairedAlignmentFlag, src/Mapping.cpp:73-158
		int f1, f2;
		if (s1.score > s1.sub_score && s2.score > s2.sub_score) {
			f1 = 0x41; f2 = 0x81;
			if (s2.best == rep_mate_at(a, s1, s1.best)) { f1 |= 0x2; f2 |= 0x2; }
			f1 |= rep_fwd_at(a, s1, s1.best) ? 0x20 : 0x10;
			f2 |= rep_fwd_at(a, s2, s2.best) ? 0x20 : 0x10;
		} else {
			f1 = one_mate_flag(a, s1, s2, 0x41);
			f2 = one_mate_flag(a, s2, s1, 0x81);
		}
		s1.mapq = eval_mapq(a, s1);
		s2.mapq = eval_mapq(a, s2);
		// OutputPairedAlignments, src/Mapping.cpp:177-270: the best candidate, or with -m every candidate from the best one on that
		// still has a positive score
		const bool both_unique = s1.score > s1.sub_score && s2.score > s2.sub_score;
		bool full = false;
		if (s1.score == 0) {
			add_unmapped++;
			write_record(a, r, s1, KG_ALN_UNMAPPED, f1, false, 0, 0, false);
		} else {
			if (s1.mapq == 60) add_unique++;
			int64_t last = -1, at = r;
			for (int i = s1.best; i < s1.can_num && !full; ++i) {
				if (rep_score_at(a, s1, i) > 0) {
					if (!next_slot(a, r, last, at)) { full = true; break; }
					int fl = a.multi_hit ? multi_flag(a, s1, s2, i, 0x41, both_unique, f1) : f1;
					int j = rep_mate_at(a, s1, i);
					bool fwd = rep_fwd_at(a, s1, i);
					if (j != -1 && rep_score_at(a, s2, j) > 0) {
						int dist = (int)(a.rep_pos[s2.l.at(j)] - a.rep_pos[s1.l.at(i)] + (fwd ? s2.rlen : 0 - s1.rlen));
						if (i == s1.best) {
							add_paired = 2;
							int ad = dist < 0 ? -dist : dist;
							if (ad < 10000) add_dist = ad;
						}
						write_record_at(a, at, s1, i, KG_ALN_MAPPED, fl, true, a.rep_pos[s2.l.at(j)], dist, !fwd);
					} else write_record_at(a, at, s1, i, KG_ALN_MAPPED, fl, false, 0, 0, !fwd);
				}
				if (!a.multi_hit) break;
			}
			if (last < 0) write_record(a, r, s1, KG_ALN_NONE, 0, false, 0, 0, false);
		}
		if (s2.score == 0) {
			add_unmapped++;
			write_record(a, r + 1, s2, KG_ALN_UNMAPPED, f2, false, 0, 0, false);
		} else {
			if (s2.mapq == 60) add_unique++;
			int64_t last = -1, at = r + 1;
			for (int j = s2.best; j < s2.can_num && !full; ++j) {
				if (rep_score_at(a, s2, j) > 0) {
					if (!next_slot(a, r + 1, last, at)) { full = true; break; }
					int fl = a.multi_hit ? multi_flag(a, s2, s1, j, 0x81, both_unique, f2) : f2;
					int i = rep_mate_at(a, s2, j);
					bool fwd = rep_fwd_at(a, s2, j);
					if (i != -1 && rep_score_at(a, s1, i) > 0) {
						bool fwd1 = rep_fwd_at(a, s1, i);
						int dist = 0 - (int)(a.rep_pos[s2.l.at(j)] - a.rep_pos[s1.l.at(i)] + (fwd1 ? s2.rlen : 0 - s1.rlen));
						write_record_at(a, at, s2, j, KG_ALN_MAPPED, fl, true, a.rep_pos[s1.l.at(i)], dist, fwd);
					} else write_record_at(a, at, s2, j, KG_ALN_MAPPED, fl, false, 0, 0, fwd);
				}
				if (!a.multi_hit) break;
			}
			if (last < 0) write_record(a, r + 1, s2, KG_ALN_NONE, 0, false, 0, 0, false);
		}
		if (full) {                                    // no extra record slot left: the pair goes to the host
			atomicAdd(&a.ctl[8 + WHY_CAPACITY], 1ull);
			a.records[r].kind = KG_ALN_HOST; a.records[r + 1].kind = KG_ALN_HOST;
			add_unmapped = 0; add_unique = 0; add_paired = 0; add_dist = 0;      // (nothing of a pair handed back is counted here)
			break;
		}
		} while (false);
		// ---- into the chunks' statistics: one set of atomics per wave where its lanes share a chunk ----
		const uint64_t have = __ballot(ck >= 0);
		if (have == 0) continue;
		const int ck0 = __shfl(ck, __ffsll((unsigned long long)have) - 1);
		if (__ballot(ck >= 0 && ck != ck0) == 0) {
			for (int off = 32; off > 0; off >>= 1) {
				add_paired += __shfl_xor(add_paired, off); add_dist += __shfl_xor(add_dist, off);
				add_unmapped += __shfl_xor(add_unmapped, off); add_unique += __shfl_xor(add_unique, off); add_host += __shfl_xor(add_host, off);
			}
			if ((threadIdx.x & 63) != 0) ck = -1;
		}
		if (ck >= 0) {
			kg_chunk_stats &cs = a.chunk_stats[ck];
			if (add_host) atomicAdd(&cs.host_pairs, add_host);
			if (add_unmapped) atomicAdd(&cs.unmapped, add_unmapped);
			if (add_unique) atomicAdd(&cs.unique, add_unique);
			if (add_paired) atomicAdd((unsigned long long *)&cs.paired, (unsigned long long)add_paired);
			if (add_dist) atomicAdd((unsigned long long *)&cs.distance, (unsigned long long)add_dist);
		}
	}
}

__global__ void aln_reset_kernel(AlnArgs a)
{
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	// (ctl[8..23]: running tallies, never reset: [8..20] why pairs went back to the host; [21..23] parked candidates, NW jobs and
	// partition plans of the batches before this one)
	if (i == 0) { a.ctl[21] += a.ctl[0]; a.ctl[22] += a.ctl[1]; a.ctl[23] += a.ctl[5]; }
	__syncthreads();
	if (i == 0) a.ctl[33] += a.ctl[32];                  // (running tally: candidates the fast plan kernel left to the general one)
	if (i < 8) a.ctl[i] = 0;
	if (i >= 24 && i < 33) a.ctl[i] = 0;
	if (i >= 34 && i <= 37) a.ctl[i] = 0;                // (aln_trivial_kernel: candidates / pairs it leaves to the general kernels, pairs it decided; [37]: unused)
	for (int c = i; c < a.n_chunks; c += gridDim.x * blockDim.x) {
		kg_chunk_stats z;
		z.paired = 0; z.distance = 0; z.lo = -1; z.hi = 0x7fffffffffffffffll; z.unmapped = 0; z.unique = 0; z.host_pairs = 0; z.rescue_wanted = 0;
		a.chunk_stats[c] = z;
	}
	for (int64_t r = i; r < a.n_reads; r += (int64_t)gridDim.x * blockDim.x) { a.r_host[r] = 0; a.r_pending[r] = 0; a.resc_n[r] = 0; a.resc_off[r] = 0; }
}

void launch_aln_reset(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_reset_kernel, dim3(grid_for_aln(a.n_reads, 256, n_cu * 8)), dim3(256), 0, stream, a);
}

void launch_aln_final(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_final_kernel, dim3(grid_for_aln(a.n_reads, 256, n_cu * 16)), dim3(256), 0, stream, a);
}

void launch_aln_pair(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_pair_kernel, dim3(grid_for_aln(a.all_paired ? a.n_reads / 2 + 1 : a.n_reads, 256, n_cu * 16)), dim3(256), 0, stream, a);
}

void launch_aln_rescue(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_rescue_kernel, dim3(grid_for_aln(a.task_capacity, 1, n_cu * 32)), dim3(64), 0, stream, a);
	hipLaunchKernelGGL(aln_post_rescue_kernel, dim3(grid_for_aln(a.n_reads, 256, n_cu * 16)), dim3(256), 0, stream, a);
}

}  // namespace kg
