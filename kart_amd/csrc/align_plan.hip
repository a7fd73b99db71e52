// align_plan.hip -- the alignment stage's planning step: aln_trivial_kernel, aln_bin_kernel, aln_plan_fast_kernel, aln_plan_kernel,
// aln_partition_kernel (the kernel <-> reference correspondence of the whole stage: align_kernels.hip).
#include "align_device.hpp"

namespace kg {

// ---- normal pairs ------------------------------------------------------------------------------------------------------------
namespace {

struct Pairs {                      // vector<SeedPair_t> of one candidate, in the lane's private memory
	int64_t gPos[kAlnMaxPairs];
	int32_t rPos[kAlnMaxPairs];
	int32_t rLen[kAlnMaxPairs], gLen[kAlnMaxPairs];
	uint8_t simple[kAlnMaxPairs];
	int num;
};

__device__ __forceinline__ void erase_empty(Pairs &v)
{
	int w = 0;
	for (int i = 0; i < v.num; ++i)
		if (v.rLen[i] != 0) {
			if (w != i) { v.gPos[w] = v.gPos[i]; v.rPos[w] = v.rPos[i]; v.rLen[w] = v.rLen[i]; v.gLen[w] = v.gLen[i]; v.simple[w] = v.simple[i]; }
			w++;
		}
	v.num = w;
}

// RemoveTandemRepeatSeeds, src/AlignmentCandidates.cpp:235-260: every read position hit by more than one seed goes
__device__ void remove_tandem_repeats(Pairs &v)
{
	if (v.num < 2) return;
	bool any = false;
	uint32_t drop = 0;
	for (int i = 0; i < v.num; ++i)
		for (int j = i + 1; j < v.num; ++j)
			if (v.rPos[i] == v.rPos[j]) { drop |= (1u << i) | (1u << j); any = true; }
	if (!any) return;
	for (int i = 0; i < v.num; ++i)
		if ((drop >> i) & 1) v.rLen[i] = v.gLen[i] = 0;
	erase_empty(v);
}

// RemoveTranslocatedSeeds, src/AlignmentCandidates.cpp:262-321.  ord[k] = index (in genome order) of the seed with the k-th
// smallest read position (read positions are distinct once the tandem repeats are gone)
__device__ void remove_translocated(Pairs &v)
{
	const int num = v.num;
	if (num < 2) return;
	int ord[kAlnMaxSeeds];
	for (int i = 0; i < num; ++i) {
		int x = i, p = i;
		while (p > 0 && v.rPos[ord[p - 1]] > v.rPos[x]) { ord[p] = ord[p - 1]; --p; }
		ord[p] = x;
	}
	bool any = false;
	for (int i = 0; i < num; ++i) {
		if (ord[i] == i) continue;
		any = true;
		int hi = ord[i];
		for (int j = i + 1; j <= hi; ++j)
			if (ord[j] > hi) hi = ord[j];
		int s1 = 0, s2 = 0;
		for (int k = i; k <= hi; ++k) {
			if (k < ord[k]) s1 += v.rLen[ord[k]];
			else s2 += v.rLen[ord[k]];
		}
		for (int k = i; k <= hi; ++k) {
			bool drop = s1 > s2 ? k > ord[k] : k < ord[k];
			if (drop) v.rLen[ord[k]] = v.gLen[ord[k]] = 0;
		}
		i = hi;
	}
	if (any) erase_empty(v);
}

// CheckSeedOverlapping, src/AlignmentCandidates.cpp:323-373
__device__ bool resolve_overlap(Pairs &v, int i, int j)
{
	bool master = true;
	int ov;
	if ((ov = v.rPos[i] + v.rLen[i] - v.rPos[j]) > 0) {
		if (v.rLen[i] < v.rLen[j]) {
			master = false;
			if (v.rLen[i] > ov) v.gLen[i] = (v.rLen[i] -= ov);
			else v.rLen[i] = v.gLen[i] = 0;
		} else if (v.rLen[j] > ov) {
			v.rPos[j] += ov; v.gPos[j] += ov; v.gLen[j] = (v.rLen[j] -= ov);
		} else v.rLen[j] = v.gLen[j] = 0;
	}
	if (v.rLen[i] > 0 && v.rLen[j] > 0 && (ov = (int)(v.gPos[i] + v.gLen[i] - v.gPos[j])) > 0) {
		if (v.gLen[i] < v.gLen[j]) {
			master = false;
			if (v.rLen[i] > ov) v.gLen[i] = (v.rLen[i] -= ov);
			else v.rLen[i] = v.gLen[i] = 0;
		} else if (v.rLen[j] > ov) {
			v.rPos[j] += ov; v.gPos[j] += ov; v.gLen[j] = (v.rLen[j] -= ov);
		} else v.rLen[j] = v.gLen[j] = 0;
	}
	return master;
}

// CheckOverlappingSeeds, src/AlignmentCandidates.cpp:375-418
__device__ void check_overlaps(Pairs &v)
{
	const int num = v.num;
	if (num < 2) return;
	bool any = false;
	for (int i = 0; i < num;) {
		if (v.rLen[i] > 0) {
			int r_end = v.rPos[i] + v.rLen[i] - 1;
			int64_t g_end = v.gPos[i] + v.gLen[i] - 1;
			for (int j = i + 1; j < num; ++j) {
				if (v.rLen[j] == 0) continue;
				if (r_end < v.rPos[j] && g_end < v.gPos[j]) break;
				if (!resolve_overlap(v, i, j)) break;
			}
			if (v.rLen[i] == 0) {
				any = true;
				int q = i - 1;
				while (q > 0 && v.rLen[q] == 0) q--;
				i = q < 0 ? 0 : q;
			} else i++;
		} else {
			any = true;
			i++;
		}
	}
	if (any) erase_empty(v);
}

__device__ __forceinline__ bool by_gpos_less(int64_t g1, int r1, int64_t g2, int r2)   // CompByGenomePos, :17-21
{
	return g1 == g2 ? r1 < r2 : g1 < g2;
}

// IdentifyNormalPairs(rlen, glen, v), src/AlignmentCandidates.cpp:420-490 (glen = -1 for a read against the genome, the
// fragment's genome length inside GenerateNormalPairAlignment).  false: more gap pairs than the envelope holds
__device__ bool identify_normal_pairs(int rlen, int glen, Pairs &v)
{
	if (v.num > 1) {
		remove_tandem_repeats(v);
		remove_translocated(v);
		check_overlaps(v);
		const int num = v.num;
		int added = 0;
		for (int i = 0, j = 1; j < num; ++i, ++j) {
			int r_gap = v.rPos[j] - (v.rPos[i] + v.rLen[i]);
			if (r_gap < 0) r_gap = 0;
			int g_gap = (int)(v.gPos[j] - (v.gPos[i] + v.gLen[i]));
			if (g_gap < 0) g_gap = 0;
			if (r_gap > 0 || g_gap > 0) {
				if (added == kAlnMaxGaps) return false;
				int t = num + added++;
				v.simple[t] = 0;
				v.rPos[t] = v.rPos[i] + v.rLen[i];
				v.gPos[t] = v.gPos[i] + v.gLen[i];
				v.rLen[t] = r_gap; v.gLen[t] = g_gap;
			}
		}
		// the appended gap pairs go between the seeds in (gPos, rPos) order: insertion, as the host does for up to 8 of them
		for (int t = num; t < num + added; ++t) {
			int64_t xg = v.gPos[t];
			int xr = v.rPos[t], xrl = v.rLen[t], xgl = v.gLen[t];
			uint8_t xs = v.simple[t];
			int p = t;
			while (p > 0 && by_gpos_less(xg, xr, v.gPos[p - 1], v.rPos[p - 1])) {
				v.gPos[p] = v.gPos[p - 1]; v.rPos[p] = v.rPos[p - 1]; v.rLen[p] = v.rLen[p - 1]; v.gLen[p] = v.gLen[p - 1]; v.simple[p] = v.simple[p - 1];
				--p;
			}
			v.gPos[p] = xg; v.rPos[p] = xr; v.rLen[p] = xrl; v.gLen[p] = xgl; v.simple[p] = xs;
		}
		v.num = num + added;
	}
	if (v.num > 0) {
		int r_gap = v.rPos[0] > 0 ? v.rPos[0] : 0;
		int g_gap = glen > 0 ? (int)v.gPos[0] : r_gap;            // glen = -1: the genome gap is the read gap (:458)
		if (r_gap > 0 || g_gap > 0) {
			for (int p = v.num; p > 0; --p) {
				v.gPos[p] = v.gPos[p - 1]; v.rPos[p] = v.rPos[p - 1]; v.rLen[p] = v.rLen[p - 1]; v.gLen[p] = v.gLen[p - 1]; v.simple[p] = v.simple[p - 1];
			}
			int64_t g = v.gPos[1] - g_gap;
			v.gPos[0] = g < 0 ? 0 : g;                             // (the reference's follow-up "gGaps += gPos" adds zero, :464)
			v.rPos[0] = 0; v.rLen[0] = r_gap; v.gLen[0] = g_gap; v.simple[0] = 0;
			v.num++;
		}
		int last = v.num - 1;
		r_gap = rlen - (v.rPos[last] + v.rLen[last]);
		g_gap = glen > 0 ? (int)(glen - (v.gPos[last] + v.gLen[last])) : r_gap;
		if (r_gap > 0 || g_gap > 0) {
			int t = v.num++;
			v.simple[t] = 0;
			v.rPos[t] = v.rPos[last] + v.rLen[last];
			v.gPos[t] = v.gPos[last] + v.gLen[last];
			v.rLen[t] = r_gap; v.gLen[t] = g_gap;
		}
	}
	return true;
}

// CheckCoordinateValidity, src/AlignmentCandidates.cpp:582-610
__device__ bool coordinates_valid(const AlnArgs &a, const Pairs &v)
{
	int64_t g1 = 0, g2 = a.two_genome_size;
	for (int i = 0; i < v.num; ++i)
		if (v.gLen[i] > 0) { g1 = v.gPos[i]; break; }
	for (int i = v.num; i-- > 0;)
		if (v.gLen[i] > 0) { g2 = v.gPos[i] + v.gLen[i] - 1; break; }
	const int64_t L = a.genome_size;
	if ((g1 < L && g2 >= L) || (g1 >= L && g2 < L)) return false;
	int i1 = end_lower_bound(a, g1), i2 = end_lower_bound(a, g2);
	if (i1 == a.n_ends || i2 == a.n_ends || a.end_chr[i1] != a.end_chr[i2]) return false;
	return true;
}

// ---- CIGAR building --------------------------------------------------------------------------------------------------------
struct Cigar {                      // vector<pair<int,char>> cigar_vec
	int32_t len[kAlnMaxCigar];
	char op[kAlnMaxCigar];
	int n;
	bool overflow;
	__device__ __forceinline__ void push(int l, char o)
	{
		if (n < kAlnMaxCigar) { len[n] = l; op[n] = o; n++; }
		else overflow = true;
	}
};

struct Work {
	uint8_t kind[kAlnMaxPairs];
	uint8_t op[kAlnMaxPairs];
	int32_t op_len[kAlnMaxPairs];
	int32_t val[kAlnMaxPairs];      // IMMEDIATE: score (-1 = the > 3000 soft clip); JOB: job index
};

// GenMappingReport's pair loop and tail (src/AlignmentCandidates.cpp:657-722) for a candidate none of whose pairs needs an alignment -- every pair is
// W_NONE, W_SIMPLE or W_IMMEDIATE (a candidate with a W_JOB / W_PENDING pair is parked for aln_finish_group_kernel): CIGAR, AlnScore, coordinates.
// `first`: the read is the first of its pair (or single).  Returns false when the result does not fit the record.
__device__ bool report_job_free_candidate(const AlnArgs &a, int64_t cand, bool first, Pairs &v, const Work &w)
{
	const int num = v.num;
	Cigar cig;
	cig.n = 0; cig.overflow = false;
	int score = 0;
	for (int j = 0; j < num; ++j) {
		if (w.kind[j] == W_NONE) continue;
		if (w.kind[j] == W_SIMPLE) {
			cig.push(v.rLen[j], 'M');
			score += v.rLen[j];
			continue;
		}
		const bool head = j == 0, tail = j == num - 1 && !head;
		if (w.op[j] != 0) cig.push(w.op_len[j], (char)w.op[j]);
		const int s = w.val[j];
		if (head) {
			if (s > 0) score += s;
			if (s <= 0) { v.gPos[0] = v.gPos[1]; v.gLen[0] = 0; }         // :674-686
		} else if (tail) {
			if (s > 0) score += s;
			if (s <= 0) { v.gPos[j] = v.gPos[j - 1] + v.gLen[j - 1]; v.gLen[j] = 0; }
		} else score += s;
	}
	if (cig.overflow) return false;
	a.rep_chr[cand] = 0;
	a.rep_pos[cand] = 0;
	a.rep_fwd[cand] = 1;
	a.rep_cigar_len[cand] = 0;
	if (cig.n > 1) {                                                     // GapPenalty, :612-622, :701-706
		int gp = 0;
		for (int i = 0; i < cig.n; ++i)
			if (cig.op[i] == 'I' || cig.op[i] == 'D') gp += cig.len[i];
		score -= gp;
		if (score <= 0) { a.rep_score[cand] = 0; a.c_score[cand] = -1; return true; }     // (c_score -1: "continue" before the best/second-best step)
	}
	if (cig.n == 0) score = 0;
	else {
		// GenCoordinateInfo, :515-562
		const int64_t gPos = v.gPos[0], end_gPos = v.gPos[num - 1] + v.gLen[num - 1] - 1;
		bool fwd;
		int chr;
		int64_t pos;
		bool rev = false;
		if (gPos < a.genome_size) {
			fwd = first;
			if (a.n_chr == 1) { chr = 0; pos = gPos + 1; }
			else {
				int it = end_lower_bound(a, gPos);
				chr = a.end_chr[it];
				pos = gPos + 1 - a.chr_fwd_start[chr];
			}
		} else {
			fwd = !first;
			rev = true;
			if (a.n_chr == 1) { chr = 0; pos = a.two_genome_size - end_gPos; }
			else {
				int it = end_lower_bound(a, gPos);
				if (it == a.n_ends) it = a.n_ends - 1;
				pos = a.contig_end[it] - end_gPos + 1;
				chr = a.end_chr[it];
			}
		}
		// GenerateCIGAR, :492-513 (the reverse strand shows the elements in reverse order)
		char *out = a.rep_cigar + cand * KG_ALN_CIGAR_MAX;
		int at = 0;
		char state = 0;
		int cnt = 0;
		bool fits = true;
		auto emit = [&](int nn, char st) {
			char buf[12];
			int k = 0;
			do { buf[k++] = (char)('0' + nn % 10); nn /= 10; } while (nn);
			if (at + k + 1 > KG_ALN_CIGAR_MAX - 1) { fits = false; return; }
			while (k) out[at++] = buf[--k];
			out[at++] = st;
		};
		for (int q = 0; q < cig.n; ++q) {
			int i = rev ? cig.n - 1 - q : q;
			if (cig.op[i] != state) {
				if (cnt > 0) emit(cnt, state);
				cnt = cig.len[i];
				state = cig.op[i];
			} else cnt += cig.len[i];
		}
		if (cnt > 0) emit(cnt, state);
		if (!fits) return false;
		a.rep_cigar_len[cand] = (uint8_t)at;
		a.rep_chr[cand] = chr;
		a.rep_pos[cand] = pos;
		a.rep_fwd[cand] = fwd ? 1 : 0;
		if (pos <= 0) score = 0;
	}
	a.rep_score[cand] = score;
	return true;
}

// The runs plan_partition's scalar loop finds, bit-parallel: the read fragment (<= 256 characters) and the text around the
// genome fragment as 2 bits per base in registers; per diagonal one XOR per 32 bases, the equality bits compressed to one per
// base (256-bit vector), the positions where 8 consecutive bits are set by shift-and doubling, the maximal runs read off in
// increasing read position.  Same runs, same order as the scalar loop (which stays for MaxGaps > 32 and for fragments at
// the very start of the text).  -1: a non-ACGT character in the read fragment, or more runs than the envelope takes.
__device__ int partition_runs_packed(const AlnArgs &a, const uint8_t *f1, int64_t g, int rL, int gL, int mg, Pairs &v)
{
	uint64_t RD[8], TW[10];
	bool ok = true;
	const uint64_t k7f = 0x7F7F7F7F7F7F7F7Full;
#pragma unroll
	for (int w = 0; w < 8; ++w) {
		uint64_t acc = 0;
#pragma unroll
		for (int h = 0; h < 4; ++h) {
			const int t0 = 32 * w + 8 * h;
			if (t0 < rL) {
				uint64_t x = reinterpret_cast<const AlnU64u *>(f1 + t0)->v;                 // 8 characters (the buffer has slack behind the last read)
				const int nv = rL - t0;
				const uint64_t keep = nv >= 8 ? ~0ull : (1ull << (8 * nv)) - 1;
				uint64_t u = x & 0xDFDFDFDFDFDFDFDFull;
				// 0x80 in every byte that equals the constant (exact per byte, no borrow between bytes)
				uint64_t ya = u ^ 0x4141414141414141ull, yc = u ^ 0x4343434343434343ull, yg = u ^ 0x4747474747474747ull, yt = u ^ 0x5454545454545454ull;
				uint64_t good = ~((((ya & k7f) + k7f) | ya) & (((yc & k7f) + k7f) | yc) & (((yg & k7f) + k7f) | yg) & (((yt & k7f) + k7f) | yt)) & 0x8080808080808080ull;
				if ((good & keep) != (0x8080808080808080ull & keep)) ok = false;
				uint64_t c2 = (x >> 1) & 0x0303030303030303ull;                              // A 0, C 1, G 3, T 2 ...
				c2 ^= (c2 >> 1) & 0x0101010101010101ull;                                     // ... one Gray step from the codes 0..3
				c2 &= keep;
				c2 = (c2 | (c2 >> 6)) & 0x000F000F000F000Full;
				c2 = (c2 | (c2 >> 12)) & 0x000000FF000000FFull;
				c2 = (c2 | (c2 >> 24)) & 0xFFFFull;
				acc |= c2 << (16 * h);
			}
		}
		RD[w] = acc;
	}
	if (!ok) return -1;
	const int64_t g0 = g - (int64_t)(mg - 1);
	const int words = (rL + 31) >> 5;
#pragma unroll
	for (int k = 0; k < 10; ++k) TW[k] = k <= words + 1 ? text_word32(a, g0 + 32 * k) : 0;
	for (int d = -(mg - 1); d <= mg - 1; ++d) {
		const int t_lo = d < 0 ? -d : 0;
		const int t_hi = rL < gL - d ? rL : gL - d;
		if (t_hi - t_lo < 8) continue;
		const int s = d + mg - 1;
		const bool far = (s >> 5) != 0;
		const int sb = (s & 31) << 1;
		uint64_t E[4] = {0, 0, 0, 0};
#pragma unroll
		for (int w = 0; w < 8; ++w) {
			const int base = w << 5;
			if (base >= t_hi || base + 32 <= t_lo) continue;
			uint64_t lo = far ? TW[w + 1] : TW[w], hi = far ? TW[w + 2] : TW[w + 1];
			uint64_t tw = sb ? (lo >> sb) | (hi << (64 - sb)) : lo;
			uint64_t diff = RD[w] ^ tw;
			uint64_t eq = ~(diff | (diff >> 1)) & 0x5555555555555555ull;             // bit 2b set: base b equal
			int b0 = t_lo > base ? t_lo - base : 0, b1 = t_hi - base < 32 ? t_hi - base : 32;
			eq &= (b1 >= 32 ? ~0ull : ((1ull << (b1 << 1)) - 1)) & ~((1ull << (b0 << 1)) - 1);
			uint64_t x = eq;
			x = (x | (x >> 1)) & 0x3333333333333333ull;
			x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
			x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
			x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
			x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
			E[w >> 1] |= x << ((w & 1) << 5);
		}
		auto shr = [](const uint64_t *q, int k, uint64_t *o) {     // o = q >> k over 256 bits, 0 < k < 64
			o[0] = (q[0] >> k) | (q[1] << (64 - k)); o[1] = (q[1] >> k) | (q[2] << (64 - k)); o[2] = (q[2] >> k) | (q[3] << (64 - k)); o[3] = q[3] >> k;
		};
		uint64_t T[4], R[4];
		shr(E, 1, T);
		for (int i = 0; i < 4; ++i) R[i] = E[i] & T[i];             // >= 2
		shr(R, 2, T);
		for (int i = 0; i < 4; ++i) R[i] &= T[i];                   // >= 4
		shr(R, 4, T);
		for (int i = 0; i < 4; ++i) R[i] &= T[i];                   // >= 8
		while ((R[0] | R[1] | R[2] | R[3]) != 0) {
			int pos = R[0] ? __ffsll((unsigned long long)R[0]) - 1 : R[1] ? 64 + __ffsll((unsigned long long)R[1]) - 1
			        : R[2] ? 128 + __ffsll((unsigned long long)R[2]) - 1 : 192 + __ffsll((unsigned long long)R[3]) - 1;
			int e = pos + 8;                                        // extend while the bases stay equal
			while (e < 256 && ((E[e >> 6] >> (e & 63)) & 1)) e++;
			if (v.num == kAlnMaxSeeds) return -1;
			int k = v.num++;
			v.rPos[k] = pos; v.gPos[k] = pos + d; v.rLen[k] = v.gLen[k] = e - pos; v.simple[k] = 1;
			for (int c = pos; c < e; ++c) R[c >> 6] &= ~(1ull << (c & 63));   // (positions of this run cannot start another)
		}
	}
	return v.num;
}

// GenerateNormalPairAlignment for a fragment pair with both sides > 30 (src/tools.cpp:146-212; non-PacBio: MaxShift = MaxGaps):
// GenerateSimplePairsFromFragmentPair -- the common 8-mers of the two fragments whose positions differ by less than MaxShift,
// merged into exact matches of at least 8 bases (src/KmerAnalysis.cpp:104-179) -- then IdentifyNormalPairs(rLen, gLen, ...) on
// them, and per resulting piece either a literal stretch or a sub-fragment alignment.
// In two halves around the reservation of its list entries (one wave_reserve per list for the whole wave, aln_partition_kernel):
// partition_compute returns 1: the pair has a plan of n_pieces pieces, n_jobs of them sub-fragment alignments, ops_need op bytes in all;
// 0: the partition is empty (the caller aligns the whole fragment); -1: outside the envelope (host).
__device__ int partition_compute(const AlnArgs &a, const uint8_t *f1, int64_t g, int rL, int gL, Pairs &v, int &n_pieces, int &n_jobs, int &ops_need)
{
	v.num = 0;
	n_pieces = n_jobs = ops_need = 0;
	const int mg = a.max_gaps;
	if (mg >= 1 && mg <= 32 && g >= (int64_t)(mg - 1) && rL <= 256) {
		int rc = partition_runs_packed(a, f1, g, rL, gL, mg, v);
		if (rc < 0) return -1;
	} else {
	// the 8-mer code maps characters through nst_nt4_table and skips 'N': plain A/C/G/T (either case) is what the comparison
	// of 2-bit codes below reproduces
	for (int i = 0; i < rL; ++i) {
		unsigned u = f1[i] & 0xDFu;
		if (!(u == 'A' || u == 'C' || u == 'G' || u == 'T')) return -1;
	}
	// runs of at least 8 equal bases along the diagonals |gpos - rpos| < MaxShift, in (diagonal, read position) order
	for (int d = -(mg - 1); d <= mg - 1; ++d) {
		int t_lo = d < 0 ? -d : 0;
		int t_hi = rL < gL - d ? rL : gL - d;
		int run = 0;
		for (int t = t_lo; t <= t_hi; ++t) {
			bool eq = false;
			if (t < t_hi) {
				unsigned ch = f1[t];
				unsigned c1 = (ch >> 1) & 3;
				c1 ^= c1 >> 1;
				eq = (int)c1 == text_code(a, g + t + d);
			}
			if (eq) run++;
			else {
				if (run >= 8) {
					if (v.num == kAlnMaxSeeds) return -1;
					int k = v.num++;
					v.rPos[k] = t - run; v.gPos[k] = t - run + d; v.rLen[k] = v.gLen[k] = run; v.simple[k] = 1;
				}
				run = 0;
			}
		}
	}
	}
	if (v.num == 0) return 0;
	// sort(SimplePairVec, CompByGenomePos), src/KmerAnalysis.cpp:177
	for (int i = 1; i < v.num; ++i) {
		int64_t xg = v.gPos[i];
		int xr = v.rPos[i], xl = v.rLen[i];
		int p = i;
		while (p > 0 && by_gpos_less(xg, xr, v.gPos[p - 1], v.rPos[p - 1])) { v.gPos[p] = v.gPos[p - 1]; v.rPos[p] = v.rPos[p - 1]; v.rLen[p] = v.gLen[p] = v.rLen[p - 1]; --p; }
		v.gPos[p] = xg; v.rPos[p] = xr; v.rLen[p] = v.gLen[p] = xl;
	}
	if (!identify_normal_pairs(rL, gL, v)) return -1;
	if (v.num == 0) return 0;
	// the pieces; op strings: the assembled one (at most rL + gL columns) and one per sub-fragment
	ops_need = rL + gL;
	for (int i = 0; i < v.num; ++i) {
		if (v.rLen[i] <= 0 && v.gLen[i] <= 0) continue;
		n_pieces++;
		bool lit = v.gLen[i] == 0 || v.rLen[i] == 0 || (v.rLen[i] == 1 && v.gLen[i] == 1) || v.simple[i];
		if (!lit) { n_jobs++; ops_need += v.rLen[i] + v.gLen[i]; }
	}
	return 1;
}

// the plan of partition_compute into the entries reserved for it; false: a list is full (host) -- what was reserved INSIDE the job list is
// left as empty jobs then (the NW kernels walk every job below the counter: none may be an earlier batch's)
__device__ bool partition_write(const AlnArgs &a, int64_t enc_off, int64_t g, int rL, int gL, const Pairs &v, int n_pieces, int n_jobs, int ops_need,
                                unsigned long long plan_at, unsigned long long piece_at, unsigned long long job_at, unsigned long long ops_at, int32_t &plan_index)
{
	if (plan_at >= (unsigned long long)a.job_capacity || piece_at + n_pieces > 4ull * (unsigned long long)a.job_capacity ||
	    job_at + n_jobs > (unsigned long long)a.job_capacity || ops_at + ops_need > (unsigned long long)a.ops_capacity) {
		for (unsigned long long k = job_at; k < job_at + (unsigned long long)n_jobs && k < (unsigned long long)a.job_capacity; ++k) { NwJobDesc jd; jd.o1 = 0; jd.o2 = 0; jd.ops = 0; jd.m = 0; jd.n = 0; a.jobs[k] = jd; }
		return false;
	}
	AlnPlan pl;
	pl.ops = (int64_t)ops_at; pl.first = (int32_t)piece_at; pl.count = n_pieces;
	a.plans[plan_at] = pl;
	unsigned long long ops_next = ops_at + (unsigned long long)(rL + gL);
	int pk = 0, jk = 0;
	for (int i = 0; i < v.num; ++i) {
		const int prl = v.rLen[i], pgl = v.gLen[i];
		if (prl <= 0 && pgl <= 0) continue;
		AlnPiece pc;
		if (pgl == 0) { pc.kind = KG_OP_GAP2; pc.v = prl; }                     // read bases against '-' (:170-174)
		else if (prl == 0) { pc.kind = KG_OP_GAP1; pc.v = pgl; }                // '-' against genome bases (:176-180)
		else if ((prl == 1 && pgl == 1) || v.simple[i]) { pc.kind = KG_OP_DIAG; pc.v = prl; }   // copied as they are (:182-186, :192)
		else {
			NwJobDesc jd;
			jd.o1 = enc_off + v.rPos[i]; jd.o2 = g + v.gPos[i]; jd.ops = (int64_t)ops_next; jd.m = prl; jd.n = pgl;
			ops_next += (unsigned long long)(prl + pgl);
			a.jobs[job_at + jk] = jd;
			pc.kind = 3; pc.v = (int32_t)(job_at + jk);
			jk++;
		}
		a.pieces[piece_at + pk++] = pc;
	}
	plan_index = (int32_t)plan_at;
	return true;
}

// ---- pass 1a: the candidates whose report needs no alignment and no private arrays -------------------------------------------------
// Most candidates of 150 bp reads at 1 % error are a few seeds ON ONE DIAGONAL, in order, without overlap, separated by single
// substituted bases: IdentifyNormalPairs (src/AlignmentCandidates.cpp:420-490) then removes nothing and only inserts the gap pairs
// between them (equal read and genome length), every gap pair is decided without nw_alignment -- the <= 2-mismatch shortcut or the
// 1 x 1 case of Process{Head,Normal,Tail}SequencePair (src/tools.cpp:240, 301, 352) -- every CIGAR element is an M, and
// GenMappingReport's result is: AlnScore = seed bases + matching gap bases, CIGAR "<rlen>M", the coordinate of the first pair
// (of the second when the head pair scored nothing, :674-686; likewise the tail).  This kernel decides exactly those candidates in
// registers -- 87 % of aln_plan_kernel's wave cycles were waits on its per-lane arrays in scratch memory (profiles/r03w) -- and
// lists every other candidate, untouched, for aln_plan_kernel (dense: its lanes all walk the general path).  KG_ALN_NO_FAST: off.
constexpr int kFastSeeds = 6;        // seeds of a candidate this kernel takes
constexpr int kFastGap = 2048;       // longest gap it looks at (head / tail gaps of candidates at repeat copies run to most of the read)

// mismatches of the read characters rd[0 .. L) against the text at g (raw characters as CalFragPairMismatchBases compares them,
// src/tools.cpp:40-47), counted up to `stop` (the decisions below only ask "at most 2?"); dash: a literal '-' in the first character
// (the 1 x 1 case then goes to nw_alignment, src/tools.cpp:229-233)
__device__ __forceinline__ int fast_gap_mismatches(const AlnArgs &a, const uint8_t *rd, int64_t g, int L, int stop, bool &dash)
{
	int n = 0;
	dash = rd[0] == '-';
	for (int b0 = 0; b0 < L && n < stop; b0 += 32) {
		const uint64_t tw = text_word32(a, g + b0);
		const int lim = L - b0 < 32 ? L - b0 : 32;
		for (int i0 = 0; i0 < lim && n < stop; i0 += 8) {
			const uint64_t w = reinterpret_cast<const AlnU64u *>(rd + b0 + i0)->v;          // (the character array has 64 bytes of slack)
			const int m = lim - i0 < 8 ? lim - i0 : 8;
			for (int i = 0; i < m; ++i) {
				const int c = (int)((w >> (8 * i)) & 255);
				const int code = (int)((tw >> (2 * (i0 + i))) & 3);
				const int t = code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T';
				n += c != t ? 1 : 0;
			}
		}
	}
	return n;
}

// A gap pair of L bases on the diagonal (read and genome side alike), role 0 = head, 1 = between seeds, 2 = tail: what
// Process{Head,Normal,Tail}SequencePair decide WITHOUT an alignment (src/tools.cpp:225-397), as aln_plan_kernel's pair loop does:
//   >= 0        : an 'M' element of L bases scoring that many identical ones (the <= 2-mismatch shortcut :240 / :301 / :352, or 1 x 1)
//   kFastClip   : the whole gap soft-clipped, score 0 (a head beyond 50 bases :307-311, a tail beyond 100 :358-362)
//   kFastSlow   : nw_alignment / the 8-mer partition / the > 3000 clip are due: the general kernel's
constexpr int kFastClip = -1, kFastSlow = -2;
__device__ __forceinline__ int fast_gap_value(const AlnArgs &a, const uint8_t *rd, int64_t g, int L, int role)
{
	if (role != 1 && L > 3000) return kFastSlow;
	bool dash = false;
	const int n = fast_gap_mismatches(a, rd, g, L, 3, dash);
	if (n <= 2 && n <= (int)(L * 0.2)) return L - n;
	if ((role == 0 && L > 50) || (role == 2 && L > 100)) return kFastClip;
	if (L == 1 && !dash) return 0;                               // one base against one other base: 1M, nothing identical
	return kFastSlow;
}

// What aln_plan_fast_kernel decides for one candidate (see above), as a value: both that kernel and aln_trivial_kernel use it.
struct FastRep {
	int state;                       // 0: decided (the fields below hold GenMappingReport's result), 1: the general kernel's, 2: CheckCoordinateValidity failed
	int score, chr, cigar_len;
	int64_t pos;
	bool fwd;
	uint64_t t0, t1;                 // the CIGAR text, at most 16 characters
};
enum { FAST_DECIDED = 0, FAST_SLOW = 1, FAST_INVALID = 2 };

// lower_bound(g): index of the first ChrLocMap key >= g; end_at(i): key i (both read the block's copy in the LDS when it holds the keys)
template <class LowerBound, class EndAt>
__device__ __forceinline__ FastRep fast_report(const AlnArgs &a, int count, const kg_seed *seeds, int64_t rbase, int rlen, bool first, LowerBound lower_bound, EndAt end_at)
{
	FastRep o;
	o.state = FAST_SLOW; o.score = 0; o.chr = 0; o.cigar_len = 0; o.pos = 0; o.fwd = true; o.t0 = o.t1 = 0;
	bool slow = count < 1 || count > kFastSeeds || rlen > 4000;
	// ---- the seeds: one diagonal, in order, no overlap; gaps of at most a text word ----
	int64_t d = 0;
	int prev_end = 0, first_r = 0, seed_bases = 0;
	int gap_at[kFastSeeds + 1], gap_len[kFastSeeds + 1];      // (indexed by unrolled constants: registers)
#pragma unroll
	for (int i = 0; i < kFastSeeds; ++i) {
		gap_at[i] = 0; gap_len[i] = 0;
		if (!slow && i < count) {
			const kg_seed sd = seeds[i];
			const int64_t di = sd.gPos - (int64_t)sd.rPos;
			if (i == 0) { d = di; first_r = sd.rPos; if (di < 0 || sd.rPos > kFastGap) slow = true; }
			else {
				if (di != d || sd.rPos < prev_end || sd.rPos - prev_end > kFastGap) slow = true;
				gap_at[i] = prev_end; gap_len[i] = sd.rPos - prev_end;
			}
			prev_end = sd.rPos + sd.len;
			seed_bases += sd.len;
		}
	}
	const int tail_len = rlen - prev_end;
	if (tail_len < 0 || tail_len > kFastGap) slow = true;
	if (slow) return o;
	// ---- CheckCoordinateValidity (:582-610) on [d, d + rlen - 1]: one strand copy, one contig ----
	const int64_t g1 = d, g2 = d + rlen - 1, L = a.genome_size;
	const int i1 = lower_bound(g1);
	bool valid = !((g1 < L && g2 >= L) || (g1 >= L && g2 < L)) && i1 < a.n_ends;
	if (valid && g2 > end_at(i1)) {
		const int i2 = lower_bound(g2);
		valid = i2 < a.n_ends && a.end_chr[i1] == a.end_chr[i2];
		if (valid) return o;          // (two keys of one contig cannot lie in one strand copy: never taken; the general path decides)
	}
	if (!valid) { o.state = FAST_INVALID; return o; }          // no report, and no best/second-best step (:647)
	// ---- the gap pairs ----
	const uint8_t *rd = a.enc + rbase;
	int score = seed_bases;
	int head_val = 1, tail_val = 1;          // (> 0: scored; 0: an M element without identical bases; kFastClip: soft-clipped)
	if (first_r > 0) { head_val = fast_gap_value(a, rd, d, first_r, 0); slow = head_val == kFastSlow; score += head_val > 0 ? head_val : 0; }
#pragma unroll
	for (int i = 1; i < kFastSeeds; ++i)
		if (!slow && i < count && gap_len[i] > 0) {
			const int v = fast_gap_value(a, rd + gap_at[i], d + gap_at[i], gap_len[i], 1);
			slow = v == kFastSlow;
			score += v > 0 ? v : 0;
		}
	if (!slow && tail_len > 0) { tail_val = fast_gap_value(a, rd + prev_end, d + prev_end, tail_len, 2); slow = tail_val == kFastSlow; score += tail_val > 0 ? tail_val : 0; }
	if (slow) return o;
	// ---- GenMappingReport's tail: GenCoordinateInfo (:515-562), GenerateCIGAR (:492-513) ----
	const int64_t gPos = head_val > 0 ? d : d + first_r;                     // a head pair that scored nothing gives its place up (:674-686)
	const int64_t end_gPos = (tail_val > 0 ? d + rlen : d + prev_end) - 1;   // ... and so does the tail pair
	bool fwd;
	int chr;
	int64_t pos;
	const bool rev = gPos >= L;
	if (!rev) {
		fwd = first;
		if (a.n_chr == 1) { chr = 0; pos = gPos + 1; }
		else { chr = a.end_chr[i1]; pos = gPos + 1 - a.chr_fwd_start[chr]; }
	} else {
		fwd = !first;
		if (a.n_chr == 1) { chr = 0; pos = a.two_genome_size - end_gPos; }
		else { pos = end_at(i1) - end_gPos + 1; chr = a.end_chr[i1]; }
	}
	// the elements: [head S] M [tail S] -- every M element merges into one; the reverse strand shows them in reverse order
	const int clip_h = head_val == kFastClip ? first_r : 0, clip_t = tail_val == kFastClip ? tail_len : 0;
	const int e_len[3] = {rev ? clip_t : clip_h, rlen - clip_h - clip_t, rev ? clip_h : clip_t};
	char out[16];
	int at = 0;
#pragma unroll
	for (int q = 0; q < 3; ++q) {
		int nn = e_len[q];
		if (nn <= 0) continue;
		char buf[4];
		int k = 0;
		do { buf[k++] = (char)('0' + nn % 10); nn /= 10; } while (nn);
		while (k) out[at++] = buf[--k];
		out[at++] = q == 1 ? 'M' : 'S';
	}
	uint64_t t0 = 0, t1 = 0;
#pragma unroll
	for (int q = 0; q < 16; ++q) {
		const uint64_t ch = q < at ? (uint64_t)(uint8_t)out[q] : 0ull;
		if (q < 8) t0 |= ch << (8 * q); else t1 |= ch << (8 * (q - 8));
	}
	o.state = FAST_DECIDED;
	o.t0 = t0; o.t1 = t1; o.cigar_len = at;
	o.chr = chr; o.pos = pos; o.fwd = fwd;
	o.score = pos <= 0 ? 0 : score;
	return o;
}

// The candidates the planning kernels walk: every chained candidate and the slots of the rescue windows -- or, when aln_trivial_kernel
// has decided the trivial pairs, the candidates of the OTHER pairs (a.slow_cands, ctl[34] of them) and the rescue slots.
__device__ __forceinline__ int64_t plan_slots(const AlnArgs &a)
{
	unsigned long long n_tasks = a.ctl[4];
	if (n_tasks > (unsigned long long)a.task_capacity) n_tasks = (unsigned long long)a.task_capacity;
	return (a.slow_cands ? (int64_t)a.ctl[34] : a.n_cands) + (int64_t)n_tasks;
}
__device__ __forceinline__ int64_t slot_cand(const AlnArgs &a, int64_t slot)
{
	if (!a.slow_cands) return slot;
	const int64_t n = (int64_t)a.ctl[34];
	return slot < n ? (int64_t)a.slow_cands[slot] : a.n_cands + (slot - n);
}

}  // namespace

__global__ __launch_bounds__(256) void aln_plan_fast_kernel(AlnArgs a)
{
	__shared__ int64_t s_end[128];
	const bool ends_in_lds = a.n_ends <= 128;
	if (ends_in_lds)
		for (int i = threadIdx.x; i < a.n_ends; i += blockDim.x) s_end[i] = a.contig_end[i];
	__syncthreads();
	auto end_at = [&](int i) { return ends_in_lds ? s_end[i] : a.contig_end[i]; };
	auto lower_bound = [&](int64_t g) {
		int lo = 0, hi = a.n_ends;
		while (lo < hi) {
			int mid = (lo + hi) >> 1;
			if (end_at(mid) < g) lo = mid + 1; else hi = mid;
		}
		return lo;
	};
	const int64_t n_all = plan_slots(a);
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t slot0 = (int64_t)blockIdx.x * blockDim.x; slot0 < n_all; slot0 += stride) {
		const int64_t slot = slot0 + threadIdx.x;
		bool slow = false;
		int64_t cand = 0;
		if (slot < n_all) {
			cand = a.plan_order ? (int64_t)a.plan_order[slot] : slot_cand(a, slot);
			a.rep_score[cand] = 0; a.rep_chr[cand] = 0; a.rep_pos[cand] = 0; a.rep_fwd[cand] = 1; a.rep_cigar_len[cand] = 0;
			const int64_t r = a.c_read[cand];
			if (!a.r_host[r] && a.c_score[cand] != 0) {
				const bool rescued = cand >= a.n_cands;
				int count;
				const kg_seed *seeds;
				if (!rescued) { const kg_candidate cd = a.cands[cand]; count = cd.count; seeds = a.cand_seeds + cd.first; }
				else { const int64_t t = cand - a.n_cands; count = a.resc_count[t]; seeds = a.resc_seeds + t * kAlnMaxSeeds; }
				const int64_t rbase = a.read_off[r];
				const int rlen = (int)(a.read_off[r + 1] - rbase);
				const int ck = chunk_of(a, r);
				const bool first = a.chunk_paired[ck] ? (((r - a.chunk_off[ck]) & 1) == 0) : true;
				const FastRep o = fast_report(a, count, seeds, rbase, rlen, first, lower_bound, end_at);
				slow = o.state == FAST_SLOW;
				if (o.state == FAST_INVALID) a.c_score[cand] = -1;
				else if (o.state == FAST_DECIDED) {
					uint64_t *dst = reinterpret_cast<uint64_t *>(a.rep_cigar + cand * KG_ALN_CIGAR_MAX);
					dst[0] = o.t0;
					if (o.cigar_len > 8) dst[1] = o.t1;
					a.rep_cigar_len[cand] = (uint8_t)o.cigar_len;
					a.rep_chr[cand] = o.chr;
					a.rep_pos[cand] = o.pos;
					a.rep_fwd[cand] = o.fwd ? 1 : 0;
					a.rep_score[cand] = o.score;
				}
			}
		}
		// ---- everything else: listed for the general kernel, densely ----
		const uint64_t mask = __ballot(slow);
		if (mask) {
			const int leader = __ffsll((unsigned long long)mask) - 1;
			unsigned long long at = 0;
			if ((int)(threadIdx.x & 63) == leader) at = atomicAdd(&a.ctl[32], (unsigned long long)__popcll(mask));
			at = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(at >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)at, leader);
			const uint64_t below = (threadIdx.x & 63) == 0 ? 0ull : (~0ull >> (64 - (threadIdx.x & 63)));
			if (slow) a.plan_slow[at + (unsigned long long)__popcll(mask & below)] = (int32_t)cand;
		}
	}
}

// ---- pass 0: the trivial pairs, start to finish, one pair per lane ---------------------------------------------------------------
// At 150 bp / 1 % error three pairs in four are trivial: each mate has ONE candidate, the two are each other's mate under
// CheckPairedAlignmentCandidates (src/Mapping.cpp:348-400: 0 <= PosDiff2 - PosDiff1 < EstDistance), and both candidates are the kind
// aln_plan_fast_kernel decides in registers.  For such a pair everything between chaining and the record is a function of ~200 bytes:
//   RemoveUnMatedAlignmentCandidates adds the two scores (:402-427), RemoveRedundantCandidates sees one candidate (:317-346),
//   GenMappingReport yields the two reports (fast_report), score > sub_score = 0 on both mates, the best candidates are mated so
//   CheckPairedFinalAlignments leaves at once (:429-438; with -m its loops change nothing for one candidate per mate),
//   SetPairedAlignmentFlag takes its first branch (:78-93), EvaluateMAPQ answers 60 (:160-175), OutputPairedAlignments prints the two
//   records with RNEXT / PNEXT / TLEN (:177-270) and counts the pair into iPaired / iDistance (:209-213).
// The per-candidate arrays (c_score, c_mate, rep_*) are never written or read for these pairs, none of the later kernels sees them:
// the pairs this kernel does NOT take are listed (a.slow_pairs, ctl[35]) with their candidates (a.slow_cands, ctl[34]), and
// aln_pair / aln_post_rescue / aln_bin / aln_plan_fast / aln_plan / aln_final walk those lists, densely.  The two 112-byte records
// of a lane are assembled in registers, staged through the LDS 32 pairs at a time and leave as whole 16-byte chunks of consecutive
// memory (aln_final_kernel writes a record field by field: 64 lanes, 64 lines per store).  KG_ALN_NO_TRIVIAL: off.
static_assert(sizeof(kg_aln_record) == 112 && offsetof(kg_aln_record, kind) == 16 && offsetof(kg_aln_record, est_lo) == 44 && offsetof(kg_aln_record, has_mate) == 52 &&
              offsetof(kg_aln_record, cigar) == 56 && offsetof(kg_aln_record, next) == 104 && offsetof(kg_aln_record, primary) == 108, "aln_trivial_kernel lays the record out by hand");

namespace {

__device__ __forceinline__ void stage_record(uint32_t *w, int64_t pos, int64_t mate_pos, int flag, int chr, int tlen, int score, int est_lo, bool flip, const FastRep &o)
{
	w[0] = (uint32_t)(uint64_t)pos; w[1] = (uint32_t)((uint64_t)pos >> 32);
	w[2] = (uint32_t)(uint64_t)mate_pos; w[3] = (uint32_t)((uint64_t)mate_pos >> 32);
	w[4] = KG_ALN_MAPPED; w[5] = (uint32_t)flag; w[6] = (uint32_t)chr; w[7] = 60; w[8] = (uint32_t)tlen;
	w[9] = (uint32_t)score; w[10] = 0;                           // score, sub_score
	w[11] = (uint32_t)est_lo; w[12] = 0x7fffffffu;               // the pair's own EstDistance interval (est_lo, est_hi]
	w[13] = 1u | ((flip ? 1u : 0u) << 8) | ((uint32_t)o.cigar_len << 16);      // has_mate, flip, cigar_len, rescue = 0
	w[14] = (uint32_t)o.t0; w[15] = (uint32_t)(o.t0 >> 32); w[16] = (uint32_t)o.t1; w[17] = (uint32_t)(o.t1 >> 32);
#pragma unroll
	for (int k = 18; k < 26; ++k) w[k] = 0;
	w[26] = 0xffffffffu;                                         // next = -1
	w[27] = 1;                                                   // primary, pad
}

}  // namespace

// One PAIR per lane.  (A form with one READ per lane -- the mates in neighbouring lanes, exchanging position, strand and length by a shuffle, half
// the chain of dependent loads per lane -- was built and measured slower, 62 against 39 ms per 100 M-read step: the staging, the flush, the
// ballots and the statistics are per wave, and a wave then covers 32 pairs instead of 64; profiles/r06g_*.)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void aln_trivial_kernel(AlnArgs a)
{
	__shared__ int64_t s_end[128];
	__shared__ __attribute__((aligned(16))) uint32_t s_rec[4][32 * 2 * 28];          // per wave: the records of 32 pairs (7168 bytes)
	const bool ends_in_lds = a.n_ends <= 128;
	if (ends_in_lds)
		for (int i = threadIdx.x; i < a.n_ends; i += blockDim.x) s_end[i] = a.contig_end[i];
	__syncthreads();
	auto end_at = [&](int i) { return ends_in_lds ? s_end[i] : a.contig_end[i]; };
	auto lower_bound = [&](int64_t g) {
		int lo = 0, hi = a.n_ends;
		while (lo < hi) {
			int mid = (lo + hi) >> 1;
			if (end_at(mid) < g) lo = mid + 1; else hi = mid;
		}
		return lo;
	};
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t *const stage = s_rec[wave];
	const int64_t n_pairs = a.n_reads >> 1;
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const long long est = a.est_distance;
	for (int64_t u0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); u0 < n_pairs; u0 += stride) {      // u0: the wave's first pair
		const int64_t u = u0 + lane;
		const bool live = u < n_pairs;
		const int64_t r = u << 1;
		bool trivial = false;
		int n1 = 0, n2 = 0;
		int64_t c1 = 0;
		FastRep o1, o2;
		o1.state = o2.state = FAST_SLOW;
		long long dist = 0;
		int rl1 = 0, rl2 = 0;
		if (live) {
			c1 = a.cand_off[r];
			const int64_t c2 = a.cand_off[r + 1], c3 = a.cand_off[r + 2];
			n1 = (int)(c2 - c1); n2 = (int)(c3 - c2);
			if (n1 == 1 && n2 == 1) {
				const kg_candidate k1 = a.cands[c1], k2 = a.cands[c2];
				dist = k2.posDiff - k1.posDiff;
				// each is the other's only and best mate (score > 0; a tie or a better rival needs a second candidate), :362-391
				if (k1.score > 0 && k2.score > 0 && dist >= 0 && dist < est) {
					const int64_t b1 = a.read_off[r], b2 = a.read_off[r + 1], b3 = a.read_off[r + 2];
					rl1 = (int)(b2 - b1); rl2 = (int)(b3 - b2);
					o1 = fast_report(a, k1.count, a.cand_seeds + k1.first, b1, rl1, true, lower_bound, end_at);
					if (o1.state == FAST_DECIDED && o1.score > 0)
						o2 = fast_report(a, k2.count, a.cand_seeds + k2.first, b2, rl2, false, lower_bound, end_at);
					trivial = o1.state == FAST_DECIDED && o2.state == FAST_DECIDED && o1.score > 0 && o2.score > 0 && o1.score <= kAlnMaxScore && o2.score <= kAlnMaxScore;
				}
			}
		}
		// ---- the pairs left to the general kernels, and their candidates, densely ----
		{
			const bool slow = live && !trivial;
			const uint64_t mask = __ballot(slow);
			if (mask) {
				const int nc = slow ? n1 + n2 : 0;
				int pre = nc;                                   // inclusive prefix sum of the lanes' candidate counts
#pragma unroll
				for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(pre, off); if (lane >= off) pre += t; }
				const int total = __shfl(pre, 63);
				const int leader = __ffsll((unsigned long long)mask) - 1;
				unsigned long long at_p = 0, at_c = 0;
				if (lane == leader) {
					at_p = atomicAdd(&a.ctl[35], (unsigned long long)__popcll(mask));
					if (total) at_c = atomicAdd(&a.ctl[34], (unsigned long long)total);
				}
				at_p = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(at_p >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)at_p, leader);
				at_c = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(at_c >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)at_c, leader);
				if (slow) {
					const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
					a.slow_pairs[at_p + (unsigned long long)__popcll(mask & below)] = (int32_t)u;
					int32_t *dst = a.slow_cands + at_c + (unsigned long long)(pre - nc);
					for (int k = 0; k < nc; ++k) dst[k] = (int32_t)(c1 + k);
				}
			}
		}
		// ---- the trivial pairs' records ----
		const uint64_t tmask = __ballot(trivial);
		if (tmask == 0) continue;
		int tl = 0;
		long long ad = 0;
		if (trivial) {
			tl = (int)(o2.pos - o1.pos + (o1.fwd ? rl2 : 0 - rl1));      // :204-207
			ad = tl < 0 ? -(long long)tl : (long long)tl;
			if (ad >= 10000) ad = 0;                                        // :211
		}
#pragma unroll
		for (int half = 0; half < 2; ++half) {
			const bool mine = trivial && (lane >> 5) == half;
			if (mine) {
				uint32_t *w = stage + (lane & 31) * 56;
				stage_record(w, o1.pos, o2.pos, 0x43 | (o1.fwd ? 0x20 : 0x10), o1.chr, tl, o1.score, (int)dist, !o1.fwd, o1);
				stage_record(w + 28, o2.pos, o1.pos, 0x83 | (o2.fwd ? 0x20 : 0x10), o2.chr, 0 - tl, o2.score, (int)dist, o2.fwd, o2);
			}
			// (a wave's LDS traffic is in program order; the fences keep the compiler from moving the reads above the writes of OTHER lanes)
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			const uint32_t hm = (uint32_t)(tmask >> (32 * half));
			if (hm == 0) continue;
			uint4 *const out = reinterpret_cast<uint4 *>(a.records + ((u0 + 32 * half) << 1));
			const uint4 *const in = reinterpret_cast<const uint4 *>(stage);
#pragma unroll
			for (int it = 0; it < 7; ++it) {
				const int q = it * 64 + lane;                   // 16-byte chunk of the half's 7168 bytes; 14 chunks per pair
				if ((hm >> (q / 14)) & 1u) out[q] = in[q];
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
		}
		// ---- what the pairs add to their chunks: iPaired / iDistance, the reads of MAPQ 60, the chunk's EstDistance interval ----
		int ck = -1;
		if (trivial) ck = chunk_of(a, r);
		const int ck0 = __shfl(ck, __ffsll((unsigned long long)tmask) - 1);
		if (__ballot(trivial && ck != ck0) == 0) {
			long long lo = trivial ? dist : -1, sum = ad;
			for (int off = 32; off > 0; off >>= 1) {
				const long long l2 = __shfl_xor(lo, off);
				lo = l2 > lo ? l2 : lo;
				sum += __shfl_xor(sum, off);
			}
			if (lane == 0) {
				kg_chunk_stats &cs = a.chunk_stats[ck0];
				const int np = __popcll(tmask);
				atomicAdd((unsigned long long *)&cs.paired, 2ull * (unsigned long long)np);
				if (sum) atomicAdd((unsigned long long *)&cs.distance, (unsigned long long)sum);
				atomicAdd(&cs.unique, 2 * np);
				atomicMax((long long *)&cs.lo, lo);
			}
		} else if (trivial) {
			kg_chunk_stats &cs = a.chunk_stats[ck];
			atomicAdd((unsigned long long *)&cs.paired, 2ull);
			if (ad) atomicAdd((unsigned long long *)&cs.distance, (unsigned long long)ad);
			atomicAdd(&cs.unique, 2);
			atomicMax((long long *)&cs.lo, dist);
		}
		if (lane == 0) atomicAdd(&a.ctl[36], (unsigned long long)__popcll(tmask));      // (pairs decided here, this batch)
	}
}

// ---- pass 1: one candidate per lane -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void aln_plan_kernel(AlnArgs a)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	int64_t n_all = plan_slots(a);                                               // chained candidates (all, or those of the pairs aln_trivial_kernel left), then the slots of the rescue windows
	if (a.plan_slow) n_all = (int64_t)a.ctl[32];                                 // ... or what aln_plan_fast_kernel left
	// (the wave's lanes stay together through the loop: what the parked candidates need of the lists is reserved for all of them by one atomic per list)
	for (int64_t slot0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); slot0 < n_all; slot0 += stride) {
		const int64_t slot = slot0 + (threadIdx.x & 63);
		// what phase 1 leaves for phase 2 (a parked candidate)
		Pairs v;
		Work w;
		int64_t cand = 0, r = 0, rbase = 0;
		int num = 0, n_new_jobs = 0, new_ops = 0, n_pending = 0;
		bool pending = false;
		// ---- phase 1: up to the point where the candidate is finished, handed to the host, or has to be parked ----
		bool park = false;
		do {
		if (slot >= n_all) break;
		// (binned: lanes of a wave then hold candidates with the same number of seeds -- the loops below run equally long)
		cand = a.plan_slow ? (int64_t)a.plan_slow[slot] : a.plan_order ? (int64_t)a.plan_order[slot] : slot_cand(a, slot);
		a.rep_score[cand] = 0; a.rep_chr[cand] = 0; a.rep_pos[cand] = 0; a.rep_fwd[cand] = 1; a.rep_cigar_len[cand] = 0;
		r = a.c_read[cand];
		if (a.r_host[r]) break;
		if (a.c_score[cand] == 0) break;                                  // GenMappingReport skips it, :643
		const bool rescued = cand >= a.n_cands;
		kg_candidate cd;
		const kg_seed *seeds;
		if (!rescued) { cd = a.cands[cand]; seeds = a.cand_seeds + cd.first; }
		else {
			int64_t t = cand - a.n_cands;
			cd.count = a.resc_count[t]; cd.first = 0; cd.posDiff = a.resc_posdiff[t]; cd.score = 0;
			seeds = a.resc_seeds + t * kAlnMaxSeeds;
		}
		if (cd.count > kAlnMaxSeeds) { flag_host(a, r, WHY_SEEDS); break; }
		rbase = a.read_off[r];
		const int rlen = (int)(a.read_off[r + 1] - rbase);
		const uint8_t *rd = a.enc + rbase;
		const int ck = chunk_of(a, r);
		const bool first = a.chunk_paired[ck] ? (((r - a.chunk_off[ck]) & 1) == 0) : true;
		v.num = cd.count;
		for (int i = 0; i < cd.count; ++i) {
			kg_seed s = seeds[i];
			v.gPos[i] = s.gPos; v.rPos[i] = s.rPos; v.rLen[i] = v.gLen[i] = s.len; v.simple[i] = 1;
		}
		if (rlen > 4000) { flag_host(a, r, WHY_READ_LEN); break; }
		if (!identify_normal_pairs(rlen, -1, v)) { flag_host(a, r, WHY_GAPS); break; }
		if (!coordinates_valid(a, v)) { a.c_score[cand] = -1; break; }      // no report, and no best/second-best step (:647)
		num = v.num;
		bool host = false, jobs = false;
		int why = WHY_PARTITION;
		for (int j = 0; j < num && !host; ++j) {
			w.kind[j] = W_NONE; w.op[j] = 0; w.op_len[j] = 0; w.val[j] = 0;
			const int rL = v.rLen[j], gL = v.gLen[j];
			if (rL == 0 && gL == 0) continue;
			if (v.simple[j]) { w.kind[j] = W_SIMPLE; continue; }
			const int role = j == 0 ? 0 : j == num - 1 ? 2 : 1;
			if (role != 1 && rL > 3000) {                                      // :671-676, :690-695
				w.kind[j] = W_IMMEDIATE; w.op[j] = 'S'; w.op_len[j] = rL; w.val[j] = -1;
				continue;
			}
			if (role == 1 && (rL == 0 || gL == 0)) {                           // ProcessNormalSequencePair, src/tools.cpp:229-233
				w.kind[j] = W_IMMEDIATE;
				if (rL > 0) { w.op[j] = 'I'; w.op_len[j] = rL; }
				else if (gL > 0) { w.op[j] = 'D'; w.op_len[j] = gL; }
				continue;
			}
			const uint8_t *f1 = rd + v.rPos[j];
			if (rL == gL) {                                                     // the <= 2-mismatch shortcut, :240, :301, :352
				bool dash_ = false;
				int n = fast_gap_mismatches(a, f1, v.gPos[j], rL, 3, dash_);      // (eight characters per load, stops at the third mismatch: only <= 2 matter here)
				if (n <= 2 && n <= (int)(rL * 0.2)) {
					w.kind[j] = W_IMMEDIATE; w.op[j] = 'M'; w.op_len[j] = rL; w.val[j] = rL - n;
					continue;
				}
			}
			if ((role == 0 && rL > 50) || (role == 2 && rL > 100)) {           // :307-311, :358-362
				w.kind[j] = W_IMMEDIATE; w.op[j] = 'S'; w.op_len[j] = rL; w.val[j] = 0;
				continue;
			}
			if (rL == 1 && gL == 1 && f1[0] != '-') {
				// one base against one base: nw_alignment can only answer with the diagonal, the quality check passes a single
				// column, nothing is trimmed, AddNewCigarElements books 1M with one identical base iff the characters are equal
				w.kind[j] = W_IMMEDIATE; w.op[j] = 'M'; w.op_len[j] = 1; w.val[j] = (char)f1[0] == text_char(a, v.gPos[j]) ? 1 : 0;
				continue;
			}
			if (rL > kAlnMaxFrag || gL > kAlnMaxFrag || rL <= 0 || gL <= 0) { host = true; break; }
			if (rL > 30 && gL > 30) {
				if (a.dbg_no_partition) { host = true; break; }
				// GenerateNormalPairAlignment's 8-mer partition, src/tools.cpp:146-212: about one candidate in thirteen has such a
				// pair, so almost every wave would walk the long path for a few lanes -- the pair is handed to the dense
				// aln_partition_kernel instead (one task per lane), which writes its outcome into the parked candidate
				w.kind[j] = W_PENDING;
				jobs = true; pending = true; n_pending++;
				continue;
			}
			// nw_alignment(rL, frag1, gL, frag2): a job for the NW kernels (its slot and op bytes are reserved below, with everything else the candidate needs)
			w.kind[j] = W_JOB; w.val[j] = -1;
			n_new_jobs++; new_ops += rL + gL;
			jobs = true;
		}
		if (host) { flag_host(a, r, why); break; }
		if (!jobs) {
			if (!report_job_free_candidate(a, cand, first, v, w)) flag_host(a, r, WHY_CIGAR);
			break;
		}
		park = true;
		} while (false);
		// park the candidate until its alignments exist.  What the wave's candidates need of the lists -- a spill slot each, their NW jobs and op
		// bytes, their partition tasks -- is reserved with ONE atomic per list for the whole wave (wave_reserve)
		const unsigned long long sp = wave_reserve(&a.ctl[0], park ? 1ull : 0ull);
		unsigned long long job_at = wave_reserve(&a.ctl[1], park ? (unsigned long long)n_new_jobs : 0ull);
		unsigned long long ops_at = wave_reserve(&a.ctl[2], park ? (unsigned long long)new_ops : 0ull);
		unsigned long long task_at = wave_reserve(&a.ctl[3], park ? (unsigned long long)n_pending : 0ull);
		if (!park) continue;
		const bool sp_ok = sp < (unsigned long long)a.spill_capacity;
		const bool jobs_ok = job_at + (unsigned long long)n_new_jobs <= (unsigned long long)a.job_capacity && ops_at + (unsigned long long)new_ops <= (unsigned long long)a.ops_capacity;
		if (!sp_ok || !jobs_ok) {
			// A list is full: the read is the host's.  Everything this lane took INSIDE the lists is still written, whichever list overflowed --
			// aln_finish_group_kernel walks every spill slot below ctl[0], the NW kernels every job below ctl[1], aln_partition_kernel every task below
			// ctl[3], and none may find an earlier batch's entry there: the spill slot names this candidate with no pairs (its read is flagged,
			// the finish pass skips it), the job slots become empty jobs, the tasks name the flagged read
			if (sp_ok) { a.spill[sp].cand = (int32_t)cand; a.spill[sp].num = 0; }
			for (unsigned long long k = job_at; k < job_at + (unsigned long long)n_new_jobs && k < (unsigned long long)a.job_capacity; ++k) { NwJobDesc jd; jd.o1 = 0; jd.o2 = 0; jd.ops = 0; jd.m = 0; jd.n = 0; a.jobs[k] = jd; }
			flag_host(a, r, WHY_CAPACITY);
			for (unsigned long long k = task_at; k < task_at + (unsigned long long)n_pending && k < (unsigned long long)a.job_capacity; ++k) {
				PartTask pt;
				pt.enc_off = rbase; pt.g = 0; pt.spill = 0; pt.j = 0; pt.read = (int32_t)r; pt.rL = 0; pt.gL = 0;
				a.part_tasks[k] = pt;
			}
			continue;
		}
		for (int j = 0; j < num; ++j) {
			if (w.kind[j] != W_JOB) continue;
			const int rL = v.rLen[j], gL = v.gLen[j];
			NwJobDesc jd;
			jd.o1 = rbase + v.rPos[j]; jd.o2 = v.gPos[j]; jd.ops = (int64_t)ops_at; jd.m = rL; jd.n = gL;
			a.jobs[job_at] = jd;
			w.val[j] = (int32_t)job_at;
			job_at++; ops_at += (unsigned long long)(rL + gL);
		}
		AlnSpill &o = a.spill[sp];
		o.cand = (int32_t)cand;
		o.num = num;
		for (int j = 0; j < num; ++j) {
			AlnSpillPair q;
			q.gPos = v.gPos[j]; q.rPos = v.rPos[j]; q.rLen = (int16_t)v.rLen[j]; q.gLen = (int16_t)v.gLen[j];
			q.val = w.val[j]; q.kind = w.kind[j]; q.op = w.op[j]; q.op_len = (int16_t)w.op_len[j];
			o.p[j] = q;
		}
		if (pending) {
			// (about one parked candidate in thirteen: a second round for those)
			if (task_at + (unsigned long long)n_pending > (unsigned long long)a.job_capacity) flag_host(a, r, WHY_CAPACITY);
			for (int j = 0; j < num; ++j) {
				if (w.kind[j] != W_PENDING) continue;
				const unsigned long long t = task_at++;
				if (t >= (unsigned long long)a.job_capacity) break;          // (the read is the host's, flagged above; every slot inside the list is written)
				PartTask pt;
				pt.enc_off = rbase + v.rPos[j]; pt.g = v.gPos[j]; pt.spill = (int32_t)sp; pt.j = j; pt.read = (int32_t)r;
				pt.rL = (int16_t)v.rLen[j]; pt.gL = (int16_t)v.gLen[j];
				a.part_tasks[t] = pt;
			}
		}
	}
}

// ---- pass 1b: the 8-mer partitions, one task per lane (dense) -----------------------------------------------------------------
__global__ __launch_bounds__(256) void aln_partition_kernel(AlnArgs a)
{
	unsigned long long n = a.ctl[3];
	if (n > (unsigned long long)a.job_capacity) n = (unsigned long long)a.job_capacity;
	const int lane = threadIdx.x & 63;
	// (the wave's lanes stay together: the list entries of all of them are reserved by one atomic per list)
	for (unsigned long long t0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); t0 < n; t0 += (unsigned long long)gridDim.x * blockDim.x) {
		const unsigned long long t = t0 + lane;
		PartTask pt;
		pt.enc_off = 0; pt.g = 0; pt.spill = 0; pt.j = 0; pt.read = 0; pt.rL = 0; pt.gL = 0;
		bool go = false;
		if (t < n) { pt = a.part_tasks[t]; go = !a.r_host[pt.read]; }
		Pairs v;
		int n_pieces = 0, n_jobs = 0, ops_need = 0, pr = -3;          // (-3: no task)
		if (go) {
			pr = partition_compute(a, a.enc + pt.enc_off, pt.g, pt.rL, pt.gL, v, n_pieces, n_jobs, ops_need);
			if (pr < 0) flag_host(a, pt.read, WHY_PARTITION);
		}
		// planned: a plan, its pieces, its jobs, its op bytes; no common 8-mer survived: the whole fragment is one alignment (src/tools.cpp:214-221)
		const bool planned = pr == 1, whole = pr == 0;
		const unsigned long long plan_at = wave_reserve(&a.ctl[5], planned ? 1ull : 0ull);
		const unsigned long long piece_at = wave_reserve(&a.ctl[6], planned ? (unsigned long long)n_pieces : 0ull);
		const unsigned long long job_at = wave_reserve(&a.ctl[1], planned ? (unsigned long long)n_jobs : whole ? 1ull : 0ull);
		const unsigned long long ops_at = wave_reserve(&a.ctl[2], planned ? (unsigned long long)ops_need : whole ? (unsigned long long)(pt.rL + pt.gL) : 0ull);
		if (planned) {
			AlnSpillPair &q = a.spill[pt.spill].p[pt.j];
			int32_t plan_index = 0;
			if (partition_write(a, pt.enc_off, pt.g, pt.rL, pt.gL, v, n_pieces, n_jobs, ops_need, plan_at, piece_at, job_at, ops_at, plan_index)) { q.kind = W_PLAN; q.val = plan_index; }
			else flag_host(a, pt.read, WHY_CAPACITY);
		} else if (whole) {
			AlnSpillPair &q = a.spill[pt.spill].p[pt.j];
			if (job_at >= (unsigned long long)a.job_capacity || ops_at + (unsigned long long)(pt.rL + pt.gL) > (unsigned long long)a.ops_capacity) {
				if (job_at < (unsigned long long)a.job_capacity) { NwJobDesc jd; jd.o1 = 0; jd.o2 = 0; jd.ops = 0; jd.m = 0; jd.n = 0; a.jobs[job_at] = jd; }      // (inside the list: an empty job, not an earlier batch's)
				flag_host(a, pt.read, WHY_CAPACITY);
			} else {
				NwJobDesc jd;
				jd.o1 = pt.enc_off; jd.o2 = pt.g; jd.ops = (int64_t)ops_at; jd.m = pt.rL; jd.n = pt.gL;
				a.jobs[job_at] = jd;
				q.kind = W_JOB; q.val = (int32_t)job_at;
			}
		}
	}
}

namespace {

// The order in which aln_plan_kernel takes the candidates: four bins by the number of seeds (none or one / two / three / more), each
// block a contiguous range of candidates -- pass 0 counts the bins (ctl[24..27]), pass 1 places the indices (ctl[28..31] run along).
__device__ __forceinline__ int plan_bin(const AlnArgs &a, int64_t cand)
{
	const int64_t r = a.c_read[cand];
	if (a.r_host[r] || a.c_score[cand] == 0) return 0;
	const int n = cand < a.n_cands ? a.cands[cand].count : a.resc_count[cand - a.n_cands];
	return n <= 1 ? 0 : n == 2 ? 1 : n == 3 ? 2 : 3;
}

}  // namespace

__global__ __launch_bounds__(256) void aln_bin_kernel(AlnArgs a, int pass)
{
	__shared__ unsigned int s_cnt[4];
	__shared__ unsigned long long s_next[4];
	const int64_t n_all = plan_slots(a);
	const int64_t per = (n_all + gridDim.x - 1) / gridDim.x;
	const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < n_all ? b0 + per : n_all;
	if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	unsigned int mine[4] = {0, 0, 0, 0};
	for (int64_t c = b0 + threadIdx.x; c < b1; c += blockDim.x) mine[plan_bin(a, slot_cand(a, c))]++;
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		unsigned int v = mine[b];
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
		if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[b], v);
	}
	__syncthreads();
	if (pass == 0) {
		if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&a.ctl[24 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
		return;
	}
	if (threadIdx.x < 4) {
		unsigned long long base = 0;
		for (int b = 0; b < (int)threadIdx.x; ++b) base += a.ctl[24 + b];
		s_next[threadIdx.x] = base + (s_cnt[threadIdx.x] ? atomicAdd(&a.ctl[28 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]) : 0ull);
	}
	__syncthreads();
	for (int64_t base = b0; base < b1; base += blockDim.x) {
		const int64_t c = base + threadIdx.x < b1 ? slot_cand(a, base + threadIdx.x) : -1;
		const int bin = c >= 0 ? plan_bin(a, c) : -1;
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const uint64_t mask = __ballot(bin == b);
			if (mask == 0) continue;
			const int leader = __ffsll((unsigned long long)mask) - 1;
			unsigned long long at = 0;
			if ((int)(threadIdx.x & 63) == leader) at = atomicAdd(&s_next[b], (unsigned long long)__popcll(mask));
			at = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(at >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)at, leader);
			const uint64_t below = (threadIdx.x & 63) == 0 ? 0ull : (~0ull >> (64 - (threadIdx.x & 63)));
			if (bin == b) a.plan_order[at + (unsigned long long)__popcll(mask & below)] = (int32_t)c;
		}
	}
}

void launch_aln_trivial(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_trivial_kernel, dim3(grid_for_aln(a.n_reads / 2 + 1, 256, n_cu * 16)), dim3(256), 0, stream, a);
}

void launch_aln_bin(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_bin_kernel, dim3(grid_for_aln(a.n_cands + a.task_capacity / 8, 256, n_cu * 8)), dim3(256), 0, stream, a, 0);
	hipLaunchKernelGGL(aln_bin_kernel, dim3(grid_for_aln(a.n_cands + a.task_capacity / 8, 256, n_cu * 8)), dim3(256), 0, stream, a, 1);
}

void launch_aln_plan_fast(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_plan_fast_kernel, dim3(grid_for_aln(a.n_cands + a.task_capacity / 8, 256, n_cu * 16)), dim3(256), 0, stream, a);
}

void launch_aln_plan(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_plan_kernel, dim3(grid_for_aln(a.n_cands + a.task_capacity / 8, 256, n_cu * 16)), dim3(256), 0, stream, a);
}

void launch_aln_partition(const AlnArgs &a, int n_cu, hipStream_t stream)
{
	hipLaunchKernelGGL(aln_partition_kernel, dim3(grid_for_aln(a.n_cands / 8 + 1, 256, n_cu * 8)), dim3(256), 0, stream, a);
}

}  // namespace kg
