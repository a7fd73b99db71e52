// kernels/md_tag.inc -- the MD:Z field of a mapped record, computed where the record is sized and where it is printed (kg_stream_set_tags,
// KG_STREAM_TAG_MD; the CLI's -md).  A fragment of text_device.hpp (included there, inside namespace kg { namespace { ... } }, for sam_kernels.hip and bam_kernels.hip); not a translation unit.
//
// The reference prints no MD (its NM is rlen - score, no edit distance); every consumer of its output runs `samtools calmd` over the file next.  Here the
// string is made from what the format kernels hold anyway: the 2-bit forward text, the read's characters and the record's contig, POS, strand and CIGAR.
// MD (SAM specification v1, 1.5: [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*) is a function of the record's SEQ AS PRINTED (the reverse complement of the read as held
// for a record shown on the other strand), its CIGAR, its contig and POS and the forward strand:
//   M (and =, X)  a column matches when the upper-cased read character is one of ACGT and equals the reference base, or when the read character is '='
//                 (calmd's rule on 4-bit codes); anything else -- N, IUPAC codes, what comp_char made of them -- is a mismatch and shows the REFERENCE base
//   D             '^' and the deleted reference bases;   I, S  read only;   N  reference only;   H, P  nothing
//   a number (possibly 0) in front, behind, and between any two of these.
// A reference position inside a hole of .amb (a run of one ambiguous character of the FASTA; .pac and the text hold random bases there) shows the hole's own
// character, upper case, and matches nothing but '=': the string calmd prints against the FASTA.  A position outside the record's contig
// (CheckCoordinateValidity excludes it) is never read from the text and shows 'N'.
// One lane walks one record.  Where the record's reference span lies inside its contig and touches no hole -- one binary search over the few hundred holes per
// record -- an M run is compared 32 columns per step: one unaligned word of the text against the read's characters packed to 2 bits, a mask for the
// characters that are not ACGT, and one loop turn per MISMATCH.  Everything else (a hole, a contig's edge) goes a column at a time.  No scratch, no LDS
// of its own, plain vector loads and stores; the host prints the same string with code of its own (host/detail/md.inc).

struct __attribute__((packed, aligned(1))) MdU64u { uint64_t v; };

// what the walk does with the string: count it, or write it into at most `cap` bytes and count on (n > cap: it did not fit, nothing was written past cap)
struct MdCount {
	int n = 0;
	__device__ __forceinline__ void ch(uint32_t) { n++; }
	__device__ __forceinline__ void num(uint32_t v) { n += u32_chars(v); }
};
struct MdWrite {
	char *p;
	int cap, n = 0;
	__device__ __forceinline__ MdWrite(char *to, int room) : p(to), cap(room) {}
	__device__ __forceinline__ void ch(uint32_t c) { if (n < cap) p[n] = (char)c; n++; }
	__device__ __forceinline__ void num(uint32_t v)
	{
		const int k = u32_chars(v);
		if (n + k <= cap) for (int i = k - 1; i >= 0; --i) { p[n + i] = (char)('0' + (int)(v % 10u)); v /= 10u; }
		n += k;
	}
};

__device__ __forceinline__ uint32_t md_base_char(uint32_t code) { return (0x54474341u >> (8u * (code & 3u))) & 0xFFu; }      // "ACGT"[code]

// 32 bases of the forward text from position p (0 <= p < genome_size: the nine bytes lie inside the text's allocation, which holds both strands and 16 more)
__device__ __forceinline__ uint64_t md_text32(const uint8_t *text, int64_t p)
{
	const uint8_t *tp = text + ((uint64_t)p >> 2);
	const uint64_t lo = reinterpret_cast<const MdU64u *>(tp)->v, hi = tp[8];
	const int sh = ((int)p & 3) << 1;
	return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// character i of SEQ as printed
__device__ __forceinline__ uint32_t md_shown(const uint8_t *seq, int rlen, bool flip, int i)
{
	if (i < 0 || i >= rlen) return 'N';
	return flip ? comp_char(seq[rlen - 1 - i]) : seq[i];
}

// characters [i0, i0 + 8) of SEQ as printed, lowest first; those at or beyond rlen are 0.  Nothing outside seq[0, rlen) is read
__device__ __forceinline__ uint64_t md_shown8(const uint8_t *seq, int rlen, bool flip, int i0)
{
	if (i0 >= 0 && i0 + 8 <= rlen) {
		if (!flip) return reinterpret_cast<const MdU64u *>(seq + i0)->v;
		return comp8(__builtin_bswap64(reinterpret_cast<const MdU64u *>(seq + rlen - 8 - i0)->v));
	}
	uint64_t w = 0;
	for (int j = 0; j < 8; ++j)
		if (i0 + j >= 0 && i0 + j < rlen) w |= (uint64_t)md_shown(seq, rlen, flip, i0 + j) << (8 * j);
	return w;
}

// 0x80 in every byte of x that equals c, exactly (no carry between bytes)
__device__ __forceinline__ uint64_t md_eq8(uint64_t x, uint64_t c)
{
	const uint64_t t = x ^ (c * 0x0101010101010101ull), L = 0x7F7F7F7F7F7F7F7Full;
	return ~(((t & L) + L) | t | L);
}

// the low two bits of each of eight bytes -> sixteen bits, byte j at bits 2j
__device__ __forceinline__ uint64_t md_gather2(uint64_t t)
{
	t = (t | t >> 6) & 0x000F000F000F000Full;
	t = (t | t >> 12) & 0x000000FF000000FFull;
	return (t | t >> 24) & 0xFFFFull;
}

// columns [i0, i0 + 32) of SEQ as printed: their 2-bit codes (the text's: A 0, C 1, G 2, T 3) at bits 2j, `bad` bit 2j = character j is none of ACGT in
// either case, `eqs` bit 2j = it is '='
__device__ __forceinline__ uint64_t md_read32(const uint8_t *seq, int rlen, bool flip, int i0, int m, uint64_t &bad, uint64_t &eqs)
{
	uint64_t codes = 0;
	bad = 0; eqs = 0;
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		if (8 * q >= m) break;
		const uint64_t w = md_shown8(seq, rlen, flip, i0 + 8 * q), u = w & 0xDFDFDFDFDFDFDFDFull;
		const uint64_t ok = md_eq8(u, 0x41) | md_eq8(u, 0x43) | md_eq8(u, 0x47) | md_eq8(u, 0x54);
		// bits 2:1 of the letter are a Gray code of the base (A 00, C 01, T 10, G 11): g ^ (g >> 1) is the text's code
		uint64_t g = (u >> 1) & 0x0303030303030303ull;
		g ^= (g >> 1) & 0x0101010101010101ull;
		codes |= md_gather2(g) << (16 * q);
		bad |= md_gather2((~ok >> 7) & 0x0101010101010101ull) << (16 * q);
		eqs |= md_gather2((md_eq8(w, 0x3D) >> 7) & 0x0101010101010101ull) << (16 * q);
	}
	return codes;
}

// the character MD shows for base `at` (0-based) of the contig [c0, c0 + clen) of the forward text: 'N' outside it, a hole's own character inside one
__device__ __forceinline__ uint32_t md_ref_char(const MdRef &R, int64_t c0, int64_t clen, int64_t at)
{
	if (at < 0 || at >= clen || c0 < 0 || c0 + at >= R.genome_size) return 'N';
	const int64_t g = c0 + at;
	int lo = 0, hi = R.n_holes;              // the first hole that ends behind g
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (R.hole_start[mid] + R.hole_len[mid] > g) hi = mid; else lo = mid + 1;
	}
	if (lo < R.n_holes && R.hole_start[lo] <= g) return R.hole_char[lo];
	return md_base_char((uint32_t)(R.text[(uint64_t)g >> 2] >> (((int)g & 3) << 1)));
}

// MD of record rec of a read whose characters, as held, are seq[0, rlen); the string goes to e (MdCount / MdWrite)
template <class E>
__device__ __forceinline__ void md_walk(const MdRef &R, const kg_aln_record &rec, const uint8_t *seq, int rlen, E &e)
{
	const bool flip = rec.flip != 0;
	const int n_cig = rec.cigar_len <= KG_ALN_CIGAR_MAX ? rec.cigar_len : 0;      // (a pooled CIGAR belongs to the long-read report: the stream makes none)
	int64_t ref_len = 0;
	{
		uint32_t num = 0;
		for (int i = 0; i < n_cig; ++i) {
			const char op = rec.cigar[i];
			if (op >= '0' && op <= '9') { num = num * 10u + (uint32_t)(op - '0'); continue; }
			if (op == 'M' || op == 'D' || op == 'N' || op == '=' || op == 'X') ref_len += num;
			num = 0;
		}
	}
	const bool chr_ok = rec.chr >= 0 && rec.chr < R.n_chr;
	const int64_t c0 = chr_ok ? R.chr_fwd_start[rec.chr] : -1, clen = chr_ok ? R.chr_len[rec.chr] : 0;
	int64_t at = rec.pos - 1;
	// the fast form: every reference base of the record lies inside the contig (and the contig inside the text) and outside every hole
	bool plain = chr_ok && at >= 0 && at + ref_len <= clen && c0 >= 0 && c0 + clen <= R.genome_size;
	if (plain && R.n_holes > 0) {
		const int64_t g0 = c0 + at;
		int lo = 0, hi = R.n_holes;          // the first hole that ends behind g0
		while (lo < hi) {
			const int mid = (lo + hi) >> 1;
			if (R.hole_start[mid] + R.hole_len[mid] > g0) hi = mid; else lo = mid + 1;
		}
		if (lo < R.n_holes && R.hole_start[lo] < g0 + ref_len) plain = false;
	}
	int r = 0;
	uint32_t run = 0, num = 0;
	for (int i = 0; i < n_cig; ++i) {
		const char op = rec.cigar[i];
		if (op >= '0' && op <= '9') { num = num * 10u + (uint32_t)(op - '0'); continue; }
		const int n = (int)num;
		num = 0;
		if (op == 'M' || op == '=' || op == 'X') {
			if (plain) {
				for (int k = 0; k < n; k += 32) {
					const int m = n - k < 32 ? n - k : 32;
					const uint64_t tw = md_text32(R.text, c0 + at + k);
					uint64_t bad, eqs;
					const uint64_t x = tw ^ md_read32(seq, rlen, flip, r + k, m, bad, eqs);
					uint64_t mis = (((x | x >> 1) & 0x5555555555555555ull) | bad) & ~eqs;
					if (m < 32) mis &= (1ull << (2 * m)) - 1ull;
					int prev = 0;
					while (mis) {
						const int j = (__ffsll((unsigned long long)mis) - 1) >> 1;
						mis &= mis - 1;
						e.num(run + (uint32_t)(j - prev));
						e.ch(md_base_char((uint32_t)(tw >> (2 * j))));
						run = 0; prev = j + 1;
					}
					run += (uint32_t)(m - prev);
				}
			} else {
				for (int k = 0; k < n; ++k) {
					const uint32_t g = md_ref_char(R, c0, clen, at + k), c = md_shown(seq, rlen, flip, r + k), u = c & 0xDFu;
					const bool base = g == 'A' || g == 'C' || g == 'G' || g == 'T';
					if (c == '=' || (base && u == g)) run++;
					else { e.num(run); e.ch(g); run = 0; }
				}
			}
			at += n; r += n;
		} else if (op == 'D') {
			e.num(run); e.ch('^'); run = 0;
			for (int k = 0; k < n; ++k) e.ch(md_ref_char(R, c0, clen, at + k));
			at += n;
		} else if (op == 'N') at += n;
		else if (op == 'I' || op == 'S') r += n;
	}
	e.num(run);
}
