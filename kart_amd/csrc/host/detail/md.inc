// host/detail/md.inc -- the MD:Z field of a mapped record (-md; SAM specification v1, section 1.5: [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*).
// A fragment of mapper.cpp (included by detail/sam.inc, inside namespace kart { namespace { ... } }); not a translation unit of its own.
//
// The reference prints no MD.  It is a function of the record's printed SEQ, its CIGAR, its contig and POS and the forward strand of the
// reference, by samtools calmd's rule: an M column matches when the upper-cased read character is one of ACGT and equals the reference base,
// or when the read character is '='; anything else is a mismatch and shows the reference base.  D shows '^' and the deleted bases; I and S
// consume read only; N skips reference; H and P nothing; = and X compare like M.  A reference position inside a hole of .amb (a run of N or
// another IUPAC code in the FASTA, random bases in .pac) shows the hole's own character and matches nothing but '='; a position outside the
// contig (CheckCoordinateValidity excludes it) shows 'N'.  The device prints the same string (kernels/md_tag.inc); the two share no code.

// bytes that hold "MD:Z:" and the string of any record with this CIGAR: a number in front (1), at most two characters per M column (the base and the
// number behind it: a run of k matches prints at most k digits), '^', the bases and a number per deletion -- 2 * reference length + 2 per operation + 1
inline size_t md_room(std::string_view cigar)
{
	size_t ref = 0, num = 0;
	for (char ch : cigar) {
		if (ch >= '0' && ch <= '9') { num = num * 10 + (size_t)(ch - '0'); continue; }
		if (ch == 'M' || ch == 'D' || ch == '=' || ch == 'X') ref += num;
		num = 0;
	}
	return 2 * ref + 2 * cigar.size() + 16;
}

inline char *md_num(char *p, long long v)      // a count, as "%lld" prints it
{
	char buf[24];
	int n = 0;
	do { buf[n++] = (char)('0' + v % 10); v /= 10; } while (v);
	while (n) *p++ = buf[--n];
	return p;
}

// the reference character MD shows at base `at` (0-based) of contig c
inline char md_ref_char(const RefData &ref, const Contig &c, int64_t at)
{
	if (at < 0 || at >= c.len) return 'N';
	const int64_t g = c.fwd_start + at;
	std::vector<Hole>::const_iterator it = std::upper_bound(ref.holes.begin(), ref.holes.end(), g, [](int64_t v, const Hole &h) { return v < h.start; });
	if (it != ref.holes.begin() && g < (it - 1)->start + (it - 1)->len) return (it - 1)->ch;
	return ref.seq[(size_t)g];
}

// shown[0, n): SEQ as the record prints it; pos: 1-based on contig chr_idx.  Returns the end of the string written at p (md_room() bytes are there)
inline char *md_put(char *p, const RefData &ref, int chr_idx, long long pos, std::string_view cigar, const char *shown, size_t n)
{
	const Contig &c = ref.contigs[(size_t)chr_idx];
	int64_t at = pos - 1;            // reference base of the next column
	size_t r = 0;                    // read character of the next column
	long long run = 0, num = 0;
	for (char op : cigar) {
		if (op >= '0' && op <= '9') { num = num * 10 + (op - '0'); continue; }
		if (op == 'M' || op == '=' || op == 'X') {
			for (long long k = 0; k < num; ++k, ++at, ++r) {
				const char g = md_ref_char(ref, c, at);
				const char ch = r < n ? shown[r] : 'N';
				const char u = (char)(ch & 0xDF);
				const bool plain = g == 'A' || g == 'C' || g == 'G' || g == 'T';      // (a hole's character, or 'N' outside the contig: no match)
				if (ch == '=' || (plain && u == g)) run++;
				else { p = md_num(p, run); *p++ = g; run = 0; }
			}
		} else if (op == 'D') {
			p = md_num(p, run); *p++ = '^'; run = 0;
			for (long long k = 0; k < num; ++k, ++at) *p++ = md_ref_char(ref, c, at);
		} else if (op == 'N') at += num;
		else if (op == 'I' || op == 'S') r += (size_t)num;
		num = 0;
	}
	return md_num(p, run);
}
