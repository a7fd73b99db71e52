// host/detail/tally.inc -- the run summary of -stats: a Tally of 64-bit counters, the ONE function that adds an output record to it, and the file's text.
// A fragment of mapper.hpp (included there, inside namespace kart); it needs <cstdint>, <string>, <string_view> and the KG_STATS_* layout of
// include/kart_amd.h: a Tally's words are a device row's words (stats_kernels.hip), widened.
//
// The file describes the records the run printed (every non-header line of -o, every record of -bo), never reads: "mapped" is FLAG & 4 == 0.
struct Tally {
	uint64_t w[KG_STATS_WORDS] = {};
	// one output record: FLAG, MAPQ and TLEN as printed, has_mate: RNEXT is "=", cigar: the CIGAR text (empty for "*")
	void add(int flag_, int mapq, bool has_mate, long long tlen, std::string_view cigar)
	{
		const unsigned flag = (unsigned)flag_;
		const bool mapped = (flag & 4) == 0, paired = (flag & 1) != 0;
		w[KG_STATS_RECORDS]++;
		for (int b = 0; b < KG_STATS_FLAG_BITS; ++b) w[KG_STATS_FLAG0 + b] += (flag >> b) & 1u;
		if (paired && (flag & 2) && mapped) w[KG_STATS_PROPER]++;
		if (paired && (flag & 12) == 0) w[KG_STATS_BOTH_MAPPED]++;
		if (paired && mapped && (flag & 8)) w[KG_STATS_SINGLETON]++;
		if (mapped) {
			const unsigned mq = (unsigned)mapq;
			w[KG_STATS_MAPQ0 + (mq < KG_STATS_MAPQ_BINS ? mq : KG_STATS_MAPQ_BINS - 1)]++;
			uint64_t v = 0;
			for (char ch : cigar) {
				if (ch >= '0' && ch <= '9') { v = v * 10 + (uint64_t)(ch - '0'); continue; }
				const int k = ch == 'M' ? 0 : ch == 'I' ? 1 : ch == 'D' ? 2 : ch == 'S' ? 3 : 4;
				w[KG_STATS_CIGAR0 + 2 * k] += v;
				w[KG_STATS_CIGAR0 + 2 * k + 1]++;
				v = 0;
			}
		}
		if (paired && has_mate && tlen > 0) w[KG_STATS_ISIZE0 + (tlen < KG_STATS_ISIZE_MAX ? (int)tlen : KG_STATS_ISIZE_MAX)]++;
	}
	// a device record (kg_aln_record) that is printed: an unmapped-kind record shows MAPQ 0, no mate and no CIGAR.  A pooled CIGAR (-pacbio) is `pooled`
	void add(const kg_aln_record &rec, std::string_view pooled = std::string_view())
	{
		if (rec.kind == KG_ALN_UNMAPPED) add(rec.flag, 0, false, 0, std::string_view());
		else if (rec.kind == KG_ALN_MAPPED)
			add(rec.flag, rec.mapq, rec.has_mate != 0, rec.tlen, rec.cigar_len == KG_ALN_CIGAR_POOLED ? pooled : std::string_view(rec.cigar, rec.cigar_len < KG_ALN_CIGAR_MAX ? rec.cigar_len : 0));
	}
	void add_row(const uint32_t *row)               // a device row (kg_stream_result::chunk_tally)
	{
		for (int i = 0; i < KG_STATS_WORDS; ++i) w[i] += row[i];
	}
	Tally &operator+=(const Tally &o)
	{
		for (int i = 0; i < KG_STATS_WORDS; ++i) w[i] += o.w[i];
		return *this;
	}
	void clear() { *this = Tally(); }
	// the -stats file
	std::string text() const
	{
		std::string out = "# kart-amd stats 1\n";
		auto row = [&out](const char *kind, const std::string &key, uint64_t a, const uint64_t *b = nullptr) {
			out += kind; out += '\t'; out += key; out += '\t'; out += std::to_string((unsigned long long)a);
			if (b) { out += '\t'; out += std::to_string((unsigned long long)*b); }
			out += '\n';
		};
		const uint64_t unmapped = w[KG_STATS_FLAG0 + 2];
		row("SN", "records", w[KG_STATS_RECORDS]);
		row("SN", "mapped", w[KG_STATS_RECORDS] - unmapped);
		row("SN", "unmapped", unmapped);
		row("SN", "proper_pair", w[KG_STATS_PROPER]);
		row("SN", "both_mapped", w[KG_STATS_BOTH_MAPPED]);
		row("SN", "singleton", w[KG_STATS_SINGLETON]);
		for (int b = 0; b < KG_STATS_FLAG_BITS; ++b) {
			char key[16];
			snprintf(key, sizeof(key), "0x%x", 1u << b);
			row("FL", key, w[KG_STATS_FLAG0 + b]);
		}
		for (int q = 0; q < KG_STATS_MAPQ_BINS; ++q)
			if (w[KG_STATS_MAPQ0 + q]) row("MQ", std::to_string(q), w[KG_STATS_MAPQ0 + q]);
		for (int d = 0; d <= KG_STATS_ISIZE_MAX; ++d)
			if (w[KG_STATS_ISIZE0 + d]) row("IS", d == KG_STATS_ISIZE_MAX ? std::string(">=") + std::to_string(d) : std::to_string(d), w[KG_STATS_ISIZE0 + d]);
		static const char *const kClass[KG_STATS_CIGAR_CLASSES] = {"M", "I", "D", "S", "other"};
		for (int k = 0; k < KG_STATS_CIGAR_CLASSES; ++k) row("CG", kClass[k], w[KG_STATS_CIGAR0 + 2 * k], &w[KG_STATS_CIGAR0 + 2 * k + 1]);
		return out;
	}
};
