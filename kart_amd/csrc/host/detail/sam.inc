// host/detail/sam.inc -- flags, MAPQ and SAM text (src/Mapping.cpp:49-315).
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
// ----------------------------------------------------------------------------------------------
// SAM text (src/Mapping.cpp:177-315; record formats in SURVEY.md App. D)
// ----------------------------------------------------------------------------------------------
#include "md.inc"       // the MD:Z field (-md); a part of this fragment: whoever includes the printer has it

inline void append_int(std::string &out, long long v)   // what "%d" / "%lld" print
{
	char buf[24];
	int n = 0;
	unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
	do { buf[n++] = (char)('0' + u % 10); u /= 10; } while (u);
	if (v < 0) buf[n++] = '-';
	while (n) out += buf[--n];
}

inline void append_qual(std::string &out, const Read &rd);

// -stats: where the records this thread prints are tallied (null: nowhere) -- set around a chunk's stage C.  The three sites below that make a record's
// text (sam_unmapped, sam_mapped_fields, sam_one_record's unmapped branch) are the only ones in the host pipeline, and each counts what it prints
thread_local Tally *t_tally = nullptr;
struct TallyInto {
	Tally *prev;
	explicit TallyInto(Tally *t) : prev(t_tally) { t_tally = t; }
	~TallyInto() { t_tally = prev; }
};

void sam_unmapped(const Ctx &cx, const Read &rd, std::string &out)
{
	if (t_tally) t_tally->add(rd.rep[0].flag, 0, false, 0, std::string_view());
	out += rd.name; out += '\t';
	append_int(out, rd.rep[0].flag);
	out += "\t*\t0\t0\t*\t*\t0\t0\t";
	out += rd.seq; out += '\t';
	if (cx.fastq) append_qual(out, rd); else out += '*';
	out += "\tAS:i:0\tXS:i:0";
	out += cx.rg_field;
	out += '\n';
}

// raw-pointer writers for the record below: one capacity check per record instead of one per field
inline char *put(char *p, std::string_view v) { memcpy(p, v.data(), v.size()); return p + v.size(); }
inline char *put(char *p, const char *lit, size_t n) { memcpy(p, lit, n); return p + n; }
inline char *put_int(char *p, long long v)   // what "%d" / "%lld" print
{
	char buf[24];
	int n = 0;
	unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
	do { buf[n++] = (char)('0' + u % 10); u /= 10; } while (u);
	if (v < 0) buf[n++] = '-';
	while (n) *p++ = buf[--n];
	return p;
}

// the qualities of the read as held (flip: reversed) -- `qual` itself is the file's bytes, held reversed when qual_rev
inline char *put_qual(char *p, const Read &rd, bool flip)
{
	if (flip == rd.qual_rev) return put(p, rd.qual);
	reverse_into(p, rd.qual.data(), rd.qual.size());
	return p + rd.qual.size();
}
inline void append_qual(std::string &out, const Read &rd)
{
	size_t at = out.size();
	out.resize(at + rd.qual.size());
	put_qual(&out[at], rd, false);
}

// flip: the record shows the reverse complement of the read as it is held (and its qualities reversed); written straight
// into the chunk's text, no temporaries
void sam_mapped_fields(const Ctx &cx, const Read &rd, int flag, int chr_idx, long long pos, int mapq, std::string_view cigar, bool has_mate,
                       long long mate_pos, int tlen, bool flip, int score, int sub_score, std::string &out)
{
	const std::string &chr = cx.ref.contigs[(size_t)chr_idx].name;
	if (t_tally) t_tally->add(flag, mapq, has_mate, tlen, cigar);
	size_t at = out.size();
	out.resize(at + rd.name.size() + chr.size() + cigar.size() + rd.seq.size() + rd.qual.size() + 192 + (cx.opt.md ? md_room(cigar) : 0) + cx.rg_field.size());
	char *p = &out[at];
	p = put(p, rd.name); *p++ = '\t';
	p = put_int(p, flag); *p++ = '\t';
	p = put(p, chr); *p++ = '\t';
	p = put_int(p, pos); *p++ = '\t';
	p = put_int(p, mapq); *p++ = '\t';
	p = put(p, cigar);
	if (has_mate) { p = put(p, "\t=\t", 3); p = put_int(p, mate_pos); *p++ = '\t'; p = put_int(p, tlen); *p++ = '\t'; }
	else p = put(p, "\t*\t0\t0\t", 7);
	size_t n = rd.seq.size();
	const char *const shown = p;                 // SEQ as printed: what MD compares
	if (!flip) p = put(p, rd.seq);
	else {
		revcomp_into(p, rd.seq.data(), n);      // GetComplementarySeq, src/tools.cpp:19-29
		p += n;
	}
	*p++ = '\t';
	if (!cx.fastq) *p++ = '*';
	else p = put_qual(p, rd, flip);
	p = put(p, "\tNM:i:", 6); p = put_int(p, rd.rlen - score);
	p = put(p, "\tAS:i:", 6); p = put_int(p, score);
	p = put(p, "\tXS:i:", 6); p = put_int(p, sub_score);
	if (cx.opt.md) { p = put(p, "\tMD:Z:", 6); p = md_put(p, cx.ref, chr_idx, pos, cigar, shown, n); }
	p = put(p, cx.rg_field);                     // -R: the read group, the last field (empty without)
	*p++ = '\n';
	out.resize((size_t)(p - out.data()));
}

void sam_mapped(const Ctx &cx, const Read &rd, const Report &rp, bool has_mate, long long mate_pos, int tlen, bool flip, std::string &out)
{
	sam_mapped_fields(cx, rd, rp.flag, rp.chr, (long long)rp.gPos, rd.mapq, rp.cigar, has_mate, mate_pos, tlen, flip, rd.score, rd.sub_score, out);
}

// the record kg_align_batch decided for a read (what Output{Paired,Singled}Alignments print for it, src/Mapping.cpp:177-315)
void sam_one_record(const Ctx &cx, const Read &rd, const kg_aln_record &rec, std::string &out, const char *cigar_pool = nullptr)
{
	if (rec.kind == KG_ALN_UNMAPPED) {
		if (t_tally) t_tally->add(rec);
		out += rd.name; out += '\t';
		append_int(out, rec.flag);
		out += "\t*\t0\t0\t*\t*\t0\t0\t";
		out += rd.seq; out += '\t';
		if (cx.fastq) append_qual(out, rd); else out += '*';
		out += "\tAS:i:0\tXS:i:0";
		out += cx.rg_field;
		out += '\n';
	} else if (rec.kind == KG_ALN_MAPPED) {
		std::string_view cigar(rec.cigar, rec.cigar_len);
		if (rec.cigar_len == KG_ALN_CIGAR_POOLED) {             // a long read's CIGAR lies in the batch's text pool (kg_longread_batch)
			int64_t at; int32_t bytes;
			memcpy(&at, rec.cigar, 8); memcpy(&bytes, rec.cigar + 8, 4);
			cigar = std::string_view(cigar_pool + at, (size_t)bytes);
		}
		sam_mapped_fields(cx, rd, rec.flag, rec.chr, (long long)rec.pos, rec.mapq, cigar, rec.has_mate != 0,
		                  (long long)rec.mate_pos, rec.tlen, rec.flip != 0, rec.score, rec.sub_score, out);
	}
}

// the records of read `at` of a batch: its own one and, with -m, the ones chained behind it
void sam_from_record(const Ctx &cx, const Read &rd, const kg_aln_record *recs, int64_t at, std::string &out, const char *cigar_pool = nullptr)
{
	for (; at >= 0; at = recs[at].next) sam_one_record(cx, rd, recs[at], out, cigar_pool);
}

// OutputPairedAlignments, src/Mapping.cpp:177-270.  Mate 2 is held reverse-complemented (App. B-2).
void output_pair(const Ctx &cx, const Read &r1, const Read &r2, Stats &st, PairStats &ps, std::string &out)
{
	if (r1.score == 0) { st.unmapped++; sam_unmapped(cx, r1, out); }
	else {
		if (r1.mapq == 60) st.unique++;
		for (int i = r1.best; i < r1.can_num; ++i) {
			const Report &rp = r1.rep[(size_t)i];
			if (rp.score > 0) {
				int j = rp.mate;
				if (j != -1 && r2.rep[(size_t)j].score > 0) {
					int dist = (int)(r2.rep[(size_t)j].gPos - rp.gPos + (rp.fwd ? r2.rlen : 0 - r1.rlen));
					if (i == r1.best) {
						ps.paired += 2;
						if (abs(dist) < 10000) ps.distance += abs(dist);
					}
					sam_mapped(cx, r1, rp, true, (long long)r2.rep[(size_t)j].gPos, dist, !rp.fwd, out);
				} else sam_mapped(cx, r1, rp, false, 0, 0, !rp.fwd, out);
			}
			if (!cx.opt.multi_hit) break;
		}
	}
	if (r2.score == 0) { st.unmapped++; sam_unmapped(cx, r2, out); }
	else {
		if (r2.mapq == 60) st.unique++;
		// mate 2 is held reverse-complemented (src/GetData.cpp:125-135): a forward report shows it flipped back
		for (int j = r2.best; j < r2.can_num; ++j) {
			const Report &rp = r2.rep[(size_t)j];
			if (rp.score > 0) {
				int i = rp.mate;
				if (i != -1 && r1.rep[(size_t)i].score > 0) {
					int dist = 0 - (int)(rp.gPos - r1.rep[(size_t)i].gPos + (r1.rep[(size_t)i].fwd ? r2.rlen : 0 - r1.rlen));
					sam_mapped(cx, r2, rp, true, (long long)r1.rep[(size_t)i].gPos, dist, rp.fwd, out);
				} else sam_mapped(cx, r2, rp, false, 0, 0, rp.fwd, out);
			}
			if (!cx.opt.multi_hit) break;
		}
	}
}

void output_single(const Ctx &cx, const Read &rd, Stats &st, std::string &out)  // OutputSingledAlignments, src/Mapping.cpp:272-315
{
	if (rd.score == 0) { st.unmapped++; sam_unmapped(cx, rd, out); return; }
	if (rd.mapq == 60) st.unique++;
	for (int i = rd.best; i < rd.can_num; ++i) {
		const Report &rp = rd.rep[(size_t)i];
		if (rp.score == rd.score) {
			sam_mapped(cx, rd, rp, false, 0, 0, !rp.fwd, out);
			if (!cx.opt.multi_hit) break;
		}
	}
}
