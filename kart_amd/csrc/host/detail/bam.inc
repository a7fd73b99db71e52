// host/detail/bam.inc -- BAM output (-bo): the reference turns every SAM line it would have printed into a BAM record with
// htslib's sam_parse1 / sam_write1 (src/Mapping.cpp:610-620, header :676-680).  htslib is not part of this build, so this is an
// own encoder of the same public format (SAM/BAM specification v1, sections 4.2 and 4.1 BGZF): the chunk's SAM text is parsed
// line by line exactly as it was printed and written as BGZF blocks of BAM records.
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.

// one BGZF block = one gzip member with the "BC" extra field carrying its total size - 1 (SAMv1 4.1)
void bgzf_append_block(const unsigned char *src, size_t n, std::string &out)
{
	unsigned char buf[65536 + 1024];
	z_stream zs;
	memset(&zs, 0, sizeof(zs));
	if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { fprintf(stderr, "Error! deflateInit2 failed\n"); exit(1); }
	zs.next_in = const_cast<unsigned char *>(src);
	zs.avail_in = (uInt)n;
	zs.next_out = buf + 18;
	zs.avail_out = (uInt)(sizeof(buf) - 18 - 8);
	if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "Error! deflate failed on a BGZF block\n"); exit(1); }
	size_t clen = (size_t)zs.total_out;
	deflateEnd(&zs);
	static const unsigned char head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
	memcpy(buf, head, 16);
	size_t bsize = 18 + clen + 8 - 1;
	buf[16] = (unsigned char)(bsize & 255); buf[17] = (unsigned char)(bsize >> 8);
	uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, (uInt)n), isize = (uint32_t)n;
	unsigned char *t = buf + 18 + clen;
	for (int i = 0; i < 4; ++i) { t[i] = (unsigned char)(crc >> (8 * i)); t[4 + i] = (unsigned char)(isize >> (8 * i)); }
	out.append((const char *)buf, 18 + clen + 8);
}

// raw BAM bytes -> BGZF blocks of at most 0xff00 bytes of payload (htslib's block size)
void bgzf_append(const std::string &raw, std::string &out)
{
	for (size_t at = 0; at < raw.size(); at += 0xff00)
		bgzf_append_block((const unsigned char *)raw.data() + at, std::min<size_t>(0xff00, raw.size() - at), out);
}

inline void put_u32(std::string &o, uint32_t v) { char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; o.append(b, 4); }
inline void put_u16(std::string &o, uint32_t v) { char b[2] = {(char)v, (char)(v >> 8)}; o.append(b, 2); }

// BAM header: magic, the SAM header text, the reference dictionary
std::string bam_header(const RefData &ref, const std::string &sam_header_text)
{
	std::string raw("BAM\1", 4);
	put_u32(raw, (uint32_t)sam_header_text.size());
	raw += sam_header_text;
	put_u32(raw, (uint32_t)ref.contigs.size());
	for (const Contig &c : ref.contigs) {
		put_u32(raw, (uint32_t)c.name.size() + 1);
		raw.append(c.name.c_str(), c.name.size() + 1);
		put_u32(raw, (uint32_t)c.len);
	}
	return raw;
}

inline int reg2bin(int64_t beg, int64_t end)   // SAMv1 5.3
{
	--end;
	if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

// an integer tag in the smallest type that holds it, as sam_parse1 chooses
void bam_put_int_tag(std::string &o, const char *tag, long long v)
{
	o.append(tag, 2);
	if (v < 0) {
		if (v >= -128) { o += 'c'; o += (char)v; }
		else if (v >= -32768) { o += 's'; put_u16(o, (uint32_t)(int32_t)v); }
		else { o += 'i'; put_u32(o, (uint32_t)(int32_t)v); }
	} else {
		if (v < 256) { o += 'C'; o += (char)v; }
		else if (v < 65536) { o += 'S'; put_u16(o, (uint32_t)v); }
		else { o += 'I'; put_u32(o, (uint32_t)v); }
	}
}

// one printed SAM record (without its newline) -> one BAM record appended to raw; false when the line cannot be a record
bool bam_from_sam_line(const std::map<std::string_view, int> &ref_id, const char *line, size_t len, std::string &raw)
{
	std::string_view f[11];
	size_t at = 0;
	int nf = 0;
	for (; nf < 11; ++nf) {
		const char *tab = (const char *)memchr(line + at, '\t', len - at);
		size_t e = tab ? (size_t)(tab - line) : len;
		f[nf] = std::string_view(line + at, e - at);
		at = e + 1;
		if (!tab) { ++nf; break; }
	}
	if (nf < 11) return false;
	auto to_ll = [](std::string_view s) { return strtoll(std::string(s).c_str(), nullptr, 10); };
	int flag = (int)to_ll(f[1]), mapq = (int)to_ll(f[4]);
	int64_t pos = to_ll(f[3]) - 1, pnext = to_ll(f[7]) - 1, tlen = to_ll(f[8]);
	int rid = -1, rnext = -1;
	if (f[2] != "*") { std::map<std::string_view, int>::const_iterator it = ref_id.find(f[2]); if (it == ref_id.end()) return false; rid = it->second; }
	if (f[6] == "=") rnext = rid;
	else if (f[6] != "*") { std::map<std::string_view, int>::const_iterator it = ref_id.find(f[6]); if (it == ref_id.end()) return false; rnext = it->second; }
	// CIGAR
	std::string cig;
	int n_cig = 0;
	int64_t ref_len = 0;
	if (f[5] != "*") {
		uint32_t num = 0;
		for (char ch : f[5]) {
			if (ch >= '0' && ch <= '9') { num = num * 10 + (uint32_t)(ch - '0'); continue; }
			const char *ops = "MIDNSHP=X", *w = strchr(ops, ch);
			if (!w) return false;
			int op = (int)(w - ops);
			put_u32(cig, num << 4 | (uint32_t)op);
			if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += num;
			n_cig++;
			num = 0;
		}
	}
	int64_t end = pos + (ref_len > 0 ? ref_len : 1);
	std::string_view seq = f[9], qual = f[10];
	uint32_t l_seq = seq == "*" ? 0 : (uint32_t)seq.size();
	size_t start = raw.size();
	put_u32(raw, 0);                                              // block_size, patched below
	put_u32(raw, (uint32_t)rid);
	put_u32(raw, (uint32_t)(int32_t)pos);
	raw += (char)(f[0].size() + 1);
	raw += (char)mapq;
	put_u16(raw, (uint32_t)reg2bin(pos, end));
	put_u16(raw, (uint32_t)n_cig);
	put_u16(raw, (uint32_t)flag);
	put_u32(raw, l_seq);
	put_u32(raw, (uint32_t)rnext);
	put_u32(raw, (uint32_t)(int32_t)pnext);
	put_u32(raw, (uint32_t)(int32_t)tlen);
	raw.append(f[0].data(), f[0].size());
	raw += '\0';
	raw += cig;
	static const struct Nt16 { unsigned char t[256]; Nt16() { memset(t, 15, 256); const char *c = "=ACMGRSVTWYHKDBN"; for (int i = 0; i < 16; ++i) { t[(unsigned char)c[i]] = (unsigned char)i; t[(unsigned char)tolower(c[i])] = (unsigned char)i; } } } nt16;
	for (uint32_t i = 0; i < l_seq; i += 2) {
		unsigned char hi = nt16.t[(unsigned char)seq[i]], lo = i + 1 < l_seq ? nt16.t[(unsigned char)seq[i + 1]] : 0;
		raw += (char)(hi << 4 | lo);
	}
	if (qual == "*" || qual.size() != l_seq) raw.append(l_seq, (char)0xFF);
	else for (uint32_t i = 0; i < l_seq; ++i) raw += (char)(qual[i] - 33);
	// optional fields: TAG:i:value and TAG:Z:value (what this program prints)
	while (at < len) {
		const char *tab = (const char *)memchr(line + at, '\t', len - at);
		size_t e = tab ? (size_t)(tab - line) : len;
		if (e - at >= 6 && line[at + 2] == ':' && line[at + 3] == 'i' && line[at + 4] == ':')
			bam_put_int_tag(raw, line + at, strtoll(std::string(line + at + 5, e - at - 5).c_str(), nullptr, 10));
		else if (e - at >= 5 && line[at + 2] == ':' && line[at + 3] == 'Z' && line[at + 4] == ':') {
			raw.append(line + at, 2); raw += 'Z'; raw.append(line + at + 5, e - at - 5); raw += '\0';
		}
		at = e + 1;
	}
	uint32_t block = (uint32_t)(raw.size() - start - 4);
	for (int i = 0; i < 4; ++i) raw[start + (size_t)i] = (char)(block >> (8 * i));
	return true;
}

// the SAM lines in text[at, end) -> BAM records appended to raw (a line that is no record is dropped, as sam_parse1 < 0 does)
void bam_from_sam_text(const Ctx &cx, const std::string &text, size_t at, size_t end, std::string &raw)
{
	while (at < end) {
		const char *nl = (const char *)memchr(text.data() + at, '\n', end - at);
		size_t e = nl ? (size_t)(nl - text.data()) : end;
		if (e > at) bam_from_sam_line(cx.bam_ref_id, text.data() + at, e - at, raw);
		at = e + 1;
	}
}

// a chunk of the device stream: `text` holds the lines the HOST printed, piece by piece (len[k] bytes each: the reads the device handed back, the pairs
// mapped again) -> the same pieces as uncompressed BAM records, len[] updated
void bam_raw_pieces(const Ctx &cx, std::string &text, std::vector<uint32_t> &len)
{
	std::string raw;
	raw.reserve(text.size());
	size_t at = 0;
	for (uint32_t &n : len) {
		const size_t before = raw.size();
		bam_from_sam_text(cx, text, at, at + n, raw);
		at += n;
		n = (uint32_t)(raw.size() - before);
	}
	text.swap(raw);
}

// the SAM text of a chunk -> BGZF-compressed BAM records (replaces the text in place)
void bam_encode_chunk(const Ctx &cx, std::string &text)
{
	std::string raw, out;
	raw.reserve(text.size());
	bam_from_sam_text(cx, text, 0, text.size(), raw);
	out.reserve(raw.size() / 3 + 64);
	bgzf_append(raw, out);
	text.swap(out);
}
