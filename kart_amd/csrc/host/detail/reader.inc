// host/detail/reader.inc -- input: getline()/gzgets() readers, mapped FASTQ, inflated gz text (src/GetData.cpp).
// A fragment of mapper.cpp (included there, inside namespace kart { namespace { ... } }); not a translation unit of its own.
// ----------------------------------------------------------------------------------------------
// input (src/GetData.cpp)
// ----------------------------------------------------------------------------------------------
struct Input {
	FILE *fp = nullptr;
	gzFile gz = nullptr;
	char *line = nullptr;
	size_t cap = 0;
	std::vector<char> gzbuf;
	bool ended = false;            // the device stream took the library to its end: nothing is left for this reader
	bool keep_raw = false;         // -un / -un2: an entry keeps the bytes of the lines it consumed (OwnedRead::raw)
	~Input() { close(); }
	void close()
	{
		if (fp) fclose(fp);
		if (gz) gzclose(gz);
		fp = nullptr; gz = nullptr;
		free(line); line = nullptr; cap = 0;
	}
};

std::string_view header_view(const char *buf, int len)  // IdentifyHeaderBegPos/EndPos, src/GetData.cpp:29-49
{
	int p1 = len - 1, p2 = len - 1;
	for (int i = 1; i < len; ++i)
		if (buf[i] != '>' && buf[i] != '@') { p1 = i; break; }
	for (int i = 1; i < len; ++i)
		if (buf[i] == ' ' || buf[i] == '/' || buf[i] == '\t') { p2 = i; break; }
	return p2 > p1 ? std::string_view(buf + p1, (size_t)(p2 - p1)) : std::string_view();
}

// a read owned by the reader itself (getline()/gzgets() paths)
struct OwnedRead {
	std::string name, seq, qual;
	std::string raw;               // Input::keep_raw: the lines of the entry as they were read, one after the other
	int rlen = 0;
};

// GetNextEntry, src/GetData.cpp:51-107.  Like the reference, the last character of every line is taken
// to be the newline (SURVEY.md App. B-11).
bool next_entry_plain(Input &in, bool fastq, OwnedRead &rd)
{
	rd = OwnedRead();
	ssize_t len = getline(&in.line, &in.cap, in.fp);
	if (len == -1) return false;
	rd.name.assign(header_view(in.line, (int)len));
	if (in.keep_raw) rd.raw.assign(in.line, (size_t)len);
	if (fastq) {
		ssize_t sl = getline(&in.line, &in.cap, in.fp);
		if (sl == -1) { rd.rlen = 0; return true; }
		rd.rlen = (int)sl - 1;
		rd.seq.assign(in.line, (size_t)rd.rlen);
		if (in.keep_raw) rd.raw.append(in.line, (size_t)sl);
		// The reference reads the '+' line and the quality line into the same buffer without looking at the results (:73): in a file
		// that ends inside a record the "qualities" are whatever the buffer still holds -- the '+' line, or the bases themselves
		ssize_t held = sl, got;
		if ((got = getline(&in.line, &in.cap, in.fp)) != -1) { held = got; if (in.keep_raw) rd.raw.append(in.line, (size_t)got); }
		if ((got = getline(&in.line, &in.cap, in.fp)) != -1) { held = got; if (in.keep_raw) rd.raw.append(in.line, (size_t)got); }
		rd.qual.assign(in.line, (size_t)std::min<ssize_t>(held, rd.rlen));
		rd.qual.resize((size_t)rd.rlen, '\0');
		rd.qual = std::string(rd.qual.c_str());   // the reference treats it as a C string
	} else {
		std::string seq;
		while (true) {
			len = getline(&in.line, &in.cap, in.fp);
			if (len == -1) break;
			if (in.line[0] == '>') { fseek(in.fp, 0 - len, SEEK_CUR); break; }
			if (in.keep_raw) rd.raw.append(in.line, (size_t)len);
			in.line[len - 1] = '\0';
			seq += in.line;
		}
		rd.rlen = (int)seq.size();
		rd.seq.swap(seq);
	}
	return true;
}

bool next_entry_gz(Input &in, bool fastq, bool pacbio, OwnedRead &rd)  // gzGetNextEntry, src/GetData.cpp:145-182
{
	rd = OwnedRead();
	int buf_size = pacbio ? 1000000 : 1000;
	in.gzbuf.resize((size_t)buf_size);
	char *buf = in.gzbuf.data();
	if (gzgets(in.gz, buf, buf_size) == NULL) return false;
	int len = (int)strlen(buf);
	std::string name(header_view(buf, len));
	if (in.keep_raw) rd.raw.assign(buf, (size_t)len);
	if (!name.empty() && (buf[0] == '@' || buf[0] == '>')) {
		rd.name = name;
		// none of the three further gzgets() results is looked at (:168-175): in a stream that ends inside a record the buffer keeps
		// the last line that did arrive, and that is what the reference takes for the bases / the qualities
		if (gzgets(in.gz, buf, buf_size) != NULL && in.keep_raw) rd.raw.append(buf);
		rd.rlen = (int)strlen(buf) - 1;
		if (rd.rlen < 0) rd.rlen = 0;
		rd.seq.assign(buf, (size_t)rd.rlen);
		if (fastq) {
			if (gzgets(in.gz, buf, buf_size) != NULL && in.keep_raw) rd.raw.append(buf);
			if (gzgets(in.gz, buf, buf_size) != NULL && in.keep_raw) rd.raw.append(buf);
			rd.qual.assign(buf, std::min<size_t>(strlen(buf), (size_t)rd.rlen));
		}
	}
	return true;
}

bool next_entry(Input &in, bool fastq, bool pacbio, OwnedRead &rd)
{
	if (in.ended) return false;
	return in.gz ? next_entry_gz(in, fastq, pacbio, rd) : next_entry_plain(in, fastq, rd);
}

// GetNextChunk, src/GetData.cpp:109-143 / 184-219
int next_chunk(const Ctx &cx, bool sep, Input &in1, Input &in2, std::deque<OwnedRead> &reads, int limit)
{
	int count = 0;
	OwnedRead rd;
	while (true) {
		if (!next_entry(in1, cx.fastq, cx.opt.pacbio, rd) || rd.rlen == 0) break;
		reads.push_back(rd);
		count++;
		bool ok = sep ? next_entry(in2, cx.fastq, cx.opt.pacbio, rd) : next_entry(in1, cx.fastq, cx.opt.pacbio, rd);
		if (!ok || rd.rlen == 0) break;
		if (cx.opt.paired) {   // mate 2 is stored reverse-complemented, qualities reversed, :125-135
			rd.seq = revcomp(rd.seq);
			if (cx.fastq) std::reverse(rd.qual.begin(), rd.qual.end());
		}
		reads.push_back(rd);
		count++;
		if (count == limit) break;
	}
	return count;
}

// ---- fast path for plain FASTQ: the file is mapped, record boundaries are found with memchr by one
// thread (exactly the line structure GetNextEntry walks with four getline() calls), and the reads are
// materialised (copies, mate-2 reverse complement) by the worker threads.
// a text that is still being written behind the bytes that exist (the inflated text of a gz file, written by a thread of its own: GzProducer,
// batch_reader.inc): the device stream reads it like a mapped plain file, a block after the other
struct GrowingText {
	virtual ~GrowingText() {}
	// waits until bytes [0, upto) exist or the text has ended; returns how many exist.  ended: nothing will follow them
	virtual size_t wait_for(size_t upto, bool &ended) = 0;
	virtual void release(size_t below) = 0;        // nobody reads in front of this byte any more
};

struct MappedFile {
	GrowingText *grow = nullptr;   // != nullptr: data[0, size) is what exists so far of a growing text (size is raised by whoever waited for more)
	const char *data = nullptr;
	size_t size = 0, pos = 0;
	bool mapped = false;
	size_t map_size = 0;           // bytes mapped (size may be lowered to the end of this process's shard)
	int fd = -1;                   // kept open beside the mapping: the stream's lanes pread() their blocks (no page-table work per input page)
	~MappedFile() { if (data && mapped) munmap(const_cast<char *>(data), map_size); if (fd >= 0 && mapped) ::close(fd); }
	// a block of text owned by someone else (the inflated part of a gz file that a batch holds)
	bool gz_lines = false;         // the text is an inflated gz stream: a record cut short is read the way gzGetNextEntry does (view_next)
	void attach(const char *text, size_t n) { data = text; size = n; pos = 0; line_end.clear(); next_line = 0; }
	bool open(const std::string &path)
	{
		int fd = ::open(path.c_str(), O_RDONLY);
		if (fd < 0) return false;
		struct stat sb;
		if (fstat(fd, &sb) != 0 || sb.st_size == 0) { ::close(fd); return false; }
		void *p = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
		if (p == MAP_FAILED) { ::close(fd); return false; }
		this->fd = fd;
		madvise(p, (size_t)sb.st_size, MADV_SEQUENTIAL);
		data = (const char *)p;
		size = map_size = (size_t)sb.st_size;
		mapped = true;
		return true;
	}
	// getline(): returns the line length including the newline when there is one, -1 at end of file
	ssize_t line(const char *&start)
	{
		if (pos >= size) return -1;
		start = data + pos;
		size_t len;
		if (next_line < line_end.size()) len = line_end[next_line++] - pos;      // indexed window
		else {
			const char *nl = (const char *)memchr(start, '\n', size - pos);
			len = nl ? (size_t)(nl - start) + 1 : size - pos;
		}
		pos += len;
		return (ssize_t)len;
	}
	// Index the lines of the next `bytes` of the file with all workers: every worker records the line ends of its slice (one
	// sweep over the text), a prefix sum places the slices' lists in line_end.
	template <class PoolT>
	void index_ahead(PoolT &pool, size_t bytes)
	{
		line_end.clear(); next_line = 0;
		size_t lo = pos, hi = std::min(size, pos + bytes);
		if (hi <= lo) return;
		int parts = std::max(1, std::min<int>(pool.size() * 4, (int)((hi - lo) >> 16) + 1));
		std::vector<size_t> cnt((size_t)parts + 1, 0);
		if (slice_ends.size() < (size_t)parts) slice_ends.resize((size_t)parts);
		auto slice = [&](int t, size_t &a, size_t &b) { a = lo + (hi - lo) * (size_t)t / (size_t)parts; b = lo + (hi - lo) * (size_t)(t + 1) / (size_t)parts; };
		pool.run(parts, [&](int t) {
			size_t a, b;
			slice(t, a, b);
			std::vector<size_t> &mine = slice_ends[(size_t)t];     // (keeps its capacity from batch to batch)
			mine.clear();
			for (const char *p = data + a, *e = data + b; p < e;) {
				const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
				if (!nl) break;
				mine.push_back((size_t)(nl - data) + 1);
				p = nl + 1;
			}
			cnt[(size_t)t + 1] = mine.size();
		});
		for (int t = 0; t < parts; ++t) cnt[(size_t)t + 1] += cnt[(size_t)t];
		line_end.resize(cnt[(size_t)parts]);
		pool.run(parts, [&](int t) {
			const std::vector<size_t> &mine = slice_ends[(size_t)t];
			if (!mine.empty()) memcpy(line_end.data() + cnt[(size_t)t], mine.data(), mine.size() * sizeof(size_t));
		});
	}
	std::vector<std::vector<size_t>> slice_ends;
	std::vector<size_t> line_end;   // absolute end offsets (one past the newline) of the indexed lines
	size_t next_line = 0;
};

struct RecView {
	const char *hdr, *seq, *qual;
	int hdr_len, rlen, qual_len;
	int raw_len;  // bytes from hdr through the last line the entry consumed (-un / -un2: Read::raw)
	bool flip;    // mate 2 of a pair: stored reverse-complemented (src/GetData.cpp:125-135)
};

// GetNextEntry on a mapped FASTQ (same arithmetic as next_entry_plain)
bool view_next(MappedFile &f, RecView &v)
{
	const char *p;
	ssize_t len = f.line(p);
	if (len == -1) return false;
	v.hdr = p; v.hdr_len = (int)len; v.raw_len = (int)len;
	// A file that ends inside a record: the reference reads the remaining lines into one buffer without looking at the results
	// (src/GetData.cpp:73, :168-175), so a line that never came is whatever the buffer still held -- `held` below.  getline()'s
	// caller does check the sequence line (:69); gzgets()'s does not and takes the header line for the bases.
	const char *held = p;
	ssize_t held_len = len, got;
	ssize_t sl = f.line(p);
	if (sl == -1) {
		if (!f.gz_lines) { v.rlen = 0; v.seq = v.qual = nullptr; v.qual_len = 0; return true; }
		p = held; sl = held_len;
	} else { held = p; held_len = sl; }
	v.seq = p; v.rlen = (int)sl - 1;
	if ((got = f.line(p)) != -1) { held = p; held_len = got; }
	if ((got = f.line(p)) != -1) { held = p; held_len = got; }
	v.qual = held; v.qual_len = (int)held_len;
	v.raw_len = (int)(f.data + f.pos - v.hdr);           // (the lines lie one behind the other: through the last one that came)
	return true;
}

// ---- FASTA on a mapped text (the device stream, stream.inc) ----
// bytes per record of a FASTA text, from the header lines (first byte '>') in [lo, hi); fewer than two: the default
double fasta_bytes_per_record(const char *data, size_t lo, size_t hi)
{
	int64_t headers = 0;
	for (const char *p = data + lo, *e = data + hi; p < e;) {
		if (*p == '>') headers++;
		const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
		if (!nl) break;
		p = nl + 1;
	}
	return headers >= 2 ? (double)(hi - lo) / (double)headers : 400.0;
}

// GetNextEntry on a mapped FASTA text as a view -- the arithmetic of next_entry_plain(), or (f.gz_lines) of next_entry_gz(): the header line, the
// first sequence line, the sequence's length, and whether it lies in more than that one line (fasta_join then makes it one string).
// `f` is a cursor without a line index.
struct FastaView {
	const char *hdr = nullptr, *seq = nullptr;
	int hdr_len = 0, rlen = 0;
	bool joined = false;
	size_t seq_pos = 0;           // where the first line behind the header starts
	size_t raw_len = 0;           // bytes from hdr through the last line the entry consumed (-un / -un2)
};

bool fasta_view_next(MappedFile &f, FastaView &v)
{
	const char *p;
	ssize_t len = f.line(p);
	if (len == -1) return false;
	v = FastaView();
	v.hdr = p; v.hdr_len = (int)len; v.seq_pos = f.pos; v.raw_len = (size_t)len;
	if (f.gz_lines) {
		if (header_view(p, (int)len).empty() || (p[0] != '@' && p[0] != '>')) return true;
		ssize_t sl = f.line(p);
		if (sl == -1) { p = v.hdr; sl = len; }            // (the buffer still holds the header line, next_entry_gz)
		v.seq = p; v.rlen = std::max(0, (int)sl - 1);
		v.raw_len = (size_t)(f.data + f.pos - v.hdr);
		return true;
	}
	int lines = 0;
	for (;;) {
		const size_t at = f.pos;
		ssize_t sl = f.line(p);
		if (sl == -1) break;
		if (p[0] == '>') { f.pos = at; break; }
		if (lines++ == 0) v.seq = p;
		v.rlen += (int)sl - 1;
	}
	v.joined = lines > 1;
	v.raw_len = (size_t)(f.data + f.pos - v.hdr);
	return true;
}

// the sequence lines of a record of a plain FASTA text, each without its last byte, one after the other (v.rlen bytes)
void fasta_join(const char *data, size_t size, const FastaView &v, char *out)
{
	MappedFile f;
	f.data = data; f.size = size; f.pos = v.seq_pos;
	const char *p;
	for (ssize_t sl; (sl = f.line(p)) != -1 && p[0] != '>'; out += sl - 1) memcpy(out, p, (size_t)(sl - 1));
}

// The records whose four lines all lie in the indexed window, as views -- the same arithmetic as view_next(), but for all
// records at once on the pool (the serial walk was the largest serial piece of the reader: ~80 ns per read)
template <class PoolT>
void views_of_indexed_records(PoolT &pool, const MappedFile &f, std::vector<RecView> &out)
{
	size_t n = f.line_end.size() / 4;
	out.resize(n);
	if (n == 0) return;
	const size_t first = f.pos;
	const char *data = f.data;
	const std::vector<size_t> &le = f.line_end;
	int parts = std::max(1, std::min<int>(pool.size() * 4, (int)(n >> 12) + 1));
	pool.run(parts, [&](int t) {
		for (size_t j = n * (size_t)t / (size_t)parts, e = n * (size_t)(t + 1) / (size_t)parts; j < e; ++j) {
			size_t l0 = j == 0 ? first : le[4 * j - 1], l1 = le[4 * j], l2 = le[4 * j + 1], l3 = le[4 * j + 2], l4 = le[4 * j + 3];
			RecView &v = out[j];
			v.hdr = data + l0; v.hdr_len = (int)(l1 - l0);
			v.seq = data + l1; v.rlen = (int)(l2 - l1) - 1;
			v.qual = data + l3; v.qual_len = (int)(l4 - l3);
			v.raw_len = (int)(l4 - l0);
			v.flip = false;
		}
	});
}

// The read as the reference holds it (mate 2 reverse-complemented, App. B-2), its bases written to `enc` -- the batch's
// character buffer for the seeding call -- on the way: a flipped mate's sequence exists only there, and its qualities stay the
// file's bytes, marked as held reversed (the SAM writers reverse, or not, when they print them).
void materialise(const RecView &v, Read &rd, char *enc)
{
	rd = Read();
	rd.name = header_view(v.hdr, v.hdr_len);
	rd.raw = std::string_view(v.hdr, (size_t)v.raw_len);      // (a view: nothing is copied; read only under -un / -un2)
	rd.rlen = v.rlen;
	int ql = std::min(v.qual_len, v.rlen);
	const char *z = ql > 0 ? (const char *)memchr(v.qual, '\0', (size_t)ql) : nullptr;
	if (z) ql = (int)(z - v.qual);
	rd.qual = std::string_view(v.qual ? v.qual : "", (size_t)ql);
	if (!v.flip) {
		memcpy(enc, v.seq, (size_t)v.rlen);
		rd.seq = std::string_view(v.seq, (size_t)v.rlen);
		return;
	}
	revcomp_into(enc, v.seq, (size_t)v.rlen);
	rd.seq = std::string_view(enc, (size_t)v.rlen);
	rd.qual_rev = true;
}

// GetNextChunk over mapped files: the same loop as next_chunk(), producing views
int next_chunk_views(const Ctx &cx, bool sep, MappedFile &f1, MappedFile &f2, std::vector<RecView> &views, int limit)
{
	int count = 0;
	RecView v;
	while (true) {
		if (!view_next(f1, v) || v.rlen == 0) break;
		v.flip = false;
		views.push_back(v);
		count++;
		bool ok = sep ? view_next(f2, v) : view_next(f1, v);
		if (!ok || v.rlen == 0) break;
		v.flip = cx.opt.paired;
		views.push_back(v);
		count++;
		if (count == limit) break;
	}
	return count;
}

bool is_fastq(const std::string &path)  // CheckReadFormat, src/GetData.cpp:8-16
{
	gzFile f = gzopen(path.c_str(), "rb");
	if (!f) return true;
	char c = 0;
	gzread(f, &c, 1);
	gzclose(f);
	return c == '@';
}
