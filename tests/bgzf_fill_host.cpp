// tests/bgzf_fill_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// GzText::fill_bgzf() (kart_amd/csrc/host/detail/batch_reader.inc) with a MemberInflater in the place of its zlib threads, without a device: the
// inflater is the device's decoder compiled for the host (kernels/bgzf_inflate.inc with BGZF_HOST_EMULATION, as tests/bgzf_inflate_host.cpp runs
// it).  The file's text is drawn twice -- through GzText::fill() in rounds of a few MB, and through a GzProducer's growing block the way the device
// stream draws it (fill_direct) -- and written to OUT.fill and OUT.producer; tests/test_bgzf_inflate_cpu.py compares them with what the same
// program writes with no inflater set.
// usage: bgzf_fill_host FILE OUT none|emu|emu-fail2 [threads]      (emu-fail2: the inflater's second run() returns false)
// stdout: one JSON line with the counters of both passes.
#include <fcntl.h>
#include <immintrin.h>
#include <sched.h>
#include <signal.h>
#include <pthread.h>
#include <sys/file.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/statvfs.h>
#include <sys/vfs.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <functional>
#include <future>
#include <malloc.h>
#include <memory>
#include <mutex>
#include <string_view>
#include <thread>

#include "../kart_amd/csrc/host/mapper.hpp"

#define BGZF_HOST_EMULATION 1
#include "../kart_amd/csrc/kernels/bgzf_block.inc"
#include "../kart_amd/csrc/kernels/bgzf_inflate.inc"

namespace kart {
namespace {
#include "../kart_amd/csrc/host/detail/types.inc"
#include "../kart_amd/csrc/host/detail/normal_pairs.inc"
#include "../kart_amd/csrc/host/detail/kmer.inc"
#include "../kart_amd/csrc/host/detail/gap_closing.inc"
#include "../kart_amd/csrc/host/detail/report.inc"
#include "../kart_amd/csrc/host/detail/pairing.inc"
#include "../kart_amd/csrc/host/detail/sam.inc"
#include "../kart_amd/csrc/host/detail/bam.inc"
#include "../kart_amd/csrc/host/detail/reader.inc"
#include "../kart_amd/csrc/host/detail/shard.inc"
#include "../kart_amd/csrc/host/detail/chunk_state.inc"
#include "../kart_amd/csrc/host/detail/writer.inc"
#include "../kart_amd/csrc/host/detail/chunk_stages.inc"
#include "../kart_amd/csrc/host/detail/pgzip.inc"
#include "../kart_amd/csrc/host/detail/batch_reader.inc"

// every member from a buffer of exactly its own size into one of exactly its text's size: an access past either end is the sanitizer's
struct EmulatedInflater : MemberInflater {
	std::vector<unsigned char> members, text;
	std::vector<int32_t> status;
	kg::bgzf::InflateShared sh;
	int calls = 0, fail_at = 0;
	unsigned char *src(size_t bytes) override
	{
		if (bytes > members.size()) members.resize(bytes);
		return members.data();
	}
	bool run(size_t src_bytes, const int64_t *member_off, const int64_t *text_off, size_t n, const unsigned char *&t, const int32_t *&s) override
	{
		if (++calls == fail_at) return false;
		if (member_off[n] != (int64_t)src_bytes || src_bytes > members.size()) return false;
		text.assign((size_t)text_off[n], 0);
		status.assign(n, -1);
		for (size_t i = 0; i < n; ++i) {
			const size_t m_bytes = (size_t)(member_off[i + 1] - member_off[i]), t_bytes = (size_t)(text_off[i + 1] - text_off[i]);
			unsigned char *m = (unsigned char *)malloc(m_bytes), *out = (unsigned char *)malloc(t_bytes);
			memcpy(m, members.data() + member_off[i], m_bytes);
			status[i] = kg::bgzf::inflate_member(sh, m, (int)m_bytes, out, (int)t_bytes);
			if (status[i] == 0 && t_bytes) memcpy(text.data() + text_off[i], out, t_bytes);
			free(m); free(out);
		}
		t = text.data(); s = status.data();
		return true;
	}
};

struct Opened {
	GzText g;
	gzFile in = nullptr;
	bool open(const char *path, int threads, const std::string &mode)
	{
		in = gzopen(path, "rb");
		if (!in) return false;
		gzbuffer(in, 1 << 20);
		g.f = in;
		g.path = path;
		g.silent = true;
		if (!g.try_bgzf(path, threads)) g.try_pgz(path, threads);
		if (mode != "none" && g.fd >= 0) {
			EmulatedInflater *e = new EmulatedInflater;
			e->fail_at = mode == "emu-fail2" ? 2 : 0;
			g.inflater.reset(e);
		}
		return true;
	}
	~Opened() { if (in) gzclose(in); }
};

bool write_file(const std::string &path, const char *p, size_t n)
{
	FILE *f = fopen(path.c_str(), "wb");
	if (!f) return false;
	if (n) fwrite(p, 1, n, f);
	return fclose(f) == 0;
}

int run(const char *path, const std::string &out, const std::string &mode, int threads)
{
	struct stat sb;
	if (stat(path, &sb) != 0) return 2;
	int64_t counters[4] = {0, 0, 0, 0};
	{
		Opened o;
		if (!o.open(path, threads, mode)) return 2;
		std::vector<char> text;
		for (int round = 0; !o.g.eof; ++round) o.g.fill(text, ((size_t)3 << 20) + (size_t)(round % 5) * 100000);
		if (!write_file(out + ".fill", text.data(), text.size())) return 2;
		counters[0] = o.g.device_bytes; counters[1] = o.g.host_bytes;
	}
	{
		Opened o;
		if (!o.open(path, threads, mode)) return 2;
		GzProducer p;
		if (!p.start(&o.g, (size_t)sb.st_size)) return 2;
		bool ended = false;
		size_t pos = 0;
		for (;;) {
			const size_t have = p.wait_for(pos + ((size_t)5 << 20), ended);
			pos = have;
			if (ended) break;
		}
		p.stop();
		if (!write_file(out + ".producer", p.base, p.produced)) return 2;
		counters[2] = o.g.device_bytes; counters[3] = o.g.host_bytes;
	}
	printf("{\"fill_device_bytes\": %lld, \"fill_host_bytes\": %lld, \"producer_device_bytes\": %lld, \"producer_host_bytes\": %lld}\n", (long long)counters[0],
	       (long long)counters[1], (long long)counters[2], (long long)counters[3]);
	return 0;
}

}  // namespace
}  // namespace kart

int main(int argc, char **argv)
{
	if (argc < 4) { fprintf(stderr, "usage: bgzf_fill_host FILE OUT none|emu|emu-fail2 [threads]\n"); return 2; }
	return kart::run(argv[1], argv[2], argv[3], argc > 4 ? atoi(argv[4]) : 4);
}
