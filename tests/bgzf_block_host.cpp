// tests/bgzf_block_host.cpp -- the device's BGZF block deflater (kart_amd/csrc/kernels/bgzf_block.inc) as a plain host program: with
// BGZF_HOST_EMULATION the same text runs thread after thread, where the sanitizers and a debugger reach it (tests/test_bgzf_block_cpu.py).
// usage: bgzf_block_host IN OUT -- IN cut every 0xff00 bytes, one member per piece, written back to back to OUT
#define BGZF_HOST_EMULATION 1
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/bgzf_block.inc"

using namespace kg::bgzf;

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<uint8_t> in;
	for (int c; (c = fgetc(f)) != EOF;) in.push_back((uint8_t)c);
	fclose(f);
	FILE *o = fopen(argv[2], "wb");
	if (!o) { perror(argv[2]); return 2; }
	static BlockShared sh;
	static_assert(sizeof(BlockShared) <= 160 * 1024, "a workgroup's LDS");
	unsigned long long errors = 0;
	for (size_t at = 0; at < in.size(); at += kPayloadMax) {
		const int n = (int)std::min<size_t>(kPayloadMax, in.size() - at);
		std::vector<uint8_t> src(in.begin() + (long)at, in.begin() + (long)at + n);      // (of the piece's own size: a read past its end is seen)
		std::vector<uint32_t> out(kMemberMax / 4, 0xAAAAAAAAu);
		const int m = deflate_block(sh, src.data(), n, out.data(), &errors);
		if (m <= 0 || m > kMemberMax || errors) { fprintf(stderr, "piece at %zu: member of %d bytes, %llu errors\n", at, m, errors); return 1; }
		fwrite(out.data(), 1, (size_t)m, o);
	}
	fclose(o);
	return 0;
}
