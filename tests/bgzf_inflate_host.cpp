// tests/bgzf_inflate_host.cpp -- the device's BGZF member inflater (kart_amd/csrc/kernels/bgzf_inflate.inc) as a plain host program: with
// BGZF_HOST_EMULATION the same text runs lane after lane, where the sanitizers and a debugger reach it (tests/test_bgzf_inflate_cpu.py).
// usage: bgzf_inflate_host IN OUT -- IN is walked member by member along BSIZE; every member is inflated from a buffer of exactly its own
// size into one of exactly ISIZE bytes, so that an access past either end is seen.  OUT gets the text (ISIZE bytes per member, zeros where
// a member was refused in front of them), stdout one line "status" per member.
#define BGZF_HOST_EMULATION 1
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels/bgzf_block.inc"
#include "kernels/bgzf_inflate.inc"

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
	static InflateShared sh;
	static_assert(sizeof(InflateShared) <= 10 * 1024, "sixteen waves of a CU share 160 KiB of LDS");
	for (size_t at = 0; at < in.size();) {
		// BSIZE: the 'BC' subfield of the extra field
		size_t size = 0;
		if (in.size() - at >= 18 && in[at] == 0x1f && in[at + 1] == 0x8b) {
			const size_t xlen = (size_t)in[at + 10] | ((size_t)in[at + 11] << 8);
			for (size_t x = at + 12; x + 6 <= at + 12 + xlen && x + 6 <= in.size();) {
				const size_t slen = (size_t)in[x + 2] | ((size_t)in[x + 3] << 8);
				if (in[x] == 'B' && in[x + 1] == 'C' && slen == 2) { size = ((size_t)in[x + 4] | ((size_t)in[x + 5] << 8)) + 1; break; }
				x += 4 + slen;
			}
		}
		if (size < 8 || at + size > in.size()) { fprintf(stderr, "no BGZF member at %zu\n", at); return 2; }
		const uint8_t *t = in.data() + at + size - 4;
		const size_t isize = (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16) | ((size_t)t[3] << 24);
		if (isize > 65536) { printf("%d\n", (int)kInflateSize); at += size; continue; }
		uint8_t *member = (uint8_t *)malloc(size), *text = (uint8_t *)calloc(isize, 1);      // (of no byte where ISIZE is 0: nothing is written then)
		if (!member || (!text && isize)) return 2;
		memcpy(member, in.data() + at, size);
		const int status = inflate_member(sh, member, (int)size, text, (int)isize);
		printf("%d\n", status);
		if (isize) fwrite(text, 1, isize, o);
		free(member); free(text);
		at += size;
	}
	fclose(o);
	return 0;
}
