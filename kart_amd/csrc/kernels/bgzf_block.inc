// kernels/bgzf_block.inc -- one BGZF block (SAMv1 4.1: a gzip member with the "BC" field) deflated by one workgroup of 256 threads.
//
// The payload (at most 0xff00 bytes, htslib's size) lies in LDS beside a hash table of the latest position of every 3-byte hash.
// The block is walked in TILES of 256 positions, one per thread:
//   match    every position looks its hash up -- the table holds positions of EARLIER tiles only -- and compares against that
//            candidate and against the byte in front of it (distance 1: runs); length 3..258, distance <= 32768
//   parse    the greedy walk "take the match, skip its bytes" is a chain through the tile; the positions on it are marked by
//            pointer doubling (eight steps), the position behind the tile's last token is carried into the next tile
//   insert   the tile's positions go into the table with atomicMax on the position, so the table's state after a tile does not
//            depend on the order in which the threads got there: two runs over the same bytes give the same tokens
// Pass 1 counts the tokens' symbols, the three code tables are built from the counts (lengths limited to 15 / 7 bits), the exact
// size of the dynamic block is known from them, and it is written in pass 2 -- which finds the same tokens again and packs their
// bits tile by tile -- only where it is smaller than the stored block (payload + 5 bytes).  The tokens are never kept: what
// stays in LDS is the payload, the table and a tile's worth of state (~145 KiB of the CU's 160).
//
// The body is written as PHASES: `BZ_FOR_T { ... }` is what thread t does between two barriers, BZ_SYNC the barrier; nothing a
// thread holds in registers lives across a phase.  Compiled for the device a phase runs once per thread; with
// BGZF_HOST_EMULATION it is a loop over t and the barrier is nothing, so that the same text runs, thread after thread, in a
// plain host program (tests/bgzf_block_host.cpp), where a debugger and the sanitizers reach it.
// Rule that makes the two equal: inside a phase no thread reads what another thread writes in that phase (atomics whose result is
// not read, and marks that are only ever set, excepted).

namespace kg {
namespace bgzf {

#if defined(BGZF_HOST_EMULATION)
#define BZ_DEV inline
#define BZ_FOR_T for (int t = 0; t < kThreads; ++t)
#define BZ_SYNC ((void)0)
#define BZ_ATOMIC_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define BZ_ATOMIC_ADD(p, v) (*(p) += (v))
#define BZ_ATOMIC_OR(p, v) (*(p) |= (v))
#else
#define BZ_DEV __device__ inline
#define BZ_FOR_T for (int t = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define BZ_SYNC __syncthreads()
#define BZ_ATOMIC_MAX(p, v) ((void)atomicMax((p), (v)))
#define BZ_ATOMIC_ADD(p, v) ((void)atomicAdd((p), (v)))
#define BZ_ATOMIC_OR(p, v) ((void)atomicOr((p), (v)))
#endif

constexpr int kThreads = 256;
constexpr int kPayloadMax = 0xff00;          // bytes of payload per block (bgzf_append)
constexpr int kMemberMax = 65536;            // BSIZE + 1 at most
constexpr int kHashBits = 14;
constexpr int kHashSize = 1 << kHashBits;
constexpr int kMinMatch = 3, kMaxMatch = 258, kMaxDist = 32768;
constexpr int kNiceMatch = 64;             // a match at distance 1 this long is taken as it is
constexpr int kFarDist = 4096;               // a match of 3 bytes further back than this costs more than its literals
constexpr int kLitSyms = 286, kDistSyms = 30, kClSyms = 19;
constexpr int kEob = 256;
constexpr int kTokenBitsMax = 48;            // 15 + 5 + 15 + 13
constexpr int kStageWords = (31 + kThreads * kTokenBitsMax) / 32 + 4;

struct BlockShared {
	uint32_t payload_w[kPayloadMax / 4 + 4];  // the payload's bytes (16 more: match_len reads whole words)
	uint32_t hash[kHashSize];                // position + 1 of the latest (earlier-tile) occurrence of the hash, 0: none
	uint32_t crc_tab[256];
	uint32_t lfreq[kLitSyms + 2], dfreq[kDistSyms + 2], cfreq[kClSyms + 1];
	uint16_t lcode[kLitSyms + 2], dcode[kDistSyms + 2], ccode[kClSyms + 1];      // bit-reversed: ready for the LSB-first stream
	uint8_t llen[kLitSyms + 2], dlen[kDistSyms + 2], clen[kClSyms + 1];
	// the code builder
	uint32_t node_w[2 * kLitSyms];
	uint16_t node_parent[2 * kLitSyms], sorted[kLitSyms + 2];
	uint8_t node_depth[2 * kLitSyms];
	uint32_t len_count[16], next_code[16];   // (in LDS, not in registers: they are indexed by a length)
	// a tile
	uint16_t t_len[kThreads], t_dist[kThreads], jmp[2][kThreads];
	uint8_t mark[kThreads], t_nb[kThreads];
	uint32_t scan[2][kThreads];
	uint64_t t_bits[kThreads];
	uint32_t stage[kStageWords];             // the tile's bits, word 0 begins with the bits carried over
	uint32_t part[kThreads];
	uint32_t cursor[2];                      // first position of the tile (relative) that begins a token; alternates with the tile's parity
	uint32_t bitpos, carry, hlit, hdist, crc, stored, member_bytes;
};

BZ_DEV uint32_t hash3(const uint8_t *p)
{
	const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
	return (v * 0x9E3779B1u) >> (32 - kHashBits);
}

// eight bytes of the payload from byte `at` on, out of three aligned words
BZ_DEV uint64_t load8(const uint32_t *w, int at)
{
	const int i = at >> 2, s = (at & 3) * 8;
	const uint64_t lo = (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
	return s ? (lo >> s) | ((uint64_t)w[i + 2] << (64 - s)) : lo;
}

// bytes that payload[a ..] and payload[b ..] share, max_len at most: eight per step (a step is one round trip to LDS, and a wave waits for its
// longest lane: byte by byte, a lane inside a run kept its wave for 258 of them)
BZ_DEV int match_len(const uint32_t *w, int a, int b, int max_len)
{
	int l = 0;
	while (l < max_len) {
		const uint64_t x = load8(w, a + l) ^ load8(w, b + l);
		if (x) { l += __builtin_ctzll(x) >> 3; break; }
		l += 8;
	}
	return l < max_len ? l : max_len;
}

BZ_DEV int ilog2(uint32_t v) { return 31 - __builtin_clz(v); }

// RFC 1951 3.2.5: the length code (0 .. 28, symbol 257 + code), its extra bits and their value
BZ_DEV void len_code(int len, int &code, int &nb, int &extra)
{
	const int l = len - kMinMatch;
	if (len == kMaxMatch) { code = 28; nb = 0; extra = 0; return; }
	if (l < 8) { code = l; nb = 0; extra = 0; return; }
	nb = ilog2((uint32_t)l) - 2;
	code = 4 * nb + 4 + ((l >> nb) & 3);
	extra = l & ((1 << nb) - 1);
}
BZ_DEV void dist_code(int dist, int &code, int &nb, int &extra)
{
	const int d = dist - 1;
	if (d < 4) { code = d; nb = 0; extra = 0; return; }
	nb = ilog2((uint32_t)d) - 1;
	code = 2 * nb + 2 + ((d >> nb) & 1);
	extra = d & ((1 << nb) - 1);
}
// RFC 1951 3.2.7: the order in which the code-length code's lengths are sent -- 16, 17, 18, 0, then 8, 7, 9, 6, 10, 5, ... 1, 15
BZ_DEV int cl_order(int i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2; }
BZ_DEV int len_extra_bits(int code) { return code < 8 || code == 28 ? 0 : (code - 4) / 4; }
BZ_DEV int dist_extra_bits(int code) { return code < 4 ? 0 : (code - 2) / 2; }

// ---- CRC-32 (the gzip polynomial, reflected) ----------------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xedb88320u;

// a(x) * b(x) mod P in the reflected representation (x^0 is bit 31)
BZ_DEV uint32_t crc_mul(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 0x80000000u; m != 0; m >>= 1) {
		if (a & m) p ^= b;
		b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
	}
	return p;
}
// x^(8 k) mod P: what k further bytes do to the CRC of the bytes in front of them (the identity pgzip.inc's combine rests on)
BZ_DEV uint32_t crc_xpow8(uint32_t k)
{
	uint32_t r = 0x80000000u, base = 0x00800000u;
	for (; k; k >>= 1) {
		if (k & 1) r = crc_mul(r, base);
		base = crc_mul(base, base);
	}
	return r;
}

// CRC-32 of payload[0, n) into sh.crc: every thread its own slice, advanced over the bytes behind it, all of them XORed
BZ_DEV void block_crc(BlockShared &sh, int n)
{
	const uint8_t *payload = (const uint8_t *)sh.payload_w;
	BZ_FOR_T {
		uint32_t c = (uint32_t)t;
		for (int i = 0; i < 8; ++i) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
		sh.crc_tab[t] = c;
	}
	BZ_SYNC;
	BZ_FOR_T {
		const int slice = (n + kThreads - 1) / kThreads;
		const int from = t * slice < n ? t * slice : n, to = from + slice < n ? from + slice : n;
		uint32_t c = 0;
		if (from < to) {
			c = 0xffffffffu;
			for (int i = from; i < to; ++i) c = sh.crc_tab[(c ^ payload[i]) & 255] ^ (c >> 8);
			c = crc_mul(crc_xpow8((uint32_t)(n - to)), c ^ 0xffffffffu);
		}
		sh.part[t] = c;
	}
	BZ_SYNC;
	BZ_FOR_T {
		if (t != 0) continue;
		uint32_t c = 0;
		for (int i = 0; i < kThreads; ++i) c ^= sh.part[i];
		sh.crc = c;
	}
	BZ_SYNC;
}

// ---- code lengths and codes ----------------------------------------------------------------------------------------------------
// Huffman lengths of the n symbols counted in freq[], none above max_bits, and their canonical codes (RFC 1951 3.2.2), bit-reversed.
// Fewer than two symbols in use: two codes of one bit, as zlib does, so that the tree is complete whatever the block holds --
// no match at all leaves the distance tree with the codes of distances 1 and 2, a single distance in use keeps its 1-bit code.
BZ_DEV void huff_build(BlockShared &sh, const uint32_t *freq, int n, int max_bits, uint8_t *lens, uint16_t *codes)
{
	// symbols in use, ascending by (count, symbol): every symbol counts those in front of it
	BZ_FOR_T {
		for (int s = t; s < n; s += kThreads) {
			lens[s] = 0; codes[s] = 0;
			const uint32_t f = freq[s];
			if (f == 0) continue;
			int rank = 0;
			for (int o = 0; o < n; ++o) {
				const uint32_t g = freq[o];
				rank += (g != 0 && (g < f || (g == f && o < s))) ? 1 : 0;
			}
			sh.sorted[rank] = (uint16_t)s;
		}
	}
	BZ_SYNC;
	BZ_FOR_T {
		if (t != 0) continue;
		int m = 0;
		for (int s = 0; s < n; ++s) m += freq[s] != 0 ? 1 : 0;
		if (m < 2) {
			const int used = m == 1 ? (int)sh.sorted[0] : 0;
			lens[used] = 1;
			lens[used == 0 ? 1 : 0] = 1;
		} else {
			// the tree: leaves 0 .. m-1 in ascending order, inner nodes m .. 2m-2 come into being in ascending order too (two queues)
			for (int i = 0; i < m; ++i) sh.node_w[i] = freq[sh.sorted[i]];
			int leaf = 0, inner = m;
			for (int next = m; next < 2 * m - 1; ++next) {
				int pick[2];
				for (int k = 0; k < 2; ++k) {
					if (leaf < m && (inner >= next || sh.node_w[leaf] <= sh.node_w[inner])) pick[k] = leaf++;
					else pick[k] = inner++;
				}
				sh.node_w[next] = sh.node_w[pick[0]] + sh.node_w[pick[1]];
				sh.node_parent[pick[0]] = sh.node_parent[pick[1]] = (uint16_t)next;
			}
			sh.node_depth[2 * m - 2] = 0;
			for (int i = 2 * m - 3; i >= 0; --i) sh.node_depth[i] = (uint8_t)(sh.node_depth[sh.node_parent[i]] + 1);      // (a depth of d needs a count of F(d): far below 256 for 0xff00 bytes)
			// lengths above the limit are folded into it; the Kraft sum is brought back to one by lengthening one of the shortest codes that can
			// be lengthened for every unit too much; the lengths then go to the symbols by rank: the rarest get the longest
			uint32_t *count = sh.len_count;
			for (int l = 0; l < 16; ++l) count[l] = 0;
			for (int i = 0; i < m; ++i) count[sh.node_depth[i] < max_bits ? sh.node_depth[i] : max_bits]++;
			uint32_t total = 0;
			for (int l = 1; l <= max_bits; ++l) total += count[l] << (max_bits - l);
			while (total != (1u << max_bits)) {
				count[max_bits]--;
				for (int l = max_bits - 1; l > 0; --l)
					if (count[l]) { count[l]--; count[l + 1] += 2; break; }
				total--;
			}
			int at = 0;
			for (int l = max_bits; l >= 1; --l)
				for (uint32_t c = 0; c < count[l]; ++c) lens[sh.sorted[at++]] = (uint8_t)l;
		}
		uint32_t *count = sh.len_count, *next_code = sh.next_code;
		for (int l = 0; l < 16; ++l) count[l] = 0;
		for (int s = 0; s < n; ++s) count[lens[s]]++;
		count[0] = 0;
		uint32_t code = 0;
		for (int l = 1; l <= max_bits; ++l) { code = (code + count[l - 1]) << 1; next_code[l] = code; }
		for (int s = 0; s < n; ++s) {
			const int l = lens[s];
			if (!l) continue;
			uint32_t c = next_code[l]++, r = 0;
			for (int i = 0; i < l; ++i) { r = (r << 1) | (c & 1); c >>= 1; }
			codes[s] = (uint16_t)r;
		}
	}
	BZ_SYNC;
}

// ---- the tiles -----------------------------------------------------------------------------------------------------------------
// thread 0's writer of the dynamic block's header: whole words straight into the member
struct BitWriter {
	uint32_t *out;
	uint64_t acc;
	int n_acc;
	uint32_t word;
};
BZ_DEV void put_bits(BitWriter &w, uint32_t v, int n)
{
	w.acc |= (uint64_t)v << w.n_acc;
	w.n_acc += n;
	if (w.n_acc >= 32) { w.out[w.word++] = (uint32_t)w.acc; w.acc >>= 32; w.n_acc -= 32; }
}

// One walk over the payload's tiles.  kEmit false: the tokens' symbols are counted (pass 1); true: their bits go behind sh.bitpos (pass 2).
template <bool kEmit> BZ_DEV void walk_tiles(BlockShared &sh, int n, uint32_t *out_words)
{
	const uint8_t *payload = (const uint8_t *)sh.payload_w;
	BZ_FOR_T {
		for (int i = t; i < kHashSize; i += kThreads) sh.hash[i] = 0;
		if (kEmit)
			for (int i = 1 + t; i < kStageWords; i += kThreads) sh.stage[i] = 0;
		if (t == 0) sh.cursor[0] = 0;
	}
	BZ_SYNC;
	int tile = 0;
	for (int base = 0; base < n; base += kThreads, ++tile) {
		const int par = tile & 1;
		// match
		BZ_FOR_T {
			const int p = base + t;
			int len = 0, dist = 0;
			const int max_len = n - p < kMaxMatch ? n - p : kMaxMatch;
			if (max_len >= kMinMatch) {
				// distance 1 first: inside a run that is the match, and one of kNiceMatch bytes is taken without a look at the table
				if (p >= 1) {
					const int l = match_len(sh.payload_w, p - 1, p, max_len);
					if (l >= kMinMatch) { len = l; dist = 1; }
				}
				const uint32_t c = len < kNiceMatch && len < max_len ? sh.hash[hash3(payload + p)] : 0u;
				if (c != 0 && p - (int)(c - 1) <= kMaxDist) {
					// (the table's match has to be longer: at equal length distance 1 is the cheaper one, and a run then uses a single distance code)
					const int cand = (int)(c - 1), l = match_len(sh.payload_w, cand, p, max_len);
					if (l > len && (l > kMinMatch || (l == kMinMatch && p - cand <= kFarDist))) { len = l; dist = p - cand; }
				}
			}
			sh.t_len[t] = (uint16_t)len; sh.t_dist[t] = (uint16_t)dist;
			sh.jmp[0][t] = (uint16_t)(t + (len ? len : 1));
			sh.mark[t] = (uint32_t)t == sh.cursor[par] ? 1 : 0;
		}
		BZ_SYNC;
		// parse: after step k the marked positions are the first 2^(k+1) of the chain that starts at the cursor, jmp is the chain's 2^(k+1)-th power
		for (int k = 0; k < 8; ++k) {
			BZ_FOR_T {
				const int j = sh.jmp[k & 1][t];
				if (sh.mark[t] && j < kThreads) sh.mark[j] = 1;
				sh.jmp[(k & 1) ^ 1][t] = j < kThreads ? sh.jmp[k & 1][j] : (uint16_t)j;
			}
			BZ_SYNC;
		}
		// insert, and the tokens
		BZ_FOR_T {
			const int p = base + t;
			if (p + kMinMatch <= n) BZ_ATOMIC_MAX(&sh.hash[hash3(payload + p)], (uint32_t)(p + 1));
			const uint32_t cur = sh.cursor[par];
			if (t == 0 && cur >= (uint32_t)kThreads) sh.cursor[par ^ 1] = cur - kThreads;      // (the whole tile lies inside a match)
			uint64_t bits = 0;
			int nb = 0;
			if (sh.mark[t]) {
				const int len = sh.t_len[t], adv = len ? len : 1;
				if (t + adv >= kThreads) sh.cursor[par ^ 1] = (uint32_t)(t + adv - kThreads);   // (the tile's last token: one writer)
				if (p < n) {
					if (!len) {
						const int b = payload[p];
						if (kEmit) { bits = sh.lcode[b]; nb = sh.llen[b]; }
						else BZ_ATOMIC_ADD(&sh.lfreq[b], 1u);
					} else {
						int lc, lnb, lex, dc, dnb, dex;
						len_code(len, lc, lnb, lex);
						dist_code(sh.t_dist[t], dc, dnb, dex);
						if (kEmit) {
							bits = sh.lcode[257 + lc]; nb = sh.llen[257 + lc];
							bits |= (uint64_t)lex << nb; nb += lnb;
							bits |= (uint64_t)sh.dcode[dc] << nb; nb += sh.dlen[dc];
							bits |= (uint64_t)dex << nb; nb += dnb;
						} else {
							BZ_ATOMIC_ADD(&sh.lfreq[257 + lc], 1u);
							BZ_ATOMIC_ADD(&sh.dfreq[dc], 1u);
						}
					}
				}
			}
			if (kEmit) { sh.t_bits[t] = bits; sh.t_nb[t] = (uint8_t)nb; sh.scan[0][t] = (uint32_t)nb; }
		}
		BZ_SYNC;
		if (!kEmit) continue;
		// where every token's bits go: the inclusive scan of their counts ends in scan[0]
		for (int k = 0; k < 8; ++k) {
			BZ_FOR_T {
				uint32_t v = sh.scan[k & 1][t];
				if (t >= (1 << k)) v += sh.scan[k & 1][t - (1 << k)];
				sh.scan[(k & 1) ^ 1][t] = v;
			}
			BZ_SYNC;
		}
		BZ_FOR_T {
			const int nb = sh.t_nb[t];
			if (!nb) continue;
			const uint32_t rel = (sh.bitpos & 31) + sh.scan[0][t] - (uint32_t)nb, w = rel >> 5, s = rel & 31;
			const uint64_t v = sh.t_bits[t];
			BZ_ATOMIC_OR(&sh.stage[w], (uint32_t)(v << s));
			const uint32_t mid = (uint32_t)(v >> (32 - s)), high = s ? (uint32_t)(v >> (64 - s)) : 0u;
			if (mid) BZ_ATOMIC_OR(&sh.stage[w + 1], mid);
			if (high) BZ_ATOMIC_OR(&sh.stage[w + 2], high);
		}
		BZ_SYNC;
		// the whole words leave, the rest is carried
		BZ_FOR_T {
			const uint32_t full = ((sh.bitpos & 31) + sh.scan[0][kThreads - 1]) >> 5, word0 = sh.bitpos >> 5;
			for (uint32_t w = (uint32_t)t; w < full; w += kThreads)
				if (word0 + w < kMemberMax / 4) out_words[word0 + w] = sh.stage[w];      // (a member never gets there: it is smaller than the stored one)
			if (t == 0) sh.carry = sh.stage[full];
		}
		BZ_SYNC;
		BZ_FOR_T {
			for (int w = t; w < kStageWords; w += kThreads) sh.stage[w] = w == 0 ? sh.carry : 0u;
			if (t == 0) sh.bitpos += sh.scan[0][kThreads - 1];
		}
		BZ_SYNC;
	}
}

// src[0, n) -> one BGZF member at out (4-byte aligned, kMemberMax bytes of room); returns its size in every thread (0: n is not 1 .. 0xff00, or
// the member did not come out at the size computed for it -- *errors counts those)
BZ_DEV int deflate_block(BlockShared &sh, const uint8_t *src, int n, uint32_t *out_words, unsigned long long *errors)
{
	if (n <= 0 || n > kPayloadMax) return 0;
	uint8_t *out = (uint8_t *)out_words;
	uint8_t *payload = (uint8_t *)sh.payload_w;
	BZ_FOR_T {
		for (int i = t; i < n; i += kThreads) payload[i] = src[i];
		for (int i = t; i < kLitSyms + 2; i += kThreads) sh.lfreq[i] = i == kEob ? 1u : 0u;
		if (t < kDistSyms + 2) sh.dfreq[t] = 0;
		if (t < kClSyms + 1) sh.cfreq[t] = 0;
		if (t < 16) payload[n + t] = 0;
	}
	BZ_SYNC;
	block_crc(sh, n);
	walk_tiles<false>(sh, n, out_words);
	huff_build(sh, sh.lfreq, kLitSyms, 15, sh.llen, sh.lcode);
	huff_build(sh, sh.dfreq, kDistSyms, 15, sh.dlen, sh.dcode);
	BZ_FOR_T {
		if (t != 0) continue;
		int hlit = 257, hdist = 1;
		for (int s = 257; s < kLitSyms; ++s) if (sh.llen[s]) hlit = s + 1;
		for (int s = 1; s < kDistSyms; ++s) if (sh.dlen[s]) hdist = s + 1;
		sh.hlit = (uint32_t)hlit; sh.hdist = (uint32_t)hdist;
		// (the lengths go out one by one, without the repeat symbols 16 / 17 / 18)
		for (int s = 0; s < hlit; ++s) sh.cfreq[sh.llen[s]]++;
		for (int s = 0; s < hdist; ++s) sh.cfreq[sh.dlen[s]]++;
	}
	BZ_SYNC;
	huff_build(sh, sh.cfreq, kClSyms, 7, sh.clen, sh.ccode);
	// the size of the dynamic block, to the bit; stored instead where that is not smaller (RFC 1951 3.2.4: 3 bits, padding, LEN, NLEN)
	BZ_FOR_T {
		if (t != 0) continue;
		uint64_t bits = 3 + 5 + 5 + 4 + 3 * kClSyms;
		for (int s = 0; s < kClSyms; ++s) bits += (uint64_t)sh.cfreq[s] * sh.clen[s];
		for (int s = 0; s < kLitSyms; ++s) bits += (uint64_t)sh.lfreq[s] * (sh.llen[s] + (s > 256 ? len_extra_bits(s - 257) : 0));
		for (int s = 0; s < kDistSyms; ++s) bits += (uint64_t)sh.dfreq[s] * (sh.dlen[s] + dist_extra_bits(s));
		const uint64_t bytes = (bits + 7) / 8;
		sh.stored = bytes >= (uint64_t)n + 5 ? 1u : 0u;
		sh.member_bytes = (uint32_t)(18 + (sh.stored ? (uint64_t)n + 5 : bytes) + 8);
		// the member's header: bgzf_append_block's head[] and BSIZE
		out_words[0] = 0x04088b1fu; out_words[1] = 0; out_words[2] = 0x0006ff00u; out_words[3] = 0x00024342u;
		BitWriter w{out_words, 0, 0, 4};
		put_bits(w, sh.member_bytes - 1, 16);
		if (sh.stored) {
			put_bits(w, 1, 8);
			put_bits(w, (uint32_t)n, 16);
			put_bits(w, (uint32_t)n ^ 0xffffu, 16);
			out[20] = (uint8_t)w.acc; out[21] = (uint8_t)(w.acc >> 8); out[22] = (uint8_t)(w.acc >> 16);
		} else {
			put_bits(w, 1, 1); put_bits(w, 2, 2);
			put_bits(w, sh.hlit - 257, 5); put_bits(w, sh.hdist - 1, 5); put_bits(w, kClSyms - 4, 4);
			for (int i = 0; i < kClSyms; ++i) put_bits(w, sh.clen[cl_order(i)], 3);
			for (uint32_t s = 0; s < sh.hlit; ++s) put_bits(w, sh.ccode[sh.llen[s]], sh.clen[sh.llen[s]]);
			for (uint32_t s = 0; s < sh.hdist; ++s) put_bits(w, sh.ccode[sh.dlen[s]], sh.clen[sh.dlen[s]]);
			sh.bitpos = w.word * 32 + (uint32_t)w.n_acc;
			sh.stage[0] = (uint32_t)w.acc;
		}
	}
	BZ_SYNC;
	const bool stored = sh.stored != 0;
	const int member = (int)sh.member_bytes;
	if (stored) {
		BZ_FOR_T {
			for (int i = t; i < n; i += kThreads) out[23 + i] = payload[i];
		}
	} else {
		walk_tiles<true>(sh, n, out_words);
		BZ_FOR_T {
			if (t != 0) continue;
			// the end-of-block symbol behind the bits carried, the last bytes one by one
			const uint32_t used = sh.bitpos & 31;
			const uint64_t acc = (uint64_t)sh.stage[0] | ((uint64_t)sh.lcode[kEob] << used);
			const uint32_t at = (sh.bitpos >> 5) * 4, tail = (used + sh.llen[kEob] + 7) / 8;
			if (at + tail + 8 != (uint32_t)member) { sh.member_bytes = 0; BZ_ATOMIC_ADD(errors, 1ull); continue; }
			for (uint32_t i = 0; i < tail; ++i) out[at + i] = (uint8_t)(acc >> (8 * i));
		}
	}
	BZ_SYNC;
	if (sh.member_bytes == 0) return 0;
	BZ_FOR_T {
		if (t >= 8) continue;
		const uint32_t v = t < 4 ? sh.crc : (uint32_t)n;
		out[member - 8 + t] = (uint8_t)(v >> (8 * (t & 3)));
	}
	BZ_SYNC;
	return member;
}

}  // namespace bgzf
}  // namespace kg
