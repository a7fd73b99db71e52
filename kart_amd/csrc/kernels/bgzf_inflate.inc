// kernels/bgzf_inflate.inc -- one BGZF member (a gzip member of at most 64 KiB, RFC 1951 / 1952) inflated by one wave of 64 lanes: the
// mirror of bgzf_block.inc, behind which it is included (it uses that file's CRC arithmetic and RFC tables).
//
// Lane 0 reads the bits: a block's header, its code lengths, then the symbols, a BATCH of kQueue tokens (a literal, or length + distance,
// with the place in the text it goes to) at a time.  All lanes then expand the batch straight into the destination: the literals first,
// then the matches, each copied by the whole wave from the text behind it (source index `from + k % dist`, so that a match may overlap
// itself).  Matches that read nothing a match of the same GROUP wrote are copied without a barrier between them; lane 0 marks the
// match in front of which the text has to be complete.  The code tables (a 10-bit and a 9-bit lookup table, the canonical walk of
// RFC 1951 3.2.2 for longer codes) and the queue lie in LDS, ~8 KiB per wave.
//
// The input is a file's bytes and is trusted in nothing:
//   reads    the bit reader never reads outside the deflate stream's bytes; behind their end it yields zeros, and the position it
//            reports then lies behind the end, which every loop that reads bits checks
//   writes   a token is queued only where it ends inside the member's own piece of the text
//   loops    every loop consumes at least one bit or produces at least one byte (or one code length) and ends at their bounds
//   tables   a set of code lengths is refused where zlib refuses it (over-subscribed; incomplete, save a single code of one bit)
//            before a table is made of it; codes the set leaves unused decode to an error
// What is accepted and what is refused is what zlib accepts and refuses (inflate() with a 32 KiB window, then gzip's CRC-32 / ISIZE).
//
// Phases as in bgzf_block.inc: `IZ_FOR_L { ... }` is what lane l does between two barriers, IZ_SYNC the barrier (a workgroup is ONE
// wave, so that the barrier costs a fence); code between the phases is the same in every lane.  With BGZF_HOST_EMULATION the same text
// runs lane after lane in a host program (tests/bgzf_inflate_host.cpp).

namespace kg {
namespace bgzf {

#if defined(BGZF_HOST_EMULATION)
#define IZ_FOR_L for (int l = 0; l < kWave; ++l)
#define IZ_SYNC ((void)0)
#else
#define IZ_FOR_L for (int l = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define IZ_SYNC __syncthreads()
#endif

constexpr int kWave = 64;
constexpr int kLitBits = 10, kDistBits = 9;  // bits the lookup tables are indexed by
constexpr int kQueue = 128;                  // tokens of a batch
constexpr int kLitMax = 288, kDistMax = 32;  // symbols of the fixed codes (286 / 287 and 30 / 31 have codes and no meaning)
constexpr int kGzHead = 12, kGzTail = 8;     // bytes of a gzip member in front of its extra field, behind its deflate stream
constexpr uint16_t kTokSync = 0x8000;        // Token::len: the text has to be complete in front of this match

// = KG_INFLATE_* (include/kart_amd.h)
enum { kInflateOk = 0, kInflateHeader = 1, kInflateStream = 2, kInflateSize = 3, kInflateCrc = 4 };
enum { kStBlock = 0, kStStored, kStBuild, kStDecode, kStFinish, kStDone };

struct Token {
	uint32_t out;       // where in the member's text
	uint16_t len;       // 0: a literal; else 3 .. 258 (| kTokSync)
	uint16_t val;       // the literal, or the distance - 1
};

struct InflateShared {
	uint16_t llut[1 << kLitBits], dlut[1 << kDistBits];      // symbol << 4 | code length; 0: no code this short begins with these bits
	uint8_t lens[kLitMax + kDistMax];                        // the literal/length code's lengths, the distance code's behind them
	uint8_t cllen[20];
	uint16_t lcode[kLitMax], dcode[kDistMax];                // bit-reversed codes
	uint16_t lsorted[kLitMax], dsorted[kDistMax];            // symbols by (length, symbol): the canonical walk
	uint16_t lcount[16], dcount[16];                         // codes of every length
	uint16_t offs[16], next_code[16];                        // (in LDS, not in registers: they are indexed by a length)
	uint32_t crc_tab[256];
	uint32_t part[kWave];
	Token q[kQueue];
	uint32_t bitpos;                                         // bits of the deflate stream consumed
	uint32_t out;                                            // bytes of text decoded (queued)
	uint32_t nq, state, status, last_block, nlit, ndist, stored_from, stored_len, crc_want;
};

// four bytes of s[0, n) from `byte` on, zeros behind the end
BZ_DEV uint32_t iz_word(const uint8_t *s, uint32_t n, uint32_t byte)
{
	uint32_t v = 0;
	if (byte + 4 <= n) {
		v = (uint32_t)s[byte] | ((uint32_t)s[byte + 1] << 8) | ((uint32_t)s[byte + 2] << 16) | ((uint32_t)s[byte + 3] << 24);
	} else {
		for (uint32_t i = 0; i < 4; ++i)
			if (byte + i < n) v |= (uint32_t)s[byte + i] << (8 * i);
	}
	return v;
}

// lane 0's reader of the stream s[0, n): 33 bits or more in `buf` after a refill(), the word behind them already on its way
struct BitReader {
	const uint8_t *s;
	uint32_t n;
	uint64_t buf;
	int nb;
	uint32_t ahead, ahead_byte;     // the word at ahead_byte: loaded, not yet in buf
};
BZ_DEV void br_open(BitReader &r, const uint8_t *s, uint32_t n, uint32_t bitpos)
{
	const uint32_t byte = bitpos >> 3, sh = bitpos & 7;
	r.s = s; r.n = n;
	r.buf = ((uint64_t)iz_word(s, n, byte) | ((uint64_t)iz_word(s, n, byte + 4) << 32)) >> sh;
	r.nb = 64 - (int)sh;
	r.ahead_byte = byte + 8;
	r.ahead = iz_word(s, n, r.ahead_byte);
}
BZ_DEV void br_refill(BitReader &r)
{
	if (r.nb > 32) return;
	r.buf |= (uint64_t)r.ahead << r.nb;
	r.nb += 32;
	r.ahead_byte += 4;
	r.ahead = iz_word(r.s, r.n, r.ahead_byte);
}
BZ_DEV uint32_t br_take(BitReader &r, int n)
{
	const uint32_t v = (uint32_t)r.buf & ((1u << n) - 1);
	r.buf >>= n; r.nb -= n;
	return v;
}
BZ_DEV uint32_t br_pos(const BitReader &r) { return 8 * r.ahead_byte - (uint32_t)r.nb; }

// The canonical code of lens[0, n) (RFC 1951 3.2.2): codes per length, the symbols in code order, every symbol's code bit-reversed.
// 0: a code zlib takes (complete, or -- single_ok -- one code of one bit); 1: no symbol has a code; -1: over-subscribed or incomplete
BZ_DEV int canon_build(InflateShared &sh, const uint8_t *lens, int n, bool single_ok, uint16_t *count, uint16_t *sorted, uint16_t *code)
{
	for (int i = 0; i < 16; ++i) count[i] = 0;
	for (int s = 0; s < n; ++s) count[lens[s] & 15]++;
	if (count[0] == n) return 1;
	int left = 1, max = 0;
	for (int i = 1; i < 16; ++i) {
		left = 2 * left - (int)count[i];
		if (left < 0) return -1;
		if (count[i]) max = i;
	}
	if (left > 0 && !(single_ok && max == 1)) return -1;
	uint32_t c = 0;
	sh.offs[1] = 0;
	for (int i = 1; i < 16; ++i) {
		c = (c + (i > 1 ? count[i - 1] : 0)) << 1;
		sh.next_code[i] = (uint16_t)c;
		if (i < 15) sh.offs[i + 1] = (uint16_t)(sh.offs[i] + count[i]);
	}
	for (int s = 0; s < n; ++s) {
		const int len = lens[s] & 15;
		if (!len) continue;
		sorted[sh.offs[len]++] = (uint16_t)s;
		uint32_t v = sh.next_code[len]++, rev = 0;
		for (int i = 0; i < len; ++i) { rev = (rev << 1) | (v & 1); v >>= 1; }
		code[s] = (uint16_t)rev;
	}
	return 0;
}

// the symbol the bits of `buf` begin with, bit by bit along the canonical code; -1: none (a code the set left unused)
BZ_DEV int canon_walk(uint64_t buf, const uint16_t *count, const uint16_t *sorted, int &used)
{
	int code = 0, first = 0, index = 0;
	for (int len = 1; len < 16; ++len) {
		code |= (int)(buf & 1);
		buf >>= 1;
		const int c = count[len];
		if (code - c < first) { used = len; return sorted[index + (code - first)]; }
		index += c; first += c;
		first <<= 1; code <<= 1;
	}
	used = 15;
	return -1;
}

// a symbol through the lookup table, along the canonical code where the table has none
BZ_DEV int iz_symbol(BitReader &r, const uint16_t *lut, int lut_bits, const uint16_t *count, const uint16_t *sorted)
{
	const uint32_t e = lut[(uint32_t)r.buf & ((1u << lut_bits) - 1)];
	if (e) { br_take(r, (int)(e & 15)); return (int)(e >> 4); }
	int used = 0;
	const int s = canon_walk(r.buf, count, sorted, used);
	br_take(r, used);
	return s;
}

BZ_DEV void iz_lut_fill(uint16_t *lut, int lut_bits, int s, int len, uint32_t code)
{
	if (len == 0 || len > lut_bits) return;
	for (uint32_t i = code; i < (1u << lut_bits); i += 1u << len) lut[i] = (uint16_t)((s << 4) | len);
}

BZ_DEV int len_base(int code) { return code == 28 ? 258 : code < 8 ? 3 + code : 3 + ((4 + (code & 3)) << len_extra_bits(code)); }
BZ_DEV int dist_base(int code) { return code < 4 ? 1 + code : 1 + ((2 + (code & 1)) << dist_extra_bits(code)); }

// lane 0: the header of the next deflate block at sh.bitpos; leaves the next state, or the status of an error
BZ_DEV void iz_block_header(InflateShared &sh, const uint8_t *s, uint32_t n, uint32_t cap)
{
	BitReader r;
	br_open(r, s, n, sh.bitpos);
	sh.last_block = br_take(r, 1);
	const uint32_t type = br_take(r, 2);
	sh.state = kStDone; sh.status = kInflateStream;
	if (type == 0) {
		const uint32_t at = (br_pos(r) + 7) >> 3;
		if (at + 4 > n) return;
		const uint32_t len = (uint32_t)s[at] | ((uint32_t)s[at + 1] << 8), nlen = (uint32_t)s[at + 2] | ((uint32_t)s[at + 3] << 8);
		if (len != (nlen ^ 0xffffu) || at + 4 + len > n) return;
		if (sh.out + len > cap) { sh.status = kInflateSize; return; }
		sh.stored_from = at + 4; sh.stored_len = len;
		sh.state = kStStored; sh.status = kInflateOk;
		return;
	}
	if (type == 3) return;
	if (type == 1) {
		for (int i = 0; i < kLitMax; ++i) sh.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
		for (int i = 0; i < kDistMax; ++i) sh.lens[kLitMax + i] = 5;
		sh.nlit = kLitMax; sh.ndist = kDistMax;
	} else {
		const uint32_t nlit = br_take(r, 5) + 257, ndist = br_take(r, 5) + 1, ncl = br_take(r, 4) + 4;
		if (nlit > 286 || ndist > 30) return;
		for (int i = 0; i < 20; ++i) sh.cllen[i] = 0;
		for (uint32_t i = 0; i < ncl; ++i) { br_refill(r); sh.cllen[cl_order((int)i)] = (uint8_t)br_take(r, 3); }
		// (the code-length code borrows the distance code's arrays: that one is built after it)
		if (canon_build(sh, sh.cllen, kClSyms, false, sh.dcount, sh.dsorted, sh.dcode) != 0) return;
		const uint32_t total = nlit + ndist;
		for (uint32_t have = 0; have < total;) {
			br_refill(r);
			int used = 0;
			const int sym = canon_walk(r.buf, sh.dcount, sh.dsorted, used);
			if (sym < 0) return;
			br_take(r, used);
			if (sym < 16) sh.lens[have++] = (uint8_t)sym;
			else {
				uint32_t rep;
				uint8_t v = 0;
				if (sym == 16) {
					if (have == 0) return;
					v = sh.lens[have - 1];
					rep = 3 + br_take(r, 2);
				} else if (sym == 17) rep = 3 + br_take(r, 3);
				else rep = 11 + br_take(r, 7);
				if (have + rep > total) return;
				for (uint32_t i = 0; i < rep; ++i) sh.lens[have++] = v;
			}
			if (br_pos(r) > 8 * n) return;
		}
		if (sh.lens[kEob] == 0) return;
		sh.nlit = nlit; sh.ndist = ndist;
	}
	if (br_pos(r) > 8 * n) return;
	sh.bitpos = br_pos(r);
	sh.state = kStBuild; sh.status = kInflateOk;
}

// lane 0: the next tokens of the block into the queue, until it is full, the block ends or the stream is at fault
BZ_DEV void iz_decode_batch(InflateShared &sh, const uint8_t *s, uint32_t n, uint32_t cap)
{
	BitReader r;
	br_open(r, s, n, sh.bitpos);
	const uint16_t *dlens_count = sh.dcount;
	uint32_t out = sh.out, nq = 0, group = 0xffffffffu;
	uint32_t state = kStDecode, status = kInflateOk;
	while (nq < (uint32_t)kQueue) {
		br_refill(r);
		const int sym = iz_symbol(r, sh.llut, kLitBits, sh.lcount, sh.lsorted);
		if (sym < 0 || sym >= kLitSyms) { state = kStDone; status = kInflateStream; break; }
		if (sym == kEob) { state = sh.last_block ? kStFinish : kStBlock; break; }
		Token t;
		t.out = out;
		if (sym < kEob) {
			if (out + 1 > cap) { state = kStDone; status = kInflateSize; break; }
			t.len = 0; t.val = (uint16_t)sym;
			out += 1;
		} else {
			const int lc = sym - 257;
			const uint32_t len = (uint32_t)len_base(lc) + br_take(r, len_extra_bits(lc));
			br_refill(r);
			const int dc = iz_symbol(r, sh.dlut, kDistBits, dlens_count, sh.dsorted);
			if (dc < 0 || dc >= kDistSyms) { state = kStDone; status = kInflateStream; break; }
			const uint32_t dist = (uint32_t)dist_base(dc) + br_take(r, dist_extra_bits(dc));
			if (dist > out) { state = kStDone; status = kInflateStream; break; }      // in front of the member's first byte
			if (out + len > cap) { state = kStDone; status = kInflateSize; break; }
			// what it reads ends at `from_end`: behind the first byte a match of this group wrote, the group ends in front of it
			const uint32_t from_end = out - dist + (len < dist ? len : dist);
			const bool sync = group == 0xffffffffu || from_end > group;
			if (sync) group = out;
			t.len = (uint16_t)(len | (sync ? kTokSync : 0)); t.val = (uint16_t)(dist - 1);
			out += len;
		}
		if (br_pos(r) > 8 * n) { state = kStDone; status = kInflateStream; break; }
		sh.q[nq++] = t;
	}
	if (br_pos(r) > 8 * n) { state = kStDone; status = kInflateStream; }
	if (state == kStDone) nq = 0;
	else { sh.out = out; sh.bitpos = br_pos(r); }
	sh.nq = nq; sh.state = state; sh.status = status;
}

// One member, m[0, m_bytes), to text[0, cap): its status in every lane.  Nothing outside either range is touched.
BZ_DEV int inflate_member(InflateShared &sh, const uint8_t *m, int m_bytes, uint8_t *text, int cap_)
{
	// the gzip header (RFC 1952): magic, deflate, FEXTRA alone, the extra field's length at offset 10; the trailer: CRC-32, ISIZE
	if (m_bytes < kGzHead + kGzTail || cap_ < 0) return kInflateHeader;
	if (m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || m[3] != 4) return kInflateHeader;
	const int xlen = (int)m[10] | ((int)m[11] << 8);
	if (m_bytes < kGzHead + xlen + kGzTail) return kInflateHeader;
	const uint8_t *s = m + kGzHead + xlen, *tail = m + m_bytes - kGzTail;
	const uint32_t n = (uint32_t)(m_bytes - kGzHead - xlen - kGzTail), cap = (uint32_t)cap_;
	const uint32_t isize = (uint32_t)tail[4] | ((uint32_t)tail[5] << 8) | ((uint32_t)tail[6] << 16) | ((uint32_t)tail[7] << 24);
	if (isize != cap) return kInflateSize;
	IZ_FOR_L {
		for (int i = l; i < 256; i += kWave) {
			uint32_t c = (uint32_t)i;
			for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
			sh.crc_tab[i] = c;
		}
		if (l == 0) {
			sh.bitpos = 0; sh.out = 0; sh.nq = 0; sh.state = kStBlock; sh.status = kInflateOk; sh.last_block = 0;
			sh.crc_want = (uint32_t)tail[0] | ((uint32_t)tail[1] << 8) | ((uint32_t)tail[2] << 16) | ((uint32_t)tail[3] << 24);
		}
	}
	IZ_SYNC;
	// every round consumes bits of the stream (a block's header, tokens) or ends the member
	for (;;) {
		const uint32_t state = sh.state;
		if (state == kStDone) break;
		if (state == kStBlock) {
			IZ_FOR_L {
				if (l == 0) iz_block_header(sh, s, n, cap);
			}
			IZ_SYNC;
		} else if (state == kStStored) {
			const uint32_t from = sh.stored_from, len = sh.stored_len, to = sh.out;
			IZ_FOR_L {
				for (uint32_t i = (uint32_t)l; i < len; i += kWave) text[to + i] = s[from + i];
			}
			IZ_SYNC;
			IZ_FOR_L {
				if (l == 0) {
					sh.out = to + len;
					sh.bitpos = 8 * (from + len);
					sh.state = sh.last_block ? kStFinish : kStBlock;
				}
			}
			IZ_SYNC;
		} else if (state == kStBuild) {
			IZ_FOR_L {
				if (l == 0) {
					// (no literal/length code at all: refused; no distance code at all: a block of literals, a distance symbol in it is at fault)
					const int rl = canon_build(sh, sh.lens, (int)sh.nlit, true, sh.lcount, sh.lsorted, sh.lcode);
					const int rd = rl == 0 ? canon_build(sh, sh.lens + sh.nlit, (int)sh.ndist, true, sh.dcount, sh.dsorted, sh.dcode) : -1;
					if (rl != 0 || rd < 0) { sh.state = kStDone; sh.status = kInflateStream; }
					else sh.state = kStDecode;
				}
				for (int i = l; i < (1 << kLitBits); i += kWave) sh.llut[i] = 0;
				for (int i = l; i < (1 << kDistBits); i += kWave) sh.dlut[i] = 0;
			}
			IZ_SYNC;
			if (sh.state == kStDecode) {
				const int nlit = (int)sh.nlit, ndist = (int)sh.ndist;
				IZ_FOR_L {
					for (int i = l; i < nlit; i += kWave) iz_lut_fill(sh.llut, kLitBits, i, sh.lens[i] & 15, sh.lcode[i]);
					for (int i = l; i < ndist; i += kWave) iz_lut_fill(sh.dlut, kDistBits, i, sh.lens[nlit + i] & 15, sh.dcode[i]);
				}
				IZ_SYNC;
			}
		} else if (state == kStDecode) {
			IZ_FOR_L {
				if (l == 0) iz_decode_batch(sh, s, n, cap);
			}
			IZ_SYNC;
			const int nq = (int)sh.nq;
			IZ_FOR_L {
				for (int i = l; i < nq; i += kWave) {
					const Token t = sh.q[i];
					if (t.len == 0) text[t.out] = (uint8_t)t.val;
				}
			}
			IZ_SYNC;
			// the matches, a group at a time: q[from] begins one, it ends in front of the next match that is marked
			for (int from = 0; from < nq;) {
				int to = from + 1;
				while (to < nq && !(sh.q[to].len & kTokSync)) ++to;
				IZ_FOR_L {
					for (int i = from; i < to; ++i) {
						const Token t = sh.q[i];
						const uint32_t len = t.len & (uint32_t)(kTokSync - 1), dist = (uint32_t)t.val + 1;
						if (len == 0) continue;
						const uint8_t *src = text + t.out - dist;
						for (uint32_t k = (uint32_t)l; k < len; k += kWave) text[t.out + k] = src[k < dist ? k : k % dist];
					}
				}
				IZ_SYNC;
				from = to;
			}
		} else {
			// kStFinish: the stream ended in its last byte, the text is as long as ISIZE says; then its CRC-32 in 64 slices
			const uint32_t produced = sh.out;
			IZ_FOR_L {
				if (l == 0) {
					sh.state = kStDone;
					if (((sh.bitpos + 7) >> 3) != n) sh.status = kInflateStream;
					else if (produced != cap) sh.status = kInflateSize;
				}
			}
			IZ_SYNC;
			if (sh.status != kInflateOk) break;
			IZ_FOR_L {
				const uint32_t slice = (produced + kWave - 1) / kWave;
				const uint32_t a = (uint32_t)l * slice < produced ? (uint32_t)l * slice : produced, b = a + slice < produced ? a + slice : produced;
				uint32_t c = 0;
				if (a < b) {
					c = 0xffffffffu;
					for (uint32_t i = a; i < b; ++i) c = sh.crc_tab[(c ^ text[i]) & 255] ^ (c >> 8);
					c = crc_mul(crc_xpow8(produced - b), c ^ 0xffffffffu);
				}
				sh.part[l] = c;
			}
			IZ_SYNC;
			IZ_FOR_L {
				if (l == 0) {
					uint32_t c = 0;
					for (int i = 0; i < kWave; ++i) c ^= sh.part[i];
					if (c != sh.crc_want) sh.status = kInflateCrc;
				}
			}
			IZ_SYNC;
		}
	}
	const int status = (int)sh.status;
	IZ_SYNC;      // (sh is the next member's from here on)
	return status;
}

}  // namespace bgzf
}  // namespace kg
