// libecc_amd/csrc/ecamd_rmd160.h -- RIPEMD-160 (Dobbertin, Bosselaers, Preneel 1996; ISO/IEC 10118-3) per item: the compression
// function with its two lines of 80 steps, the padding, and a one-shot over a message held as little-endian words (the slot format of
// ecamd_hash.hip).  Compiles for the device (ecamd_hash3.hip: one item per lane) and for the host (tests/hash_table_host_shim.cpp).
//
// Written from the algorithm's definition, on 32-bit little-endian words:
//
//   IV        67452301 efcdab89 98badcfe 10325476 c3d2e1f0
//   step j    T = ((A + f(B, C, D) + X[r(j)] + K(j)) <<< s(j)) + E;  A = E, E = D, D = C <<< 10, C = B, B = T
//   f         per group of 16 steps, left line: x ^ y ^ z, (x & y) | (~x & z), (x | ~y) ^ z, (x & z) | (y & ~z), x ^ (y | ~z); the
//             right line takes them in the opposite order
//   K         left 0, 5a827999, 6ed9eba1, 8f1bbcdc, a953fd4e; right 50a28be6, 5c4dd124, 6d703ef3, 7a6d76e9, 0
//   r, s      the word orders and shift counts of the two lines: the tables below
//   combine   h0' = h1 + C + D', h1' = h2 + D + E', h2' = h3 + E + A', h3' = h4 + A + B', h4' = h0 + B + C'
//   padding   0x80, zeros, the bit count little-endian in the last eight octets of the last 64-octet block (as MD4)
//
// All 160 steps are unrolled, so every table entry is a constant and the state and the block stay in registers.
//
// SECRET DATA: none.  What is hashed here is a message; the tables are indexed by the step number only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ERMD_FN __host__ __device__ __forceinline__
#else
#define ERMD_FN inline
#endif

namespace ecrmd {

typedef uint8_t u8;
typedef uint32_t u32;

enum : int { DIGEST_BYTES = 20, BLOCK_BYTES = 64 };

// libecc's hash_alg_type number (RIPEMD160 = 15) -> digest octets, 0: another
ERMD_FN int hash_size(int hash_type) { return hash_type == 15 ? (int)DIGEST_BYTES : 0; }
ERMD_FN int block_size(int hash_type) { return hash_type == 15 ? (int)BLOCK_BYTES : 0; }

ERMD_FN u32 rotl(u32 x, int r) { return (x << r) | (x >> (32 - r)); }

// f of group G (0 .. 4)
template <int G> ERMD_FN u32 f(u32 x, u32 y, u32 z)
{
	return G == 0 ? (x ^ y ^ z) : G == 1 ? ((x & y) | (~x & z)) : G == 2 ? ((x | ~y) ^ z) : G == 3 ? ((x & z) | (y & ~z)) : (x ^ (y | ~z));
}

ERMD_FN void init(u32 *h)
{
	h[0] = 0x67452301u; h[1] = 0xefcdab89u; h[2] = 0x98badcfeu; h[3] = 0x10325476u; h[4] = 0xc3d2e1f0u;
}

// sixteen steps of one line: FG the group of f, K the constant, R / S at 16 * GRP
template <int FG, int GRP, bool RIGHT> ERMD_FN void group(u32 &a, u32 &b, u32 &c, u32 &d, u32 &e, const u32 *x, u32 K)
{
	constexpr int RL[80] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 7, 4, 13, 1, 10, 6, 15, 3, 12, 0, 9, 5, 2, 14, 11, 8,
				3, 10, 14, 4, 9, 15, 8, 1, 2, 7, 0, 6, 13, 11, 5, 12, 1, 9, 11, 10, 0, 8, 12, 4, 13, 3, 7, 15, 14, 5, 6, 2,
				4, 0, 5, 9, 7, 12, 2, 10, 14, 1, 3, 8, 11, 6, 15, 13};
	constexpr int RR[80] = {5, 14, 7, 0, 9, 2, 11, 4, 13, 6, 15, 8, 1, 10, 3, 12, 6, 11, 3, 7, 0, 13, 5, 10, 14, 15, 8, 12, 4, 9, 1, 2,
				15, 5, 1, 3, 7, 14, 6, 9, 11, 8, 12, 2, 10, 0, 4, 13, 8, 6, 4, 1, 3, 11, 15, 0, 5, 12, 2, 13, 9, 7, 10, 14,
				12, 15, 10, 4, 1, 5, 8, 7, 6, 2, 13, 14, 0, 3, 9, 11};
	constexpr int SL[80] = {11, 14, 15, 12, 5, 8, 7, 9, 11, 13, 14, 15, 6, 7, 9, 8, 7, 6, 8, 13, 11, 9, 7, 15, 7, 12, 15, 9, 11, 7, 13, 12,
				11, 13, 6, 7, 14, 9, 13, 15, 14, 8, 13, 6, 5, 12, 7, 5, 11, 12, 14, 15, 14, 15, 9, 8, 9, 14, 5, 6, 8, 6, 5, 12,
				9, 15, 5, 11, 6, 8, 13, 12, 5, 12, 13, 14, 11, 8, 5, 6};
	constexpr int SR[80] = {8, 9, 9, 11, 13, 15, 15, 5, 7, 7, 8, 11, 14, 14, 12, 6, 9, 13, 15, 7, 12, 8, 9, 11, 7, 7, 12, 7, 6, 15, 13, 11,
				9, 7, 15, 11, 8, 6, 6, 14, 12, 13, 5, 14, 13, 13, 7, 5, 15, 5, 8, 11, 14, 14, 6, 14, 6, 9, 12, 9, 12, 5, 15, 8,
				8, 5, 12, 9, 12, 5, 14, 6, 8, 13, 6, 5, 15, 13, 11, 11};
#pragma unroll
	for (int j = 16 * GRP; j < 16 * GRP + 16; j++) {
		const u32 t = rotl(a + f<FG>(b, c, d) + x[RIGHT ? RR[j] : RL[j]] + K, RIGHT ? SR[j] : SL[j]) + e;
		a = e; e = d; d = rotl(c, 10); c = b; b = t;
	}
}

// one compression: h <- CF(h, x), x the block as 16 little-endian words
ERMD_FN void compress(u32 *h, const u32 *x)
{
	u32 al = h[0], bl = h[1], cl = h[2], dl = h[3], el = h[4];
	u32 ar = h[0], br = h[1], cr = h[2], dr = h[3], er = h[4];
	group<0, 0, false>(al, bl, cl, dl, el, x, 0x00000000u);
	group<4, 0, true>(ar, br, cr, dr, er, x, 0x50a28be6u);
	group<1, 1, false>(al, bl, cl, dl, el, x, 0x5a827999u);
	group<3, 1, true>(ar, br, cr, dr, er, x, 0x5c4dd124u);
	group<2, 2, false>(al, bl, cl, dl, el, x, 0x6ed9eba1u);
	group<2, 2, true>(ar, br, cr, dr, er, x, 0x6d703ef3u);
	group<3, 3, false>(al, bl, cl, dl, el, x, 0x8f1bbcdcu);
	group<1, 3, true>(ar, br, cr, dr, er, x, 0x7a6d76e9u);
	group<4, 4, false>(al, bl, cl, dl, el, x, 0xa953fd4eu);
	group<0, 4, true>(ar, br, cr, dr, er, x, 0x00000000u);
	const u32 t = h[1] + cl + dr;
	h[1] = h[2] + dl + er;
	h[2] = h[3] + el + ar;
	h[3] = h[4] + al + br;
	h[4] = h[0] + bl + cr;
	h[0] = t;
}

// little-endian word j of the padded message (msg: the message as little-endian words, readable up to the word that holds the last
// octet); len_word: the index of the word that takes the bit count
ERMD_FN u32 padded_word(const u32 *msg, u32 len, u32 j, u32 len_word)
{
	const u32 pos = 4u * j;
	if (j == len_word) {
		return len << 3;   // (inputs are far below 2^29 octets: the count fits one word, the word after it is zero)
	}
	if (pos > len) {
		return 0u;
	}
	if (pos == len) {
		return 0x80u;
	}
	const u32 w = msg[j], rem = len - pos;
	return rem >= 4u ? w : ((w & (0xffffffffu >> (8u * (4u - rem)))) | (0x80u << (8u * rem)));
}

// RIPEMD-160 of len octets (len < 2^29) held as words; h: the five words of the digest
ERMD_FN void hash_words(const u32 *msg, u32 len, u32 *h)
{
	init(h);
	const u32 nblocks = (len + 9u + 63u) / 64u, len_word = 16u * nblocks - 2u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < nblocks; b++) {
		u32 x[16];
#pragma unroll
		for (u32 t = 0; t < 16; t++) {
			x[t] = padded_word(msg, len, 16u * b + t, len_word);
		}
		compress(h, x);
	}
}

// the digest's words as its 20 octets, little-endian
ERMD_FN void digest_bytes(const u32 *h, u8 *out)
{
#pragma unroll
	for (int k = 0; k < 20; k++) {
		out[k] = (u8)(h[k >> 2] >> (8 * (k & 3)));
	}
}

// one slot (a little-endian u32 length, then the octets; stride a multiple of 4) -> 20 octets at out; a length that does not fit the
// slot gives zeros
ERMD_FN void slot_digest(const u8 *slot, u32 stride, u8 *out)
{
	const u32 *words = (const u32 *)slot;
	const u32 len = words[0];
	u32 h[5];
	if (len > stride - 4u) {
#pragma unroll
		for (int k = 0; k < 5; k++) {
			h[k] = 0;
		}
	} else {
		hash_words(words + 1, len, h);
	}
	digest_bytes(h, out);
}

}  // namespace ecrmd
