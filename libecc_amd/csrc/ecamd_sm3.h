// libecc_amd/csrc/ecamd_sm3.h -- SM3 (GB/T 32905-2016), the hash SM2 is specified with, per item: the compression function, the
// padding, a one-shot over a message held as little-endian words (the slot format of ecamd_hash.hip) and a streamed form (init,
// absorb whole blocks, finish) for inputs that share a prefix (SM2's Z, ecamd_sm2z.h).  Compiles for the device (ecamd_hash2.hip:
// one item per lane) and for the host (ecamd_host_sigfam.cpp: the prefix midstate; tests/sighash2_host_shim.cpp).
//
// Written from the standard's definitions, on 32-bit big-endian words:
//
//   IV           7380166f 4914b2b9 172442d7 da8a0600 a96f30bc 163138aa e38dee4d b0fb0e4e
//   T_j          79cc4519 for rounds 0 .. 15, 7a879d8a for rounds 16 .. 63
//   FF_j, GG_j   x ^ y ^ z for rounds 0 .. 15; the majority / the choice function after
//   P0(x), P1(x) x ^ (x <<< 9) ^ (x <<< 17), x ^ (x <<< 15) ^ (x <<< 23)
//   expansion    W_j = P1(W_(j-16) ^ W_(j-9) ^ (W_(j-3) <<< 15)) ^ (W_(j-13) <<< 7) ^ W_(j-6), W'_j = W_j ^ W_(j+4)
//   round        SS1 = ((A <<< 12) + E + (T_j <<< j)) <<< 7, SS2 = SS1 ^ (A <<< 12), TT1 = FF(A, B, C) + D + SS2 + W'_j,
//                TT2 = GG(E, F, G) + H + SS1 + W_j; D = C, C = B <<< 9, B = A, A = TT1, H = G, G = F <<< 19, F = E, E = P0(TT2)
//   V           <- (A .. H) ^ V after 64 rounds; padding 0x80, zeros, the bit count in the last eight octets (as SHA-256)
//
// The expansion runs in a window of sixteen words, so every index is a constant and the state stays in registers.
//
// SECRET DATA: none.  What is hashed here is a message, an id and public curve and key octets; there is no table at all.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ESM3_FN __host__ __device__ __forceinline__
#else
#define ESM3_FN inline
#endif

namespace ecsm3 {

typedef uint8_t u8;
typedef uint32_t u32;

enum : int { DIGEST_BYTES = 32, BLOCK_BYTES = 64 };

ESM3_FN u32 rotl(u32 x, u32 r)
{
	r &= 31u;
	return r ? ((x << r) | (x >> (32u - r))) : x;
}
ESM3_FN u32 p0(u32 x) { return x ^ rotl(x, 9) ^ rotl(x, 17); }
ESM3_FN u32 p1(u32 x) { return x ^ rotl(x, 15) ^ rotl(x, 23); }

ESM3_FN void init(u32 *st)
{
	st[0] = 0x7380166fu; st[1] = 0x4914b2b9u; st[2] = 0x172442d7u; st[3] = 0xda8a0600u;
	st[4] = 0xa96f30bcu; st[5] = 0x163138aau; st[6] = 0xe38dee4du; st[7] = 0xb0fb0e4eu;
}

// one compression: st <- CF(st, block).  w (the block as 16 big-endian words) is used up as the expansion window.
ESM3_FN void compress(u32 *st, u32 *w)
{
	u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 r = 0; r < 64; r += 16) {
		const u32 T = r == 0 ? 0x79cc4519u : 0x7a879d8au;
#pragma unroll
		for (u32 t = 0; t < 16; t++) {
			// the window holds W_(r+t) .. W_(r+t+15) at [(t + k) & 15]
			const u32 wj = w[t], wj4 = w[(t + 4) & 15];
			const u32 a12 = rotl(a, 12);
			const u32 ss1 = rotl(a12 + e + rotl(T, r + t), 7);
			const u32 ss2 = ss1 ^ a12;
			const u32 ff = r == 0 ? (a ^ b ^ c) : ((a & b) | (a & c) | (b & c));
			const u32 gg = r == 0 ? (e ^ f ^ g) : ((e & f) | (~e & g));
			const u32 tt1 = ff + d + ss2 + (wj ^ wj4);
			const u32 tt2 = gg + h + ss1 + wj;
			d = c; c = rotl(b, 9); b = a; a = tt1;
			h = g; g = rotl(f, 19); f = e; e = p0(tt2);
			// W_(j+16) from W_j, W_(j+7), W_(j+13), W_(j+3), W_(j+10), into the place of W_j
			w[t] = p1(wj ^ w[(t + 7) & 15] ^ rotl(w[(t + 13) & 15], 15)) ^ rotl(w[(t + 3) & 15], 7) ^ w[(t + 10) & 15];
		}
	}
	st[0] ^= a; st[1] ^= b; st[2] ^= c; st[3] ^= d; st[4] ^= e; st[5] ^= f; st[6] ^= g; st[7] ^= h;
}

// absorb one whole block of 64 octets
ESM3_FN void absorb(u32 *st, const u8 *block)
{
	u32 w[16];
	for (int t = 0; t < 16; t++) {
		w[t] = ((u32)block[4 * t] << 24) | ((u32)block[4 * t + 1] << 16) | ((u32)block[4 * t + 2] << 8) | (u32)block[4 * t + 3];
	}
	compress(st, w);
}

// The end of a stream: `absorbed` octets (a multiple of 64) are in st already, `rest` more come from at(0) .. at(rest - 1); the
// padding counts both.  st is the digest's eight words afterwards.
template <class ByteAt> ESM3_FN void finish(u32 *st, u32 absorbed, u32 rest, const ByteAt &at)
{
	const u32 nblocks = (rest + 9u + 63u) / 64u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < nblocks; b++) {
		u32 w[16];
		for (u32 t = 0; t < 16; t++) {
			u32 v = 0;
			for (u32 k = 0; k < 4; k++) {
				const u32 pos = 64u * b + 4u * t + k;
				const u32 byte = pos < rest ? (u32)at(pos) : (pos == rest ? 0x80u : 0u);
				v = (v << 8) | byte;
			}
			w[t] = v;
		}
		if (b + 1 == nblocks) {
			w[15] = (absorbed + rest) << 3;   // (inputs are far below 2^29 octets: the count fits the last word)
		}
		compress(st, w);
	}
}

ESM3_FN u32 bswap(u32 x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

// big-endian word j of the padded message (msg: the message as little-endian words, readable up to the word that holds the
// last octet)
ESM3_FN u32 padded_word(const u32 *msg, u32 len, u32 j, u32 last_word)
{
	const u32 pos = 4u * j;
	u32 w = 0;
	if (pos < len) {
		w = bswap(msg[j]);
		const u32 rem = len - pos;
		if (rem < 4u) {
			const u32 keep = 0xffffffffu << (8u * (4u - rem));
			w = (w & keep) | (0x80u << (8u * (3u - rem)));
		}
	} else if (pos == len) {
		w = 0x80000000u;
	}
	if (j == last_word) {
		w = len << 3;
	}
	return w;
}

// SM3 of len octets (len < 2^29) held as words; the digest as eight big-endian words
ESM3_FN void hash_words(const u32 *msg, u32 len, u32 *dg)
{
	init(dg);
	const u32 nblocks = (len + 9u + 63u) / 64u, last_word = 16u * nblocks - 1u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < nblocks; b++) {
		u32 w[16];
#pragma unroll
		for (u32 t = 0; t < 16; t++) {
			w[t] = padded_word(msg, len, 16u * b + t, last_word);
		}
		compress(dg, w);
	}
}

// the digest's words as its 32 octets
ESM3_FN void digest_bytes(const u32 *dg, u8 *out)
{
	for (int k = 0; k < 8; k++) {
		out[4 * k] = (u8)(dg[k] >> 24);
		out[4 * k + 1] = (u8)(dg[k] >> 16);
		out[4 * k + 2] = (u8)(dg[k] >> 8);
		out[4 * k + 3] = (u8)dg[k];
	}
}

}  // namespace ecsm3
