// libecc_amd/csrc/ecamd_bash.h -- BASH224 / 256 / 384 / 512 (STB 34.101.77, bash-hash) per item, as libecc runs it on a little-endian
// host: the permutation bash-f on 24 64-bit words held in registers, the sponge, and a one-shot over a message held as little-endian
// words (the slot format of ecamd_hash.hip).  Compiles for the device (ecamd_hash3.hip: one item per lane) and for the host
// (tests/hash_table_host_shim.cpp).  These are the hashes BIGN is specified with on bign384v1 (BASH384) and bign512v1 (BASH512).
//
// Written from the standard's definitions.  The state is 24 words S[0 .. 23], octets little-endian, seen as 8 columns (S[v], S[v + 8],
// S[v + 16]):
//
//   bash-s     on a column (W0, W1, W2) with the rotations (m1, n1, m2, n2):
//                T0 = W0 <<< m1;  W0 ^= W1 ^ W2;  T1 = W1 ^ (W0 <<< n1);  W1 = T0 ^ T1;  W2 ^= (W2 <<< m2) ^ (T1 <<< n2);
//                then with the new values, all three at once:  W0 ^= ~W2 | W1;  W1 ^= W0 | W2;  W2 ^= W0 & W1
//   rotations  column 0: (8, 53, 14, 1); column v + 1: those of column v times 7 mod 64
//   round      bash-s on every column, the word permutation PERM (new S[i] = old S[PERM[i]]), S[23] ^= C[round]; 24 rounds
//   constants  C[0] = 3bf5080ac8ba94b1, C[t + 1] = C[t] >> 1, XORed with dc2be1997fe0d8ae where C[t] is odd (ECAMD_BASH_RC;
//              tests/test_hash_table_host.py checks the list against this rule)
//   sponge     hsize = 28, 32, 48, 64 octets of digest; rate = 192 - 2 hsize octets (136, 128, 96, 64).  The state starts as zeros
//              with the octet hsize at offset 184 (the low octet of S[23]).  Each block is WRITTEN OVER the first rate octets (not
//              XORed) and the state permuted; the last block is the rest of the message (possibly empty), the octet 0x40 and zeros.
//              The digest is the first hsize octets of the state.
//
// On the device the 24 rounds are unrolled: the permutation of the words is then a renaming of registers, and every rotation count is
// a constant.
//
// SECRET DATA: none.  What is hashed here is a message; there is no table indexed by data.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EBSH_FN __host__ __device__ __forceinline__
#else
#define EBSH_FN inline
#endif

// STB 34.101.77: the round constants C_1 .. C_24
#define ECAMD_BASH_RC                                                                                                                         \
	0x3bf5080ac8ba94b1ull, 0xc1d1659c1bbd92f6ull, 0x60e8b2ce0ddec97bull, 0xec5fb8fe790fbc13ull, 0xaa043de6436706a7ull,                    \
	0x8929ff6a5e535bfdull, 0x98bf1e2c50c97550ull, 0x4c5f8f162864baa8ull, 0x262fc78b14325d54ull, 0x1317e3c58a192eaaull,                    \
	0x098bf1e2c50c9755ull, 0xd8ee19681d669304ull, 0x6c770cb40eb34982ull, 0x363b865a0759a4c1ull, 0xc73622b47c4c0aceull,                    \
	0x639b115a3e260567ull, 0xede6693460f3da1dull, 0xaad8d5034f9935a0ull, 0x556c6a81a7cc9ad0ull, 0x2ab63540d3e64d68ull,                    \
	0x155b1aa069f326b4ull, 0x0aad8d5034f9935aull, 0x0556c6a81a7cc9adull, 0xde8082cd72debc78ull

namespace ecbash {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

// libecc's hash_alg_type number (BASH224 = 17 .. BASH512 = 20) -> digest octets, 0: not one of the four
EBSH_FN int hash_size(int hash_type)
{
	return hash_type == 17 ? 28 : hash_type == 18 ? 32 : hash_type == 19 ? 48 : hash_type == 20 ? 64 : 0;
}
// the rate in octets
EBSH_FN int block_size(int hash_type)
{
	const int hs = hash_size(hash_type);
	return hs ? 192 - 2 * hs : 0;
}

EBSH_FN u64 rotl(u64 x, int r) { return r ? ((x << r) | (x >> (64 - r))) : x; }

// rotation k (m1, n1, m2, n2) of column v: the first column's times 7^v mod 64
constexpr int rot_of(int v, int k)
{
	int r = k == 0 ? 8 : k == 1 ? 53 : k == 2 ? 14 : 1;
	for (int i = 0; i < v; i++) {
		r = (7 * r) & 63;
	}
	return r;
}

template <int V> EBSH_FN void column(u64 &w0, u64 &w1, u64 &w2)
{
	constexpr int M1 = rot_of(V, 0), N1 = rot_of(V, 1), M2 = rot_of(V, 2), N2 = rot_of(V, 3);
	// the linear half
	const u64 t0 = rotl(w0, M1);
	const u64 x0 = w0 ^ w1 ^ w2;
	const u64 t1 = w1 ^ rotl(x0, N1);
	const u64 x1 = t0 ^ t1;
	const u64 x2 = w2 ^ rotl(w2, M2) ^ rotl(t1, N2);
	// the three S-boxes, bit-sliced
	w0 = x0 ^ (~x2 | x1);
	w1 = x1 ^ (x0 | x2);
	w2 = x2 ^ (x0 & x1);
}

// bash-f
template <class RC> EBSH_FN void permute(u64 *s, const RC &rc)
{
	constexpr int PERM[24] = {15, 10, 9, 12, 11, 14, 13, 8, 17, 16, 19, 18, 21, 20, 23, 22, 6, 3, 0, 5, 2, 7, 4, 1};
#pragma unroll
	for (int round = 0; round < 24; round++) {
		column<0>(s[0], s[8], s[16]);
		column<1>(s[1], s[9], s[17]);
		column<2>(s[2], s[10], s[18]);
		column<3>(s[3], s[11], s[19]);
		column<4>(s[4], s[12], s[20]);
		column<5>(s[5], s[13], s[21]);
		column<6>(s[6], s[14], s[22]);
		column<7>(s[7], s[15], s[23]);
		u64 t[24];
#pragma unroll
		for (int i = 0; i < 24; i++) {
			t[i] = s[PERM[i]];
		}
#pragma unroll
		for (int i = 0; i < 24; i++) {
			s[i] = t[i];
		}
		s[23] ^= (u64)rc[round];
	}
}

// little-endian word j (32 bits) of the message with the octet 0x40 behind its last octet and zeros after (msg: the message as
// little-endian words, readable up to the word that holds the last octet)
EBSH_FN u32 padded_word(const u32 *msg, u32 len, u32 j)
{
	const u32 pos = 4u * j;
	if (pos > len) {
		return 0u;
	}
	if (pos == len) {
		return 0x40u;
	}
	const u32 w = msg[j], rem = len - pos;
	return rem >= 4u ? w : ((w & (0xffffffffu >> (8u * (4u - rem)))) | (0x40u << (8u * rem)));
}

// BASH of len octets (len < 2^29) held as words; s: the 24 words of the final state.  BITS: 224, 256, 384 or 512.
template <int BITS, class RC> EBSH_FN void hash_words(const RC &rc, const u32 *msg, u32 len, u64 *s)
{
	constexpr u32 HSIZE = (u32)BITS / 8u, RATE = 192u - 2u * HSIZE, WORDS = RATE / 8u;
#pragma unroll
	for (int k = 0; k < 23; k++) {
		s[k] = 0;
	}
	s[23] = HSIZE;
	const u32 nfull = len / RATE;
	// iteration nfull is the rest (possibly empty) with the padding
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b <= nfull; b++) {
#pragma unroll
		for (u32 w = 0; w < WORDS; w++) {
			const u32 j = 2u * (WORDS * b + w);
			s[w] = (u64)padded_word(msg, len, j) | ((u64)padded_word(msg, len, j + 1u) << 32);
		}
		permute(s, rc);
	}
}

// the first BITS / 8 octets of the state
template <int BITS> EBSH_FN void digest_bytes(const u64 *s, u8 *out)
{
#pragma unroll
	for (int k = 0; k < BITS / 8; k++) {
		out[k] = (u8)(s[k >> 3] >> (8 * (k & 7)));
	}
}

// one slot (a little-endian u32 length, then the octets; stride a multiple of 4) -> BITS / 8 octets at out; a length that does not
// fit the slot gives zeros
template <int BITS, class RC> EBSH_FN void slot_digest(const RC &rc, const u8 *slot, u32 stride, u8 *out)
{
	const u32 *words = (const u32 *)slot;
	const u32 len = words[0];
	u64 s[24];
	if (len > stride - 4u) {
#pragma unroll
		for (int k = 0; k < 24; k++) {
			s[k] = 0;
		}
	} else {
		hash_words<BITS>(rc, words + 1, len, s);
	}
	digest_bytes<BITS>(s, out);
}

}  // namespace ecbash
