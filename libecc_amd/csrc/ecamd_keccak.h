// libecc_amd/csrc/ecamd_keccak.h -- SHA3-224 / -256 / -384 / -512 (FIPS 202) per item: Keccak-f[1600] on 25 64-bit lanes held in
// registers, the sponge with the rate of each digest size, and a one-shot over a message held as little-endian words (the slot format
// of ecamd_hash.hip).  Compiles for the device (ecamd_hash3.hip: one item per lane) and for the host (tests/hash_table_host_shim.cpp).
//
// Written from the standard's definitions.  Lane (x, y) of the state is a[x + 5 y], its octets little-endian:
//
//   theta   C[x] = a[x, 0] ^ .. ^ a[x, 4];  D[x] = C[x - 1] ^ (C[x + 1] <<< 1);  a[x, y] ^= D[x]
//   rho/pi  b[y, 2 x + 3 y] = a[x, y] <<< RHO[x, y]
//   chi     a[x, y] = b[x, y] ^ (~b[x + 1, y] & b[x + 2, y])
//   iota    a[0, 0] ^= RC[round]                                   (24 rounds; RC: ECAMD_KECCAK_RC, indexed by the round number only)
//   sponge  rate = 200 - 2 hsize octets (144, 136, 104, 72); the message, then 0x06, zeros, and 0x80 into the last octet of the last
//           block (one octet 0x86 where they meet); every block is XORed into the first rate octets and permuted; the digest is the first
//           hsize octets of the state
//
// This unit has its own copy of the permutation: keccak_f1600 of ecamd_hash.hip (SHAKE256 for Ed448) stays as it is.  On the device
// the 24 rounds are unrolled, so every rotation count and every lane index is a constant and the state never leaves registers.
//
// SECRET DATA: none.  What is hashed here is a message; there is no table indexed by data.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EKK_FN __host__ __device__ __forceinline__
#else
#define EKK_FN inline
#endif

// FIPS 202 section 3.2.5: the round constants of iota
#define ECAMD_KECCAK_RC                                                                                                                       \
	0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,                    \
	0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,                    \
	0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,                    \
	0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,                    \
	0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull

namespace eckk {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

// libecc's hash_alg_type number (SHA3_224 = 5 .. SHA3_512 = 8) -> digest octets, 0: not one of the four
EKK_FN int hash_size(int hash_type)
{
	return hash_type == 5 ? 28 : hash_type == 6 ? 32 : hash_type == 7 ? 48 : hash_type == 8 ? 64 : 0;
}
// the rate in octets
EKK_FN int block_size(int hash_type)
{
	const int hs = hash_size(hash_type);
	return hs ? 200 - 2 * hs : 0;
}

EKK_FN u64 rotl(u64 x, int r) { return r ? ((x << r) | (x >> (64 - r))) : x; }

// Keccak-f[1600]
template <class RC> EKK_FN void permute(u64 *a, const RC &rc)
{
	// rho's offsets by lane index x + 5 y
	constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
#pragma unroll
	for (int round = 0; round < 24; round++) {
		u64 c[5], b[25];
#pragma unroll
		for (int x = 0; x < 5; x++) {
			c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
		}
#pragma unroll
		for (int x = 0; x < 5; x++) {
			const u64 d = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1);
#pragma unroll
			for (int y = 0; y < 5; y++) {
				b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y] ^ d, RHO[x + 5 * y]);
			}
		}
#pragma unroll
		for (int y = 0; y < 5; y++) {
#pragma unroll
			for (int x = 0; x < 5; x++) {
				a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
			}
		}
		a[0] ^= (u64)rc[round];
	}
}

// little-endian word j (32 bits) of the message with the octet `pad` behind its last octet and zeros after (msg: the message as
// little-endian words, readable up to the word that holds the last octet)
EKK_FN u32 padded_word(const u32 *msg, u32 len, u32 j, u32 pad)
{
	const u32 pos = 4u * j;
	if (pos > len) {
		return 0u;
	}
	if (pos == len) {
		return pad;
	}
	const u32 w = msg[j], rem = len - pos;
	return rem >= 4u ? w : ((w & (0xffffffffu >> (8u * (4u - rem)))) | (pad << (8u * rem)));
}

// SHA3 of len octets (len < 2^29) held as words; st: the 25 lanes of the final state.  HSIZE: 28, 32, 48 or 64.
template <int HSIZE, class RC> EKK_FN void hash_words(const RC &rc, const u32 *msg, u32 len, u64 *st)
{
	constexpr u32 RATE = 200u - 2u * (u32)HSIZE, LANES = RATE / 8u;
#pragma unroll
	for (int k = 0; k < 25; k++) {
		st[k] = 0;
	}
	const u32 nfull = len / RATE;
	// iteration nfull is the rest (possibly empty) with the padding
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b <= nfull; b++) {
#pragma unroll
		for (u32 w = 0; w < LANES; w++) {
			const u32 j = 2u * (LANES * b + w);
			st[w] ^= (u64)padded_word(msg, len, j, 0x06u) | ((u64)padded_word(msg, len, j + 1u, 0x06u) << 32);
		}
		if (b == nfull) {
			st[LANES - 1u] ^= 0x8000000000000000ull;
		}
		permute(st, rc);
	}
}

// the first HSIZE octets of the state
template <int HSIZE> EKK_FN void digest_bytes(const u64 *st, u8 *out)
{
#pragma unroll
	for (int k = 0; k < HSIZE; k++) {
		out[k] = (u8)(st[k >> 3] >> (8 * (k & 7)));
	}
}

// one slot (a little-endian u32 length, then the octets; stride a multiple of 4) -> HSIZE octets at out; a length that does not fit
// the slot gives zeros
template <int HSIZE, class RC> EKK_FN void slot_digest(const RC &rc, const u8 *slot, u32 stride, u8 *out)
{
	const u32 *words = (const u32 *)slot;
	const u32 len = words[0];
	u64 st[25];
	if (len > stride - 4u) {
#pragma unroll
		for (int k = 0; k < 25; k++) {
			st[k] = 0;
		}
	} else {
		hash_words<HSIZE>(rc, words + 1, len, st);
	}
	digest_bytes<HSIZE>(st, out);
}

}  // namespace eckk
