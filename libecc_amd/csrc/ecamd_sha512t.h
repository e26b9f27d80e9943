// libecc_amd/csrc/ecamd_sha512t.h -- SHA-512/224 and SHA-512/256 (FIPS 180-4 sections 5.3.6, 6.7) per item: the SHA-512 compression of
// ecamd_rfc6979.h (ecrfc::compress<512>) from the two truncated variants' own initial values, the digest cut to 28 / 32 octets, and a
// one-shot over a message held as little-endian words (the slot format of ecamd_hash.hip).  Compiles for the device (ecamd_hash3.hip:
// one item per lane) and for the host (tests/hash_table_host_shim.cpp).  k_sha2_slots of ecamd_hash.hip is not involved.
//
//   block 128 octets; padding 0x80, zeros, the bit count in the last sixteen octets (here: the last word; messages are far below
//   2^29 octets); T = 224: the first 28 octets of H0 .. H3 big-endian, T = 256: H0 .. H3
//
// SECRET DATA: none.  What is hashed here is a message; the round constants are indexed by the round number only.
#pragma once
#include <stdint.h>
#include "ecamd_rfc6979.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ES5T_FN __host__ __device__ __forceinline__
#else
#define ES5T_FN inline
#endif

namespace ecs5t {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum : int { BLOCK_BYTES = 128 };

// libecc's hash_alg_type number (SHA512_224 = 9, SHA512_256 = 10) -> digest octets, 0: neither
ES5T_FN int hash_size(int hash_type) { return hash_type == 9 ? 28 : hash_type == 10 ? 32 : 0; }
ES5T_FN int block_size(int hash_type) { return hash_size(hash_type) ? (int)BLOCK_BYTES : 0; }

// FIPS 180-4 5.3.6.1 / 5.3.6.2
template <int T> ES5T_FN void init(u64 *h)
{
	if (T == 224) {
		h[0] = 0x8c3d37c819544da2ull; h[1] = 0x73e1996689dcd4d6ull; h[2] = 0x1dfab7ae32ff9c82ull; h[3] = 0x679dd514582f9fcfull;
		h[4] = 0x0f6d2b697bd44da8ull; h[5] = 0x77e36f7304c48942ull; h[6] = 0x3f9d85a86a1d36c8ull; h[7] = 0x1112e6ad91d692a1ull;
	} else {
		h[0] = 0x22312194fc2bf72cull; h[1] = 0x9f555fa3c84c64c2ull; h[2] = 0x2393b86b6f53b151ull; h[3] = 0x963877195940eabdull;
		h[4] = 0x96283ee2a88effe3ull; h[5] = 0xbe5e1e2553863992ull; h[6] = 0x2b0199fc2c85b8aaull; h[7] = 0x0eb72ddc81c52ca2ull;
	}
}

ES5T_FN u32 bswap(u32 x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

// big-endian word j (32 bits) of the padded message (msg: the message as little-endian words, readable up to the word that holds the
// last octet)
ES5T_FN u32 padded_word(const u32 *msg, u32 len, u32 j, u32 last_word)
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

// SHA-512/T of len octets (len < 2^29) held as words; h: the eight words of the final state.  K: ECAMD_SHA512_K.
template <int T, class KT> ES5T_FN void hash_words(const KT &K, const u32 *msg, u32 len, u64 *h)
{
	init<T>(h);
	const u32 nblocks = (len + 17u + 127u) / 128u, last_word = 32u * nblocks - 1u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < nblocks; b++) {
		u64 w[16];
#pragma unroll
		for (u32 t = 0; t < 16; t++) {
			const u32 j = 32u * b + 2u * t;
			w[t] = ((u64)padded_word(msg, len, j, last_word) << 32) | padded_word(msg, len, j + 1u, last_word);
		}
		ecrfc::compress<512>(h, w, K);
	}
}

// the first T / 8 octets of the state, big-endian
template <int T> ES5T_FN void digest_bytes(const u64 *h, u8 *out)
{
#pragma unroll
	for (int k = 0; k < T / 8; k++) {
		out[k] = (u8)(h[k >> 3] >> (56 - 8 * (k & 7)));
	}
}

// one slot (a little-endian u32 length, then the octets; stride a multiple of 4) -> T / 8 octets at out; a length that does not fit
// the slot gives zeros
template <int T, class KT> ES5T_FN void slot_digest(const KT &K, const u8 *slot, u32 stride, u8 *out)
{
	const u32 *words = (const u32 *)slot;
	const u32 len = words[0];
	u64 h[8];
	if (len > stride - 4u) {
#pragma unroll
		for (int k = 0; k < 8; k++) {
			h[k] = 0;
		}
	} else {
		hash_words<T>(K, words + 1, len, h);
	}
	digest_bytes<T>(h, out);
}

}  // namespace ecs5t
