// libecc_amd/csrc/ecamd_streebog.h -- Streebog-256 and Streebog-512 (GOST R 34.11-2012, RFC 6986), the hashes ECRDSA (GOST R 34.10-2012)
// is specified with, per item.  Compiles for the device (ecamd_hash2.hip: one item per lane) and for the host
// (tests/sighash2_host_shim.cpp).
//
// Written from the standard's definitions, on eight 64-bit words per 512-bit vector (word j = octets 8j .. 8j + 7 of the vector
// read as a little-endian integer, so nothing is byte-swapped on gfx950 or x86):
//
//   pi           the standard's 8-bit substitution (table below), S = pi on every octet
//   P            the transposition of the 8 x 8 octet matrix
//   L            every 64-bit row times the matrix A over GF(2) (64 rows below, in the standard's order: row 0 belongs to the
//                most significant bit)
//   LPS(x)       all three at once through T[j][b] = the L-contribution of pi(b) in octet j of a row:
//                out[i] = XOR over j of T[j][octet i of x[j]];  T[j][b] = XOR over the set bits k of pi(b) of A[8 (7 - j) + (7 - k)]
//                (table_entry below: the table is BUILT from pi and A, 8 x 256 x 64 bits = 16 KiB, never stored in the source)
//   g_N(h, m)    K = LPS(h ^ N), t = LPS(K ^ m), then twelve times K = LPS(K ^ C_r) with t = LPS(K ^ t) in between (the last key
//                is only XORed): h ^= t ^ K ^ m
//   hash         h = 0 (512) or 0x01 in every octet (256), N = Sigma = 0; per whole block m: g_N, N += 512, Sigma += m; the
//                rest with 0x01 behind it and zeros: g_N, N += its bits, Sigma += m; then g_0(h, N), g_0(h, Sigma).
//                N and Sigma are sums mod 2^512: the carries run through all eight words (add512).
//   digest       Streebog-512: the eight words of h; Streebog-256: words 4 .. 7
//
// Byte order: the message's first octet is the least significant octet of word 0 and the digest is the words' little-endian octets,
// word 0 (or 4) first.  That is the order of libecc's hash/streebog.c, which the signature schemes are checked against
// (tests/golden/sig_msg.json pins it); the examples of RFC 6986 print the same vectors most significant octet first.
//
// The table and the round constants are reached through template parameters (anything indexable): the kernel passes a pointer into
// LDS for T and a __constant__ array for C, the host build plain arrays.
//
// SECRET DATA: none.  Every look-up is indexed by octets derived from the message, which is public for all three signature
// schemes (ECRDSA and ECGDSA hash the message, SM2 the message behind Z), and so are h, N and Sigma: no scanned variant of the
// table look-up is needed, in secret-scalar mode (ecamd_ctx_set_secret_scalars) either.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ESB_FN __host__ __device__ __forceinline__
#else
#define ESB_FN inline
#endif

// the substitution pi of GOST R 34.11-2012 (row = high nibble, column = low nibble)
#define ECAMD_STREEBOG_PI                                                                                                  \
	0xFC, 0xEE, 0xDD, 0x11, 0xCF, 0x6E, 0x31, 0x16, 0xFB, 0xC4, 0xFA, 0xDA, 0x23, 0xC5, 0x04, 0x4D, /* 0 */            \
	0xE9, 0x77, 0xF0, 0xDB, 0x93, 0x2E, 0x99, 0xBA, 0x17, 0x36, 0xF1, 0xBB, 0x14, 0xCD, 0x5F, 0xC1, /* 1 */            \
	0xF9, 0x18, 0x65, 0x5A, 0xE2, 0x5C, 0xEF, 0x21, 0x81, 0x1C, 0x3C, 0x42, 0x8B, 0x01, 0x8E, 0x4F, /* 2 */            \
	0x05, 0x84, 0x02, 0xAE, 0xE3, 0x6A, 0x8F, 0xA0, 0x06, 0x0B, 0xED, 0x98, 0x7F, 0xD4, 0xD3, 0x1F, /* 3 */            \
	0xEB, 0x34, 0x2C, 0x51, 0xEA, 0xC8, 0x48, 0xAB, 0xF2, 0x2A, 0x68, 0xA2, 0xFD, 0x3A, 0xCE, 0xCC, /* 4 */            \
	0xB5, 0x70, 0x0E, 0x56, 0x08, 0x0C, 0x76, 0x12, 0xBF, 0x72, 0x13, 0x47, 0x9C, 0xB7, 0x5D, 0x87, /* 5 */            \
	0x15, 0xA1, 0x96, 0x29, 0x10, 0x7B, 0x9A, 0xC7, 0xF3, 0x91, 0x78, 0x6F, 0x9D, 0x9E, 0xB2, 0xB1, /* 6 */            \
	0x32, 0x75, 0x19, 0x3D, 0xFF, 0x35, 0x8A, 0x7E, 0x6D, 0x54, 0xC6, 0x80, 0xC3, 0xBD, 0x0D, 0x57, /* 7 */            \
	0xDF, 0xF5, 0x24, 0xA9, 0x3E, 0xA8, 0x43, 0xC9, 0xD7, 0x79, 0xD6, 0xF6, 0x7C, 0x22, 0xB9, 0x03, /* 8 */            \
	0xE0, 0x0F, 0xEC, 0xDE, 0x7A, 0x94, 0xB0, 0xBC, 0xDC, 0xE8, 0x28, 0x50, 0x4E, 0x33, 0x0A, 0x4A, /* 9 */            \
	0xA7, 0x97, 0x60, 0x73, 0x1E, 0x00, 0x62, 0x44, 0x1A, 0xB8, 0x38, 0x82, 0x64, 0x9F, 0x26, 0x41, /* A */            \
	0xAD, 0x45, 0x46, 0x92, 0x27, 0x5E, 0x55, 0x2F, 0x8C, 0xA3, 0xA5, 0x7D, 0x69, 0xD5, 0x95, 0x3B, /* B */            \
	0x07, 0x58, 0xB3, 0x40, 0x86, 0xAC, 0x1D, 0xF7, 0x30, 0x37, 0x6B, 0xE4, 0x88, 0xD9, 0xE7, 0x89, /* C */            \
	0xE1, 0x1B, 0x83, 0x49, 0x4C, 0x3F, 0xF8, 0xFE, 0x8D, 0x53, 0xAA, 0x90, 0xCA, 0xD8, 0x85, 0x61, /* D */            \
	0x20, 0x71, 0x67, 0xA4, 0x2D, 0x2B, 0x09, 0x5B, 0xCB, 0x9B, 0x25, 0xD0, 0xBE, 0xE5, 0x6C, 0x52, /* E */            \
	0x59, 0xA6, 0x74, 0xD2, 0xE6, 0xF4, 0xB4, 0xC0, 0xD1, 0x66, 0xAF, 0xC2, 0x39, 0x4B, 0x63, 0xB6  /* F */

// the 64 rows of the matrix A of the linear map l, in the standard's order
#define ECAMD_STREEBOG_A                                                                                                   \
	0x8e20faa72ba0b470ull, 0x47107ddd9b505a38ull, 0xad08b0e0c3282d1cull, 0xd8045870ef14980eull,                        \
	0x6c022c38f90a4c07ull, 0x3601161cf205268dull, 0x1b8e0b0e798c13c8ull, 0x83478b07b2468764ull,                        \
	0xa011d380818e8f40ull, 0x5086e740ce47c920ull, 0x2843fd2067adea10ull, 0x14aff010bdd87508ull,                        \
	0x0ad97808d06cb404ull, 0x05e23c0468365a02ull, 0x8c711e02341b2d01ull, 0x46b60f011a83988eull,                        \
	0x90dab52a387ae76full, 0x486dd4151c3dfdb9ull, 0x24b86a840e90f0d2ull, 0x125c354207487869ull,                        \
	0x092e94218d243cbaull, 0x8a174a9ec8121e5dull, 0x4585254f64090fa0ull, 0xaccc9ca9328a8950ull,                        \
	0x9d4df05d5f661451ull, 0xc0a878a0a1330aa6ull, 0x60543c50de970553ull, 0x302a1e286fc58ca7ull,                        \
	0x18150f14b9ec46ddull, 0x0c84890ad27623e0ull, 0x0642ca05693b9f70ull, 0x0321658cba93c138ull,                        \
	0x86275df09ce8aaa8ull, 0x439da0784e745554ull, 0xafc0503c273aa42aull, 0xd960281e9d1d5215ull,                        \
	0xe230140fc0802984ull, 0x71180a8960409a42ull, 0xb60c05ca30204d21ull, 0x5b068c651810a89eull,                        \
	0x456c34887a3805b9ull, 0xac361a443d1c8cd2ull, 0x561b0d22900e4669ull, 0x2b838811480723baull,                        \
	0x9bcf4486248d9f5dull, 0xc3e9224312c8c1a0ull, 0xeffa11af0964ee50ull, 0xf97d86d98a327728ull,                        \
	0xe4fa2054a80b329cull, 0x727d102a548b194eull, 0x39b008152acb8227ull, 0x9258048415eb419dull,                        \
	0x492c024284fbaec0ull, 0xaa16012142f35760ull, 0x550b8e9e21f7a530ull, 0xa48b474f9ef5dc18ull,                        \
	0x70a6a56e2440598eull, 0x3853dc371220a247ull, 0x1ca76e95091051adull, 0x0edd37c48a08a6d8ull,                        \
	0x07e095624504536cull, 0x8d70c431ac02a736ull, 0xc83862965601dd1bull, 0x641c314b2b8ee083ull

// the twelve round constants C_1 .. C_12 as the standard prints them: eight words each, the most significant first
#define ECAMD_STREEBOG_C                                                                                                   \
	0xb1085bda1ecadae9ull, 0xebcb2f81c0657c1full, 0x2f6a76432e45d016ull, 0x714eb88d7585c4fcull,                        \
	0x4b7ce09192676901ull, 0xa2422a08a460d315ull, 0x05767436cc744d23ull, 0xdd806559f2a64507ull, /* C1 */               \
	0x6fa3b58aa99d2f1aull, 0x4fe39d460f70b5d7ull, 0xf3feea720a232b98ull, 0x61d55e0f16b50131ull,                        \
	0x9ab5176b12d69958ull, 0x5cb561c2db0aa7caull, 0x55dda21bd7cbcd56ull, 0xe679047021b19bb7ull, /* C2 */               \
	0xf574dcac2bce2fc7ull, 0x0a39fc286a3d8435ull, 0x06f15e5f529c1f8bull, 0xf2ea7514b1297b7bull,                        \
	0xd3e20fe490359eb1ull, 0xc1c93a376062db09ull, 0xc2b6f443867adb31ull, 0x991e96f50aba0ab2ull, /* C3 */               \
	0xef1fdfb3e81566d2ull, 0xf948e1a05d71e4ddull, 0x488e857e335c3c7dull, 0x9d721cad685e353full,                        \
	0xa9d72c82ed03d675ull, 0xd8b71333935203beull, 0x3453eaa193e837f1ull, 0x220cbebc84e3d12eull, /* C4 */               \
	0x4bea6bacad474799ull, 0x9a3f410c6ca92363ull, 0x7f151c1f1686104aull, 0x359e35d7800fffbdull,                        \
	0xbfcd1747253af5a3ull, 0xdfff00b723271a16ull, 0x7a56a27ea9ea63f5ull, 0x601758fd7c6cfe57ull, /* C5 */               \
	0xae4faeae1d3ad3d9ull, 0x6fa4c33b7a3039c0ull, 0x2d66c4f95142a46cull, 0x187f9ab49af08ec6ull,                        \
	0xcffaa6b71c9ab7b4ull, 0x0af21f66c2bec6b6ull, 0xbf71c57236904f35ull, 0xfa68407a46647d6eull, /* C6 */               \
	0xf4c70e16eeaac5ecull, 0x51ac86febf240954ull, 0x399ec6c7e6bf87c9ull, 0xd3473e33197a93c9ull,                        \
	0x0992abc52d822c37ull, 0x06476983284a0504ull, 0x3517454ca23c4af3ull, 0x8886564d3a14d493ull, /* C7 */               \
	0x9b1f5b424d93c9a7ull, 0x03e7aa020c6e4141ull, 0x4eb7f8719c36de1eull, 0x89b4443b4ddbc49aull,                        \
	0xf4892bcb929b0690ull, 0x69d18d2bd1a5c42full, 0x36acc2355951a8d9ull, 0xa47f0dd4bf02e71eull, /* C8 */               \
	0x378f5a541631229bull, 0x944c9ad8ec165fdeull, 0x3a7d3a1b25894224ull, 0x3cd955b7e00d0984ull,                        \
	0x800a440bdbb2ceb1ull, 0x7b2b8a9aa6079c54ull, 0x0e38dc92cb1f2a60ull, 0x7261445183235adbull, /* C9 */               \
	0xabbedea680056f52ull, 0x382ae548b2e4f3f3ull, 0x8941e71cff8a78dbull, 0x1fffe18a1b336103ull,                        \
	0x9fe76702af69334bull, 0x7a1e6c303b7652f4ull, 0x3698fad1153bb6c3ull, 0x74b4c7fb98459cedull, /* C10 */              \
	0x7bcd9ed0efc889fbull, 0x3002c6cd635afe94ull, 0xd8fa6bbbebab0761ull, 0x2001802114846679ull,                        \
	0x8a1d71efea48b9caull, 0xefbacd1d7d476e98ull, 0xdea2594ac06fd85dull, 0x6bcaa4cd81f32d1bull, /* C11 */              \
	0x378ee767f11631baull, 0xd21380b00449b17aull, 0xcda43c32bcdf1d77ull, 0xf82012d430219f9bull,                        \
	0x5d80ef9d1891cc86ull, 0xe71da4aa88e12852ull, 0xfaf417d5d9b21b99ull, 0x48bc924af11bd720ull /* C12 */

namespace ecsb {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum : int { BLOCK_BYTES = 64, TABLE_WORDS = 8 * 256 };

// hash_type: libecc's hash_alg_type number (STREEBOG256 = 13, STREEBOG512 = 14) -> digest octets, 0: neither
ESB_FN int hash_size(int hash_type) { return hash_type == 13 ? 32 : hash_type == 14 ? 64 : 0; }

// T[j][b], kept at index 256 j + b: the row that octet value b contributes from octet position j
template <class PiT, class AT> ESB_FN u64 table_entry(const PiT &pi, const AT &A, u32 j, u32 b)
{
	const u32 v = (u32)pi[b];
	u64 t = 0;
	for (u32 k = 0; k < 8; k++) {
		t ^= ((v >> k) & 1u) ? (u64)A[8u * (7u - j) + (7u - k)] : (u64)0;
	}
	return t;
}

// out = LPS(a ^ b); out may be a or b
template <class Tab> ESB_FN void xlps(const Tab &T, const u64 *a, const u64 *b, u64 *out)
{
	u64 x[8], r[8];
#pragma unroll
	for (int j = 0; j < 8; j++) {
		x[j] = a[j] ^ b[j];
	}
#pragma unroll
	for (int i = 0; i < 8; i++) {
		u64 t = 0;
#pragma unroll
		for (int j = 0; j < 8; j++) {
			t ^= (u64)T[256 * j + (int)((x[j] >> (8 * i)) & 0xffu)];
		}
		r[i] = t;
	}
#pragma unroll
	for (int i = 0; i < 8; i++) {
		out[i] = r[i];
	}
}

// h <- g_N(h, m).  C: the 96 words of ECAMD_STREEBOG_C (word j of C_r is C[8 (r - 1) + 7 - j]).
template <class Tab, class CT> ESB_FN void g_n(const Tab &T, const CT &C, u64 *h, const u64 *m, const u64 *N)
{
	u64 K[8], t[8], c[8];
	xlps(T, h, N, K);
	xlps(T, K, m, t);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (int r = 0; r < 12; r++) {
#pragma unroll
		for (int j = 0; j < 8; j++) {
			c[j] = (u64)C[8 * r + 7 - j];
		}
		xlps(T, K, c, K);
		if (r < 11) {
			xlps(T, K, t, t);
		}
	}
#pragma unroll
	for (int j = 0; j < 8; j++) {
		h[j] ^= t[j] ^ K[j] ^ m[j];
	}
}

// acc += v mod 2^512
ESB_FN void add512(u64 *acc, const u64 *v)
{
	u64 carry = 0;
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const u64 s = acc[j] + v[j];
		const u64 c1 = s < v[j] ? 1u : 0u;
		const u64 s2 = s + carry;
		const u64 c2 = s2 < carry ? 1u : 0u;
		acc[j] = s2;
		carry = c1 | c2;
	}
}

// little-endian word j (32 bits) of the message with its padding octet 0x01 behind the last octet (msg: the message as
// little-endian words, readable up to the word that holds the last octet)
ESB_FN u32 padded_word(const u32 *msg, u32 len, u32 j)
{
	const u32 pos = 4u * j;
	if (pos > len) {
		return 0u;
	}
	if (pos == len) {
		return 1u;
	}
	const u32 w = msg[j], rem = len - pos;
	return rem >= 4u ? w : ((w & (0xffffffffu >> (8u * (4u - rem)))) | (1u << (8u * rem)));
}

// Streebog of len octets (len < 2^29) held as words; h: the eight words of the final state.  BITS: 256 or 512.
template <int BITS, class Tab, class CT> ESB_FN void hash_words(const Tab &T, const CT &C, const u32 *msg, u32 len, u64 *h)
{
	u64 N[8], S[8], M[8], Z[8];
#pragma unroll
	for (int j = 0; j < 8; j++) {
		h[j] = BITS == 256 ? 0x0101010101010101ull : 0ull;
		N[j] = 0;
		S[j] = 0;
		Z[j] = 0;
	}
	const u32 nfull = len / 64u;
	// iteration nfull is the rest (possibly empty) with its padding
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b <= nfull; b++) {
#pragma unroll
		for (u32 j = 0; j < 8; j++) {
			M[j] = (u64)padded_word(msg, len, 16u * b + 2u * j) | ((u64)padded_word(msg, len, 16u * b + 2u * j + 1u) << 32);
		}
		g_n(T, C, h, M, N);
		u64 bits[8] = {b < nfull ? (u64)512 : (u64)(8u * (len & 63u)), 0, 0, 0, 0, 0, 0, 0};
		add512(N, bits);
		add512(S, M);
	}
	g_n(T, C, h, N, Z);
	g_n(T, C, h, S, Z);
}

// the state's words as the digest's octets
template <int BITS> ESB_FN void digest_bytes(const u64 *h, u8 *out)
{
	const int first = BITS == 256 ? 4 : 0;
	for (int j = first; j < 8; j++) {
		for (int k = 0; k < 8; k++) {
			out[8 * (j - first) + k] = (u8)(h[j] >> (8 * k));
		}
	}
}

}  // namespace ecsb
