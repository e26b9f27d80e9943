// libecc_amd/csrc/ecamd_belt.h -- the BelT block cipher and BelT-hash of STB 34.101.31, for BIGN (STB 34.101.45), which hashes its
// commitment with BelT-hash whatever hash the message had.
//
// Written from the standard's definitions, on 32-bit little-endian words (the standard's octet strings read as words u1 u2 ...
// are little-endian words, so nothing is byte-swapped on gfx950 or x86):
//
//   H            the standard's 8-bit substitution (table below)
//   G_r(u)       H on each of the four octets of u, then a rotation to the left by r bits
//   F_theta(X)   the block cipher: X = a || b || c || d (128 bits), theta = theta_1 .. theta_8 (256 bits); eight rounds of seven
//                G steps; the round keys are K_j = theta_((j - 1) mod 8 + 1), j = 1 .. 56, so round i uses K_(7i-6) .. K_(7i)
//   sigma1(u)    u = u1 || u2 || u3 || u4 (128 bits each): F_(u1 || u2)(u3 ^ u4) ^ u3 ^ u4
//   sigma2(u)    theta1 = sigma1(u) || u4, theta2 = ~sigma1(u) || u3: (F_theta1(u1) ^ u1) || (F_theta2(u2) ^ u2)
//   belt-hash    state: a 128-bit count of message bits, s (128 bits, zero), h (256 bits, the standard's constant = H(0) .. H(31));
//                per 256-bit block X (the last one zero-padded): s ^= sigma1(X || h), h = sigma2(X || h) -- sigma1 is shared,
//                so three encryptions; the digest is sigma2(count || s || h).
//
// The table is reached through a template parameter `Tab` (anything indexable by an octet): the kernel passes a pointer into
// LDS, the host build (tests/bign_host_shim.cpp) a plain array.
//
// SECRET DATA: what BIGN's verification and signing hash is public -- the OID, the coordinates of the commitment W, which every
// verifier recomputes from the signature, and the digest of the message (the message itself for hash_type 16) -- so k_belt_slots
// and the host shims pass a plain table and the look-ups are indexed by public octets.  DBIGN's nonce generator (ecamd_dbign_nonce.h,
// k_dbign_nonce) is different: its belt-hash runs over the private key and its block cipher is keyed by the result, so there EVERY
// substitution index depends on the private key.  In the library's default mode that kernel gathers from the LDS table like the
// others (the default mode allows secret-dependent addresses: the comb does the same); in secret-scalar mode
// (ecamd_ctx_set_secret_scalars) it passes ScanTab below, whose look-up reads all 64 dwords of the table at addresses that do not
// depend on the index and keeps the wanted octet with compares and shifts.  A Tab whose g() is overloaded (ScanTab) also gets the
// rolled form of the cipher, encrypt_rolled: the scan is long, and eight unrolled rounds of it would not fit the instruction cache.
//
// LDS layout: the table is kept as 256 OCTETS (64 dwords).  For ds_read_u8 the bank of byte address a is (a / 4) mod 32 within a
// 32-lane group and equal dwords broadcast, so a gather meets at most 2 distinct dwords per bank (2 LDS cycles per group at worst);
// a table of 256 words (the substituted octet pre-shifted) would put 8 dwords on each bank.  This follows from the bank rule; the
// conflict counter has not been read (profiles/r12_bign.md).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECB_FN __host__ __device__ __forceinline__
#else
#define ECB_FN inline
#endif

// the substitution H of STB 34.101.31 (row = high nibble, column = low nibble)
#define ECAMD_BELT_H                                                                                                       \
	0xB1, 0x94, 0xBA, 0xC8, 0x0A, 0x08, 0xF5, 0x3B, 0x36, 0x6D, 0x00, 0x8E, 0x58, 0x4A, 0x5D, 0xE4, /* 0 */            \
	0x85, 0x04, 0xFA, 0x9D, 0x1B, 0xB6, 0xC7, 0xAC, 0x25, 0x2E, 0x72, 0xC2, 0x02, 0xFD, 0xCE, 0x0D, /* 1 */            \
	0x5B, 0xE3, 0xD6, 0x12, 0x17, 0xB9, 0x61, 0x81, 0xFE, 0x67, 0x86, 0xAD, 0x71, 0x6B, 0x89, 0x0B, /* 2 */            \
	0x5C, 0xB0, 0xC0, 0xFF, 0x33, 0xC3, 0x56, 0xB8, 0x35, 0xC4, 0x05, 0xAE, 0xD8, 0xE0, 0x7F, 0x99, /* 3 */            \
	0xE1, 0x2B, 0xDC, 0x1A, 0xE2, 0x82, 0x57, 0xEC, 0x70, 0x3F, 0xCC, 0xF0, 0x95, 0xEE, 0x8D, 0xF1, /* 4 */            \
	0xC1, 0xAB, 0x76, 0x38, 0x9F, 0xE6, 0x78, 0xCA, 0xF7, 0xC6, 0xF8, 0x60, 0xD5, 0xBB, 0x9C, 0x4F, /* 5 */            \
	0xF3, 0x3C, 0x65, 0x7B, 0x63, 0x7C, 0x30, 0x6A, 0xDD, 0x4E, 0xA7, 0x79, 0x9E, 0xB2, 0x3D, 0x31, /* 6 */            \
	0x3E, 0x98, 0xB5, 0x6E, 0x27, 0xD3, 0xBC, 0xCF, 0x59, 0x1E, 0x18, 0x1F, 0x4C, 0x5A, 0xB7, 0x93, /* 7 */            \
	0xE9, 0xDE, 0xE7, 0x2C, 0x8F, 0x0C, 0x0F, 0xA6, 0x2D, 0xDB, 0x49, 0xF4, 0x6F, 0x73, 0x96, 0x47, /* 8 */            \
	0x06, 0x07, 0x53, 0x16, 0xED, 0x24, 0x7A, 0x37, 0x39, 0xCB, 0xA3, 0x83, 0x03, 0xA9, 0x8B, 0xF6, /* 9 */            \
	0x92, 0xBD, 0x9B, 0x1C, 0xE5, 0xD1, 0x41, 0x01, 0x54, 0x45, 0xFB, 0xC9, 0x5E, 0x4D, 0x0E, 0xF2, /* A */            \
	0x68, 0x20, 0x80, 0xAA, 0x22, 0x7D, 0x64, 0x2F, 0x26, 0x87, 0xF9, 0x34, 0x90, 0x40, 0x55, 0x11, /* B */            \
	0xBE, 0x32, 0x97, 0x13, 0x43, 0xFC, 0x9A, 0x48, 0xA0, 0x2A, 0x88, 0x5F, 0x19, 0x4B, 0x09, 0xA1, /* C */            \
	0x7E, 0xCD, 0xA4, 0xD0, 0x15, 0x44, 0xAF, 0x8C, 0xA5, 0x84, 0x50, 0xBF, 0x66, 0xD2, 0xE8, 0x8A, /* D */            \
	0xA2, 0xD7, 0x46, 0x52, 0x42, 0xA8, 0xDF, 0xB3, 0x69, 0x74, 0xC5, 0x51, 0xEB, 0x23, 0x29, 0x21, /* E */            \
	0xD4, 0xEF, 0xD9, 0xB4, 0x3A, 0x62, 0x28, 0x75, 0x91, 0x14, 0x10, 0xEA, 0x77, 0x6C, 0xDA, 0x1D  /* F */

namespace ecbelt {

enum : int { DIGEST_BYTES = 32, BLOCK_BYTES = 32 };

template <class Tab> ECB_FN uint32_t g(const Tab &H, uint32_t u, int r)
{
	const uint32_t t = (uint32_t)H[u & 0xffu] | ((uint32_t)H[(u >> 8) & 0xffu] << 8) | ((uint32_t)H[(u >> 16) & 0xffu] << 16) |
			   ((uint32_t)H[u >> 24] << 24);
	return (t << r) | (t >> (32 - r));
}

// The table behind a look-up that forms no address from its index: w points at the 256 octets as 64 dwords (octet i in bits
// 8 (i mod 4) of dword i / 4); every look-up reads all of them in order -- on the device at wave-uniform LDS addresses, which
// broadcast -- and keeps the one wanted with a compare.
struct ScanTab {
	const uint32_t *w;
	ECB_FN uint8_t operator[](uint32_t i) const
	{
		uint32_t t = 0;
#pragma unroll 16
		for (uint32_t j = 0; j < 64u; j++) {
			const uint32_t T = w[j];
			t = (i >> 2) == j ? T : t;
		}
		return (uint8_t)(t >> (8u * (i & 3u)));
	}
};

// G_r(u) over ScanTab: one scan serves the four octets
ECB_FN uint32_t g(const ScanTab &H, uint32_t u, int r)
{
	const uint32_t i0 = u & 0xffu, i1 = (u >> 8) & 0xffu, i2 = (u >> 16) & 0xffu, i3 = u >> 24;
	uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
#pragma unroll 16
	for (uint32_t j = 0; j < 64u; j++) {
		const uint32_t T = H.w[j];
		t0 = (i0 >> 2) == j ? T : t0;
		t1 = (i1 >> 2) == j ? T : t1;
		t2 = (i2 >> 2) == j ? T : t2;
		t3 = (i3 >> 2) == j ? T : t3;
	}
	const uint32_t t = ((t0 >> (8u * (i0 & 3u))) & 0xffu) | (((t1 >> (8u * (i1 & 3u))) & 0xffu) << 8) |
			   (((t2 >> (8u * (i2 & 3u))) & 0xffu) << 16) | (((t3 >> (8u * (i3 & 3u))) & 0xffu) << 24);
	return (t << r) | (t >> (32 - r));
}

// x <- F_key(x) with the eight rounds as a loop: the round keys K_(7i-6) .. K_(7i) are key[0 .. 6] of a copy that is rotated by
// seven places (= back by one) after each round, so every index is still a constant.  The same bytes as encrypt below.
template <class Tab> ECB_FN void encrypt_rolled(const Tab &H, const uint32_t (&key)[8], uint32_t (&x)[4])
{
	uint32_t a = x[0], b = x[1], c = x[2], d = x[3];
	uint32_t k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3], k4 = key[4], k5 = key[5], k6 = key[6], k7 = key[7];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (uint32_t i = 1; i <= 8; i++) {
		b ^= g(H, a + k0, 5);
		c ^= g(H, d + k1, 21);
		a -= g(H, b + k2, 13);
		const uint32_t e = g(H, b + c + k3, 21) ^ i;
		b += e;
		c -= e;
		d += g(H, c + k4, 13);
		b ^= g(H, a + k5, 21);
		c ^= g(H, d + k6, 5);
		const uint32_t na = b, nb = d, nc = a, nd = c;
		a = na;
		b = nb;
		c = nc;
		d = nd;
		const uint32_t last = k7;
		k7 = k6;
		k6 = k5;
		k5 = k4;
		k4 = k3;
		k3 = k2;
		k2 = k1;
		k1 = k0;
		k0 = last;
	}
	x[0] = b;
	x[1] = d;
	x[2] = a;
	x[3] = c;
}

// x <- F_key(x).  Fully unrolled, so that every index into key[] is a constant (the arrays stay in registers).
template <class Tab> ECB_FN void encrypt(const Tab &H, const uint32_t (&key)[8], uint32_t (&x)[4])
{
	uint32_t a = x[0], b = x[1], c = x[2], d = x[3];
#pragma unroll
	for (uint32_t i = 1; i <= 8; i++) {
		const uint32_t o = 7u * (i - 1u);   // K_(7i-6+t) = theta_((o + t) mod 8 + 1)
		b ^= g(H, a + key[o & 7u], 5);
		c ^= g(H, d + key[(o + 1u) & 7u], 21);
		a -= g(H, b + key[(o + 2u) & 7u], 13);
		const uint32_t e = g(H, b + c + key[(o + 3u) & 7u], 21) ^ i;
		b += e;
		c -= e;
		d += g(H, c + key[(o + 4u) & 7u], 13);
		b ^= g(H, a + key[(o + 5u) & 7u], 21);
		c ^= g(H, d + key[(o + 6u) & 7u], 5);
		// a <-> b, c <-> d, b <-> c
		const uint32_t na = b, nb = d, nc = a, nd = c;
		a = na;
		b = nb;
		c = nc;
		d = nd;
	}
	x[0] = b;
	x[1] = d;
	x[2] = a;
	x[3] = c;
}

ECB_FN void encrypt(const ScanTab &H, const uint32_t (&key)[8], uint32_t (&x)[4]) { encrypt_rolled(H, key, x); }

// One step of the iteration on a 256-bit block X: t = sigma1(X || h) is XORed into s, and h <- sigma2(X || h).
template <class Tab> ECB_FN void step(const Tab &H, const uint32_t (&X)[8], uint32_t (&s)[4], uint32_t (&h)[8])
{
	uint32_t t[4], key[8], blk[4];
#pragma unroll
	for (int j = 0; j < 4; j++) {
		t[j] = h[j] ^ h[4 + j];
	}
#pragma unroll
	for (int j = 0; j < 4; j++) {
		blk[j] = t[j];
	}
	encrypt(H, X, blk);
#pragma unroll
	for (int j = 0; j < 4; j++) {
		t[j] ^= blk[j];   // sigma1(X || h)
		s[j] ^= t[j];
	}
	// first half: F_(t || h2)(X1) ^ X1
#pragma unroll
	for (int j = 0; j < 4; j++) {
		key[j] = t[j];
		key[4 + j] = h[4 + j];
		blk[j] = X[j];
	}
	encrypt(H, key, blk);
	uint32_t n1[4];
#pragma unroll
	for (int j = 0; j < 4; j++) {
		n1[j] = blk[j] ^ X[j];
	}
	// second half: F_(~t || h1)(X2) ^ X2
#pragma unroll
	for (int j = 0; j < 4; j++) {
		key[j] = ~t[j];
		key[4 + j] = h[j];
		blk[j] = X[4 + j];
	}
	encrypt(H, key, blk);
#pragma unroll
	for (int j = 0; j < 4; j++) {
		h[j] = n1[j];
		h[4 + j] = blk[j] ^ X[4 + j];
	}
}

// word j of the zero-padded message: msg holds the message as little-endian words (the buffer is readable up to the word
// that holds the last byte)
ECB_FN uint32_t padded_word(const uint32_t *msg, uint32_t len, uint32_t j)
{
	const uint32_t pos = 4u * j;
	if (pos >= len) {
		return 0u;
	}
	const uint32_t w = msg[j], rem = len - pos;
	return rem >= 4u ? w : (w & (0xffffffffu >> (8u * (4u - rem))));
}

// BelT-hash of len bytes (len < 2^29); the digest as eight little-endian words
template <class Tab> ECB_FN void hash_words(const Tab &H, const uint32_t *msg, uint32_t len, uint32_t (&out)[8])
{
	const uint8_t iv[32] = {0xB1, 0x94, 0xBA, 0xC8, 0x0A, 0x08, 0xF5, 0x3B, 0x36, 0x6D, 0x00, 0x8E, 0x58, 0x4A, 0x5D, 0xE4,
				0x85, 0x04, 0xFA, 0x9D, 0x1B, 0xB6, 0xC7, 0xAC, 0x25, 0x2E, 0x72, 0xC2, 0x02, 0xFD, 0xCE, 0x0D};
	uint32_t s[4] = {0u, 0u, 0u, 0u}, h[8], X[8];
#pragma unroll
	for (int j = 0; j < 8; j++) {
		h[j] = (uint32_t)iv[4 * j] | ((uint32_t)iv[4 * j + 1] << 8) | ((uint32_t)iv[4 * j + 2] << 16) | ((uint32_t)iv[4 * j + 3] << 24);
	}
	const uint32_t nblocks = (len + 31u) / 32u;
	// iteration nblocks is the finalisation: sigma2((count || s) || h); what its step adds to s is not read any more
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (uint32_t b = 0; b <= nblocks; b++) {
		if (b < nblocks) {
#pragma unroll
			for (uint32_t j = 0; j < 8; j++) {
				X[j] = padded_word(msg, len, 8u * b + j);
			}
		} else {
			X[0] = len << 3;   // the count of bits, 128 bits little-endian
			X[1] = len >> 29;
			X[2] = 0u;
			X[3] = 0u;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				X[4 + j] = s[j];
			}
		}
		step(H, X, s, h);
	}
#pragma unroll
	for (int j = 0; j < 8; j++) {
		out[j] = h[j];
	}
}

}  // namespace ecbelt
