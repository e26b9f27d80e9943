// libecc_amd/csrc/ecamd_dbign_nonce.h -- the nonce of deterministic BIGN (STB 34.101.45 section 6.3.3) per item, as the reference runs
// it (__bign_determinitic_nonce, sig/bign_common.c:200-342), its non-standard choices included.  Compiles for the device
// (ecamd_detnonce.hip: one item per lane) and for the host (tests/det_nonce_host_shim.cpp).
//
//   qlen    octets of the generator's order q, qbits its bits, l = qlen / 2 (integer division: BIGN_S0_LEN)
//   theta   belt-hash(oid || the first 2 l octets of the private key written to qlen octets and byte-reversed || t); for an odd
//           qlen (29, 66) the top octet of d is not hashed
//   r       the digest h of hlen octets, zero-padded; n = hlen / 16, raised to 2 when it is 0 or 1 (SHA-224: 28 octets, two blocks)
//   i = 1, 2, ...:  s = r_1 ^ .. ^ r_(n-1);  r_1 .. r_(n-2) <- r_2 .. r_(n-1);  r_(n-1) <- F_theta(s) ^ r_n ^ <i>_128 (i as a
//           little-endian u32 in the first four octets);  r_n <- s
//   k       after each iteration: qlen < 16 n: the first qlen octets of r as a little-endian number, bits from qbits up cleared;
//           otherwise the first 16 n octets (the reference's "small hash, big order" branch)
//   accept  when i >= 2 n and 0 < k < q.  The reference goes on until i wraps; here MAX_REJECTS candidates rejected at i >= 2 n end
//           the item with status 1 and a zero nonce (the cap and the reasoning of ecamd_rfc6979.h: no libecc order rejects more than
//           about half)
//
// r is kept as 32 little-endian words, so its first words ARE the limbs of k.  The number of blocks n is a run-time value of the call
// (the same for every lane); the moves between blocks are selects on it, so every index into r is a constant and r stays in registers.
// belt-hash's input (at most 64 + 66 + 64 octets) is laid out once as little-endian words in a per-item word buffer `tb` of IN_WORDS
// words with stride `ts` (the kernel: LDS, word w of lane l at [w * 64 + l]; the host: a plain array, ts = 1) and zeroed before the
// function returns.
//
// SECRET DATA: the private key, theta, r after the first iteration and k.  Every BelT substitution here is indexed by them: see the
// note in ecamd_belt.h and pass ScanTab where no address may depend on a secret.  The only secret-dependent branch is the standard's
// own acceptance test.
#pragma once
#include <stdint.h>
#include "ecamd_belt.h"
#include "ecamd_rfc6979.h"   // ecrfc::sub_limbs, ecrfc::limbs_to_be, ECR_FN

namespace ecdbign {

typedef uint8_t u8;
typedef uint32_t u32;

enum : int {
	NL = ecrfc::NL,
	MAX_QLEN = ecrfc::MAX_QLEN,
	MAX_OID = 64,
	MAX_T = 64,
	MAX_DIGEST = 128,
	MAX_BLOCKS = MAX_DIGEST / 16,
	IN_WORDS = 56,        // belt-hash's input: 64 + 66 + 64 octets at most, seven blocks of eight words
	MAX_REJECTS = 1000
};

// the blocks of r the generator works on
ECR_FN u32 blocks(u32 hlen) { return hlen / 16u <= 1u ? 2u : hlen / 16u; }

ECR_FN void tb_or_le(u32 *tb, int ts, u32 pos, u32 byte) { tb[(pos >> 2) * ts] |= byte << (8u * (pos & 3u)); }
ECR_FN void tb_zero(u32 *tb, int ts)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (int w = 0; w < IN_WORDS; w++) {
		tb[w * ts] = 0;
	}
}

// theta: eight little-endian words
template <class Tab>
ECR_FN void theta(const Tab &H, const u8 *priv, u32 qlen, const u8 *oid, u32 oid_len, const u8 *t, u32 t_len, u32 *tb, int ts, uint32_t (&th)[8])
{
	const u32 l2 = 2u * (qlen / 2u), len = oid_len + l2 + t_len;
	tb_zero(tb, ts);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < oid_len; b++) {
		tb_or_le(tb, ts, b, oid[b]);
	}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < l2; b++) {
		tb_or_le(tb, ts, oid_len + b, priv[qlen - 1u - b]);
	}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < t_len; b++) {
		tb_or_le(tb, ts, oid_len + l2 + b, t[b]);
	}
	// belt-hash as ecbelt::hash_words runs it, the words read from the lane's column (zero behind the input)
	const u8 iv[32] = {0xB1, 0x94, 0xBA, 0xC8, 0x0A, 0x08, 0xF5, 0x3B, 0x36, 0x6D, 0x00, 0x8E, 0x58, 0x4A, 0x5D, 0xE4,
			   0x85, 0x04, 0xFA, 0x9D, 0x1B, 0xB6, 0xC7, 0xAC, 0x25, 0x2E, 0x72, 0xC2, 0x02, 0xFD, 0xCE, 0x0D};
	uint32_t s[4] = {0u, 0u, 0u, 0u}, X[8];
#pragma unroll
	for (int j = 0; j < 8; j++) {
		th[j] = (u32)iv[4 * j] | ((u32)iv[4 * j + 1] << 8) | ((u32)iv[4 * j + 2] << 16) | ((u32)iv[4 * j + 3] << 24);
	}
	const u32 nblocks = (len + 31u) / 32u;   // at most IN_WORDS / 8
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b <= nblocks; b++) {
		if (b < nblocks) {
#pragma unroll
			for (u32 j = 0; j < 8; j++) {
				X[j] = tb[(8u * b + j) * ts];
			}
		} else {
			X[0] = len << 3;
			X[1] = 0u;
			X[2] = 0u;
			X[3] = 0u;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				X[4 + j] = s[j];
			}
		}
		ecbelt::step(H, X, s, th);
	}
	tb_zero(tb, ts);
}

// The generator.  priv: qlen octets big-endian; dig: hlen <= MAX_DIGEST octets; oid, t: at most MAX_OID / MAX_T octets; q: NL
// little-endian limbs; tb / ts: the word buffer (IN_WORDS words).  k: NL limbs out.  Returns 0, or 1 with k = 0 when MAX_REJECTS
// candidates were rejected; *rejects: the candidates rejected at i >= 2 n.
template <class Tab>
ECR_FN int nonce(const Tab &H, const u8 *priv, const u8 *dig, u32 hlen, const u8 *oid, u32 oid_len, const u8 *t, u32 t_len, const u32 *q,
		 u32 qbits, u32 *tb, int ts, u32 *k, u32 *rejects)
{
	const u32 qlen = (qbits + 7u) / 8u;
	uint32_t th[8];
	theta(H, priv, qlen, oid, oid_len, t, t_len, tb, ts, th);
	u32 r[4 * MAX_BLOCKS];
#pragma unroll
	for (int w = 0; w < 4 * MAX_BLOCKS; w++) {
		u32 v = 0;
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const u32 pos = 4u * (u32)w + (u32)b;
			if (pos < hlen) {
				v |= (u32)dig[pos] << (8 * b);
			}
		}
		r[w] = v;
	}
	const u32 n = blocks(hlen);
	const bool whole = qlen >= 16u * n;      // k is all of the n blocks
	u32 rej = 0;
	int status = 1;
	for (u32 i = 1;; i++) {
		uint32_t s[4] = {0u, 0u, 0u, 0u}, rn[4] = {0u, 0u, 0u, 0u}, blk[4];
#pragma unroll
		for (int j = 0; j < MAX_BLOCKS; j++) {
#pragma unroll
			for (int z = 0; z < 4; z++) {
				s[z] ^= (u32)j + 1u < n ? r[4 * j + z] : 0u;
				rn[z] = (u32)j + 1u == n ? r[4 * j + z] : rn[z];
			}
		}
#pragma unroll
		for (int z = 0; z < 4; z++) {
			blk[z] = s[z];
		}
		ecbelt::encrypt(H, th, blk);
#pragma unroll
		for (int z = 0; z < 4; z++) {
			blk[z] ^= rn[z];
		}
		blk[0] ^= i;
		// ascending: block j + 1 is read before it is written
#pragma unroll
		for (int j = 0; j < MAX_BLOCKS; j++) {
#pragma unroll
			for (int z = 0; z < 4; z++) {
				const u32 next = j + 1 < MAX_BLOCKS ? r[4 * (j + 1 < MAX_BLOCKS ? j + 1 : 0) + z] : 0u;
				r[4 * j + z] = (u32)j + 2u < n ? next : (u32)j + 2u == n ? blk[z] : (u32)j + 1u == n ? s[z] : r[4 * j + z];
			}
		}
		if (i < 2u * n) {
			continue;
		}
		u32 any = 0;
#pragma unroll
		for (int l = 0; l < NL; l++) {
			u32 v = (u32)l < 4u * n ? r[l] : 0u;
			if (!whole) {
				const u32 lo = 32u * (u32)l;
				v = lo >= qbits ? 0u : (qbits - lo >= 32u ? v : v & ((1u << (qbits - lo)) - 1u));
			}
			k[l] = v;
			any |= v;
		}
		u32 d[NL];
		if (any != 0u && ecrfc::sub_limbs(k, q, d)) {
			status = 0;
			break;
		}
		if (++rej >= (u32)MAX_REJECTS) {
#pragma unroll
			for (int l = 0; l < NL; l++) {
				k[l] = 0;
			}
			break;
		}
	}
	*rejects = rej;
	return status;
}

}  // namespace ecdbign
