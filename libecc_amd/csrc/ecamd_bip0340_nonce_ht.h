// libecc_amd/csrc/ecamd_bip0340_nonce_ht.h -- the semi-deterministic nonce of BIP0340 signing per item (_bip0340_sign,
// sig/bip0340.c:213-294) over ANY hash of echm::Hash<ID> (ecamd_hmac.h): ecamd_bip0340_nonce.h's generator restated over the hash
// trait.  Compiles for the device (ecamd_bip0340_nonce_ht.hip: one item per lane) and for the host
// (tests/bip0340_nonce_ht_host_shim.cpp; ecamd_host_sigfam.cpp computes the two tag hashes of a call with tag_hash below).
//
//   H       the call's hash, HS = H::HSIZE its octets (20 with RIPEMD-160 .. 64), BLOCK 64 .. 144
//   Y       the key pair's public half, affine; d = x, or q - x when Y.y is odd; x = 0 and x >= q fail (:229-232)
//   mask    H(H(tag_aux) || H(tag_aux) || aux), aux as qlen big-endian octets
//   t       (d || 0 ..) ^ (mask || 0 ..) over tl = max(qlen, HS) octets (HS = 20 beside qlen = 66 is the widest gap)
//   k       OS2I(H(H(tag_nonce) || H(tag_nonce) || t || Y.x || m)) mod q, over the whole digest; k = 0 fails (:292-294)
//
// The hash input is a FUNCTION of (block, word) in memory order, as the trait wants it: the part in front of the message -- the
// two tag hashes, then aux or t || Y.x, at most 2 * 64 + 66 + 66 octets -- lies in a per-item word buffer `tb` of PRE_WORDS words with
// stride `ts` (the kernel: LDS, word w of lane l at [w * 64 + l]; the host: a plain array, ts = 1), four octets per word packed
// little-endian; the message is streamed from where it lies.  No midstate of the two tag hashes is kept: 2 HS octets fill whole blocks
// for SHA-2, SM3 and Streebog-512 only, so every hash absorbs the whole prefix from the buffer, as ecamd_hmac.h absorbs its key block.
// The two hashes of an item are two passes of ONE loop around ONE call of H::hash, so a kernel holds one copy of its compression
// function or permutation.  The buffer is zeroed before the function returns.
//
// SECRET DATA: x, d, t, the nonce hash's state and k.  Every address into tb depends on qlen, clen, HS and the lane only; no branch
// depends on a secret except the reference's own failures (x out of range, k = 0); the reduction mod q is a fixed number of
// conditional subtractions by selects.  With Streebog (13, 14) the hash itself looks its table up by state octets that depend on t:
// the entry points refuse those two in secret-scalar mode (include/libecc_amd.h).
#pragma once
#include <stdint.h>
#include "ecamd_hmac.h"

namespace ecbipht {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum : int {
	NL = ecrfc::NL,
	MAX_QLEN = ecrfc::MAX_QLEN,
	MAX_CLEN = 66,
	PRE_WORDS = 66,       // 2 * 64 + 66 + 66 = 260 octets: 65 words, and one that stays zero
	TAG_WORDS = 16        // a tag hash as words in memory order: HS / 4 <= 16
};

// what ec_schnorr_sign_batch defines as the fixed fields of a BIP0340 slot: H(tag) || H(tag) || <r> || <Y.x>
EHM_FN u32 fixed_len(u32 hsize, u32 clen) { return 2u * hsize + 2u * clen; }
// a slot (u32 length, then the hash input) holds its fixed fields and fits the stride
EHM_FN bool slot_ok(u32 len, u32 stride, u32 hsize, u32 clen) { return stride >= 4u && len <= stride - 4u && len >= fixed_len(hsize, clen); }

// octet `pos` of the word buffer (memory order)
EHM_FN void tb_or(u32 *tb, int ts, u32 pos, u32 byte) { tb[(pos >> 2) * ts] |= byte << (8u * (pos & 3u)); }
EHM_FN void tb_zero(u32 *tb, int ts)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (int w = 0; w < PRE_WORDS; w++) {
		tb[w * ts] = 0;
	}
}

// the four octets at offset g (a multiple of 4) of  <plen octets of tb> || <mlen octets at msg>  in memory order, zero behind the end
EHM_FN u32 stream_word(const u32 *tb, int ts, u32 plen, const u8 *msg, u32 mlen, u32 g)
{
	const u32 total = plen + mlen;
	u32 v = 0;
	if (g < plen) {
		v = tb[(g >> 2) * ts];        // zero behind plen inside its last word; plen <= 260, so g >> 2 < PRE_WORDS
	}
	if (g + 4u > plen && g < total) {
		if (g >= plen && g + 4u <= total) {
			__builtin_memcpy(&v, msg + (g - plen), 4);
		} else {
#pragma unroll
			for (u32 j = 0; j < 4u; j++) {
				const u32 pos = g + j - plen;   // below plen this wraps and fails the compare
				const u32 byte = pos < mlen ? msg[pos] : 0u;
				v |= byte << (8u * j);
			}
		}
	}
	return v;
}

// H(tag) as H::DW words in memory order (the host runs this once per call and tag)
template <class H, class Env> EHM_FN void tag_hash(const Env &env, const char *tag, u32 len, u32 *out)
{
	u32 tb[PRE_WORDS];
	tb_zero(tb, 1);
	for (u32 i = 0; i < len; i++) {
		tb_or(tb, 1, i, (u8)tag[i]);
	}
	H::hash(env, [&](u32 b, u32 t) -> u32 { return stream_word(tb, 1, len, (const u8 *)0, 0u, 4u * (b * (u32)H::BW + t)); }, len, out);
}

// The generator.  priv, aux: qlen octets big-endian; Y: X || Y, clen octets each; tag_aux, tag_nonce: the tag hashes as H::DW words;
// msg / mlen: the message; q: NL little-endian limbs; tb / ts: the word buffer (PRE_WORDS words).  k: NL limbs out.  Returns 0, or
// 1 with k = 0 where the reference fails: x = 0, x >= q, k = 0.
template <class H, class Env>
EHM_FN int nonce(const Env &env, const u8 *priv, const u8 *Y, u32 clen, const u8 *aux, const u32 *tag_aux, const u32 *tag_nonce, const u8 *msg,
		 u32 mlen, const u32 *q, u32 qbits, u32 *tb, int ts, u32 *k)
{
	constexpr u32 DW = (u32)H::DW, BW = (u32)H::BW, HS = (u32)H::HSIZE;
	static_assert(HS % 4u == 0u && DW <= (u32)TAG_WORDS, "a tag hash is whole words");
	const u32 qlen = (qbits + 7u) / 8u;
	u32 x[NL], d[NL], any = 0;
#pragma unroll
	for (int l = 0; l < NL; l++) {
		x[l] = 0;
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const u32 bp = 4u * (u32)l + (u32)b;
			if (bp < qlen) {
				x[l] |= (u32)priv[qlen - 1u - bp] << (8 * b);
			}
		}
		any |= x[l];
	}
	const bool x_ok = ecrfc::sub_limbs(x, q, d) != 0u && any != 0u;   // 0 < x < q
	ecrfc::sub_limbs(q, x, d);
	const bool y_odd = (Y[2u * clen - 1u] & 1u) != 0u;
#pragma unroll
	for (int l = 0; l < NL; l++) {
		d[l] = y_odd ? d[l] : x[l];
	}
	const u32 tl = qlen > HS ? qlen : HS;
	u32 dg[DW];
#pragma unroll
	for (u32 t = 0; t < DW; t++) {
		dg[t] = 0;
	}
	// pass 0: mask = H(tag_aux || tag_aux || aux); pass 1: H(tag_nonce || tag_nonce || t || Y.x || m)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 pass = 0; pass < 2u; pass++) {
		tb_zero(tb, ts);
#pragma unroll
		for (u32 t = 0; t < DW; t++) {
			const u32 w = pass == 0u ? tag_aux[t] : tag_nonce[t];
			tb[t * ts] = w;
			tb[(DW + t) * ts] = w;
		}
		if (pass == 0u) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
			for (u32 i = 0; i < qlen; i++) {
				tb_or(tb, ts, 2u * HS + i, aux[i]);
			}
		} else {
#pragma unroll
			for (int l = 0; l < NL; l++) {
#pragma unroll
				for (int b = 0; b < 4; b++) {
					const u32 bp = 4u * (u32)l + (u32)b;
					if (bp < qlen) {
						tb_or(tb, ts, 2u * HS + (qlen - 1u - bp), (d[l] >> (8 * b)) & 0xffu);
					}
				}
			}
#pragma unroll
			for (u32 t = 0; t < DW; t++) {
				tb[(2u * DW + t) * ts] ^= dg[t];   // 2 HS is a multiple of 4: the mask's words are the buffer's
			}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
			for (u32 i = 0; i < clen; i++) {
				tb_or(tb, ts, 2u * HS + tl + i, Y[i]);
			}
		}
		const u32 plen = 2u * HS + (pass == 0u ? qlen : tl + clen), ml = pass == 0u ? 0u : mlen;
		u32 out[DW];
		H::hash(env, [&](u32 b, u32 t) -> u32 { return stream_word(tb, ts, plen, msg, ml, 4u * (b * BW + t)); }, plen + ml, out);
#pragma unroll
		for (u32 t = 0; t < DW; t++) {
			dg[t] = out[t];
		}
	}
	tb_zero(tb, ts);
	// k = digest mod q: bit by bit from the top, k <- 2 k + bit, minus q when that is not below q (k < q < 2^528, so 2 k + 1 fits)
#pragma unroll
	for (int l = 0; l < NL; l++) {
		k[l] = 0;
	}
#pragma unroll
	for (u32 t = 0; t < DW; t++) {
		const u32 w = echm::bswap(dg[t]);   // the digest's octets 4 t .. 4 t + 3, the first on top
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
		for (int j = 31; j >= 0; j--) {
			u32 carry = (w >> j) & 1u;
#pragma unroll
			for (int l = 0; l < NL; l++) {
				const u32 v = k[l];
				k[l] = (v << 1) | carry;
				carry = v >> 31;
			}
			u32 e[NL];
			const u32 below = ecrfc::sub_limbs(k, q, e);
#pragma unroll
			for (int l = 0; l < NL; l++) {
				k[l] = below ? k[l] : e[l];
			}
		}
	}
	any = 0;
#pragma unroll
	for (int l = 0; l < NL; l++) {
		any |= k[l];
	}
	const bool ok = x_ok && any != 0u;
#pragma unroll
	for (int l = 0; l < NL; l++) {
		k[l] = ok ? k[l] : 0u;
	}
	return ok ? 0 : 1;
}

}  // namespace ecbipht
