// libecc_amd/csrc/ecamd_bip0340_nonce.h -- the semi-deterministic nonce of BIP0340 signing per item, as the reference runs it
// (_bip0340_sign, sig/bip0340.c:213-294).  Compiles for the device (ecamd_detnonce.hip: one item per lane) and for the host
// (tests/det_nonce_host_shim.cpp).
//
//   H       the call's hash: SHA-224, SHA-256, SHA-384 or SHA-512 (the reference does not fix it to SHA-256), hsize its octets
//   Y       the key pair's public half, affine; d = x, or q - x when Y.y is odd; x = 0 and x >= q fail (:229-232)
//   mask    H(H(tag_aux) || H(tag_aux) || aux), aux as qlen big-endian octets (the value libecc draws below 2^(8 qlen))
//   t       qlen > hsize: the qlen octets of d with the first hsize XORed with mask; otherwise mask with its first qlen octets
//           XORed with d -- in both cases (d || 0 ..) ^ (mask || 0 ..) over max(qlen, hsize) octets
//   k       OS2I(H(H(tag_nonce) || H(tag_nonce) || t || Y.x || m)) mod q, over the whole digest; k = 0 fails (:292-294)
//
// The two tag hashes are the same for every item: the host computes them once per call (tag_hash below) and hands them over as
// the hash's own big-endian words.  The part of a hash input in front of the message -- the two tag hashes, then aux or t || Y.x, at
// most 128 + 66 + 66 octets -- is laid out as big-endian 32-bit words in a per-item word buffer `tb` of PRE_WORDS words with stride
// `ts` (the kernel: LDS, word w of lane l at [w * 64 + l]; the host: a plain array, ts = 1); 2 hsize is a multiple of 8, so the
// buffer's words are the hash's words.  The message is streamed from where it lies.  The buffer is zeroed before the function returns.
//
// SECRET DATA: x, d, t, the nonce hash's state and k.  No table is indexed by any of them and no branch depends on them except the
// reference's own failures (x out of range, k = 0); the reduction mod q is a fixed number of conditional subtractions by selects.
#pragma once
#include <stdint.h>
#include "ecamd_rfc6979.h"   // SHA-2 compression, limbs, ECR_FN

namespace ecbip {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum : int {
	NL = ecrfc::NL,
	MAX_QLEN = ecrfc::MAX_QLEN,
	MAX_CLEN = 66,
	PRE_WORDS = 66,       // 2 * 64 + 66 + 66 octets, rounded up to a whole 64-bit word
	TAG_WORDS = 8
};

// what ec_schnorr_sign_batch defines as the fixed fields of a BIP0340 slot: H(tag) || H(tag) || <r> || <Y.x>
ECR_FN u32 fixed_len(u32 hsize, u32 clen) { return 2u * hsize + 2u * clen; }
// a slot (u32 length, then the hash input) holds its fixed fields and fits the stride
ECR_FN bool slot_ok(u32 len, u32 stride, u32 hsize, u32 clen) { return stride >= 4u && len <= stride - 4u && len >= fixed_len(hsize, clen); }

ECR_FN void tb_or(u32 *tb, int ts, u32 pos, u32 byte) { tb[(pos >> 2) * ts] |= byte << (8u * (3u - (pos & 3u))); }
ECR_FN void tb_xor(u32 *tb, int ts, u32 pos, u32 byte) { tb[(pos >> 2) * ts] ^= byte << (8u * (3u - (pos & 3u))); }
ECR_FN void tb_zero(u32 *tb, int ts)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (int w = 0; w < PRE_WORDS; w++) {
		tb[w * ts] = 0;
	}
}

// the four octets at offset g (a multiple of 4) of  <plen octets of tb> || <mlen octets at msg> || 80 || 00 ..  as a big-endian word
ECR_FN u32 stream_word(const u32 *tb, int ts, u32 plen, const u8 *msg, u32 mlen, u32 g)
{
	const u32 total = plen + mlen;
	u32 v = 0;
	if (g < plen) {
		v = tb[(g >> 2) * ts];        // zero behind plen inside its last word
	}
	if (g + 4u > plen && g < total) {
		if (g >= plen && g + 4u <= total) {
			u32 w;
			__builtin_memcpy(&w, msg + (g - plen), 4);
			v = __builtin_bswap32(w);
		} else {
#pragma unroll
			for (u32 j = 0; j < 4u; j++) {
				const u32 pos = g + j - plen;   // below plen this wraps and fails the compare
				const u32 byte = pos < mlen ? msg[pos] : 0u;
				v |= byte << (24u - 8u * j);
			}
		}
	}
	if ((total & ~3u) == g) {
		v |= 0x80u << (24u - 8u * (total & 3u));
	}
	return v;
}

// st = H(<plen octets of tb> || <mlen octets at msg>): the eight state words
template <int ALG, typename KT>
ECR_FN void hash_pre_msg(const u32 *tb, int ts, u32 plen, const u8 *msg, u32 mlen, typename ecrfc::Alg<ALG>::W *st, KT Kt)
{
	typedef typename ecrfc::Alg<ALG>::W W;
	constexpr u32 BLOCK = ecrfc::Alg<ALG>::BLOCK;
	const u32 total = plen + mlen;
	const u32 nb = (total + 1u + (u32)ecrfc::Alg<ALG>::LENF + BLOCK - 1u) / BLOCK;
	ecrfc::iv<ALG>(st);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < nb; b++) {
		W w[16];
#pragma unroll
		for (int t = 0; t < 16; t++) {
			const u32 g = BLOCK * b + (u32)sizeof(W) * (u32)t;
			W v;
			if (sizeof(W) == 8) {
				v = (W)(((u64)stream_word(tb, ts, plen, msg, mlen, g) << 32) | stream_word(tb, ts, plen, msg, mlen, g + 4u));
			} else {
				v = (W)stream_word(tb, ts, plen, msg, mlen, g);
			}
			if (g == BLOCK * nb - (u32)sizeof(W)) {
				v = (W)(8u * total);      // the length field: the words in front of this one are zero
			}
			w[t] = v;
		}
		ecrfc::compress<ALG>(st, w, Kt);
	}
}

// H(tag) for a tag of at most 55 octets, as the hash's words (one block; the host runs this once per call)
template <int ALG, typename KT> ECR_FN void tag_hash(const char *tag, u32 len, typename ecrfc::Alg<ALG>::W *out, KT Kt)
{
	u32 tb[PRE_WORDS];
	tb_zero(tb, 1);
	for (u32 i = 0; i < len; i++) {
		tb_or(tb, 1, i, (u8)tag[i]);
	}
	hash_pre_msg<ALG>(tb, 1, len, (const u8 *)0, 0u, out, Kt);
}

// the tag hash twice at the head of the buffer
template <int ALG> ECR_FN void put_tags(u32 *tb, int ts, const typename ecrfc::Alg<ALG>::W *tag)
{
	typedef typename ecrfc::Alg<ALG>::W W;
	constexpr int VW = ecrfc::Hmac<ALG>::VW;
#pragma unroll
	for (int c = 0; c < 2; c++) {
#pragma unroll
		for (int t = 0; t < VW; t++) {
			if (sizeof(W) == 8) {
				tb[(2 * (c * VW + t)) * ts] = (u32)((u64)tag[t] >> 32);
				tb[(2 * (c * VW + t) + 1) * ts] = (u32)tag[t];
			} else {
				tb[(c * VW + t) * ts] = (u32)tag[t];
			}
		}
	}
}

// The generator.  priv, aux: qlen octets big-endian; Y: X || Y, clen octets each; tag_aux, tag_nonce: the tag hashes as words;
// msg / mlen: the message; q: NL little-endian limbs; tb / ts: the word buffer (PRE_WORDS words).  k: NL limbs out.  Returns 0, or
// 1 with k = 0 where the reference fails: x = 0, x >= q, k = 0.
template <int ALG, typename KT>
ECR_FN int nonce(const u8 *priv, const u8 *Y, u32 clen, const u8 *aux, const typename ecrfc::Alg<ALG>::W *tag_aux,
		 const typename ecrfc::Alg<ALG>::W *tag_nonce, const u8 *msg, u32 mlen, const u32 *q, u32 qbits, u32 *tb, int ts, KT Kt, u32 *k)
{
	typedef typename ecrfc::Alg<ALG>::W W;
	constexpr int VW = ecrfc::Hmac<ALG>::VW, HS = ecrfc::Alg<ALG>::HSIZE, WB = (int)sizeof(W);
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
	// mask = H(tag_aux || tag_aux || aux)
	W st[8];
	tb_zero(tb, ts);
	put_tags<ALG>(tb, ts, tag_aux);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 i = 0; i < qlen; i++) {
		tb_or(tb, ts, 2u * HS + i, aux[i]);
	}
	hash_pre_msg<ALG>(tb, ts, 2u * HS + qlen, (const u8 *)0, 0u, st, Kt);
	// t || Y.x behind the nonce tag
	const u32 tl = qlen > (u32)HS ? qlen : (u32)HS;
	tb_zero(tb, ts);
	put_tags<ALG>(tb, ts, tag_nonce);
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
	for (int t = 0; t < VW; t++) {
#pragma unroll
		for (int j = 0; j < WB; j++) {
			tb_xor(tb, ts, 2u * HS + (u32)(WB * t + j), (u32)(st[t] >> (8 * (WB - 1 - j))) & 0xffu);
		}
	}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 i = 0; i < clen; i++) {
		tb_or(tb, ts, 2u * HS + tl + i, Y[i]);
	}
	hash_pre_msg<ALG>(tb, ts, 2u * HS + tl + clen, msg, mlen, st, Kt);
	tb_zero(tb, ts);
	// k = digest mod q: bit by bit from the top, k <- 2 k + bit, minus q when that is not below q (k < q < 2^528, so 2 k + 1 fits)
#pragma unroll
	for (int l = 0; l < NL; l++) {
		k[l] = 0;
	}
#pragma unroll
	for (int t = 0; t < VW; t++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
		for (int j = 8 * WB - 1; j >= 0; j--) {
			u32 carry = (u32)(st[t] >> j) & 1u;
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

}  // namespace ecbip
