// libecc_amd/csrc/ecamd_sm2z.h -- SM2's Z = H(ENTL || ID || a || b || xG || yG || xY || yY) per item (GB/T 32918.2, sig/sm2.c:121-205
// of libecc), for the message-level SM2 entry points: H is SM3 (ecamd_sm3.h) or SHA-224 / 256 / 384 / 512 (the compression of
// ecamd_rfc6979.h).  Compiles for the device (k_sm2_z, ecamd_hash2.hip) and for the host (ecamd_host_sigfam.cpp, tests/sighash2_host_shim.cpp).
//
// Everything but the key is the same for every item of a call, so the host absorbs the whole blocks of the PREFIX
// ENTL || ID || a || b || xG || yG once (prefix_init) and hands the kernel the midstate and the octets left over (less than one
// block) in a Prefix, a kernel argument; an item then hashes  tail || xY || yY  from the midstate: two compressions for SM3 on a
// 256-bit curve where the whole input takes four or more.
//
//   ENTL    the bit length of ID as two octets, big-endian; ID has at most MAX_ID octets here (libecc allows 8191)
//   a .. yG the curve's coefficients and generator, BYTECEIL(|p|) octets each, big-endian
//   xY, yY  the octets of the affine key as the caller gave them (an imported key exports the same octets; one that does not
//           import is rejected by the caller whatever its Z)
//
// SECRET DATA: none; every input is public.
#pragma once
#include <stdint.h>
#include <string.h>
#include "ecamd_sm3.h"
#include "ecamd_rfc6979.h"

namespace ecsm2z {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum : int { MAX_ID = 1024, MAX_CLEN = 66, SM3 = 11 };

struct Prefix {
	u64 mid[8];      // the state after the whole blocks of the prefix (32-bit hashes: the low halves)
	u32 absorbed;    // octets in mid
	u32 tail_len;    // octets of the prefix behind them, below the block size
	int hash_type;   // libecc's hash_alg_type number: 1 .. 4 or 11
	u8 tail[128];
};

// digest octets of the hashes Z can be computed with, 0: not one of them
ESM3_FN int hash_size(int hash_type) { return hash_type == SM3 ? 32 : ecrfc::hash_size(hash_type); }
ESM3_FN u32 block_size(int hash_type) { return (hash_type == 3 || hash_type == 4) ? 128u : 64u; }

// SHA-2's end of a stream, as ecsm3::finish
template <int ALG, class ByteAt, typename KT>
ESM3_FN void sha2_finish(typename ecrfc::Alg<ALG>::W *st, u32 absorbed, u32 rest, const ByteAt &at, KT Kt)
{
	typedef typename ecrfc::Alg<ALG>::W W;
	constexpr u32 BLOCK = ecrfc::Alg<ALG>::BLOCK, LENF = ecrfc::Alg<ALG>::LENF, WB = sizeof(W);
	const u32 nblocks = (rest + 1u + LENF + BLOCK - 1u) / BLOCK;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 b = 0; b < nblocks; b++) {
		W w[16];
		for (u32 t = 0; t < 16; t++) {
			W v = 0;
			for (u32 k = 0; k < WB; k++) {
				const u32 pos = BLOCK * b + WB * t + k;
				const u32 byte = pos < rest ? (u32)at(pos) : (pos == rest ? 0x80u : 0u);
				v = (W)(v << 8) | (W)byte;
			}
			w[t] = v;
		}
		if (b + 1 == nblocks) {
			w[15] = (W)((absorbed + rest) << 3);   // (far below 2^29 octets)
		}
		ecrfc::compress<ALG>(st, w, Kt);
	}
}

template <int ALG, typename KT> static inline void sha2_prefix(Prefix &P, const u8 *buf, u32 len, KT Kt)
{
	typedef typename ecrfc::Alg<ALG>::W W;
	constexpr u32 BLOCK = ecrfc::Alg<ALG>::BLOCK, WB = sizeof(W);
	W st[8];
	ecrfc::iv<ALG>(st);
	u32 off = 0;
	for (; off + BLOCK <= len; off += BLOCK) {
		W w[16];
		for (u32 t = 0; t < 16; t++) {
			W v = 0;
			for (u32 k = 0; k < WB; k++) {
				v = (W)(v << 8) | (W)buf[off + WB * t + k];
			}
			w[t] = v;
		}
		ecrfc::compress<ALG>(st, w, Kt);
	}
	for (int j = 0; j < 8; j++) {
		P.mid[j] = (u64)st[j];
	}
	P.absorbed = off;
}

// The host's half: the prefix of a call.  a, b, gx, gy: clen octets each, big-endian.  k256 / k512: the SHA-2 round constants.
// Returns 0, or -1 for a hash or lengths outside what Z is computed for.
template <typename K256, typename K512>
static inline int prefix_init(Prefix &P, int hash_type, const u8 *id, u32 id_len, const u8 *a, const u8 *b, const u8 *gx, const u8 *gy, u32 clen,
			      K256 k256, K512 k512)
{
	if (hash_size(hash_type) == 0 || id_len > (u32)MAX_ID || clen == 0 || clen > (u32)MAX_CLEN || (id_len && !id)) {
		return -1;
	}
	u8 buf[2 + MAX_ID + 4 * MAX_CLEN];
	u32 len = 0;
	buf[len++] = (u8)((8u * id_len) >> 8);
	buf[len++] = (u8)(8u * id_len);
	if (id_len) {
		memcpy(buf + len, id, id_len);
	}
	len += id_len;
	const u8 *parts[4] = {a, b, gx, gy};
	for (int k = 0; k < 4; k++) {
		memcpy(buf + len, parts[k], clen);
		len += clen;
	}
	memset(&P, 0, sizeof(P));
	P.hash_type = hash_type;
	if (hash_type == SM3) {
		u32 st[8];
		ecsm3::init(st);
		u32 off = 0;
		for (; off + 64u <= len; off += 64u) {
			ecsm3::absorb(st, buf + off);
		}
		for (int j = 0; j < 8; j++) {
			P.mid[j] = st[j];
		}
		P.absorbed = off;
	} else if (hash_type == 1) {
		sha2_prefix<224>(P, buf, len, k256);
	} else if (hash_type == 2) {
		sha2_prefix<256>(P, buf, len, k256);
	} else if (hash_type == 3) {
		sha2_prefix<384>(P, buf, len, k512);
	} else {
		sha2_prefix<512>(P, buf, len, k512);
	}
	P.tail_len = len - P.absorbed;
	memcpy(P.tail, buf + P.absorbed, P.tail_len);
	return 0;
}

// octet pos of  tail || key
struct TailKey {
	const u8 *tail;
	u32 tail_len;
	const u8 *key;
	ESM3_FN u8 operator()(u32 pos) const { return pos < tail_len ? tail[pos] : key[pos - tail_len]; }
};

template <int ALG, typename KT> ESM3_FN void sha2_item(const Prefix &P, const TailKey &at, u32 rest, u8 *out, KT Kt)
{
	typedef typename ecrfc::Alg<ALG>::W W;
	W st[8];
	for (int j = 0; j < 8; j++) {
		st[j] = (W)P.mid[j];
	}
	sha2_finish<ALG>(st, P.absorbed, rest, at, Kt);
	constexpr int WB = sizeof(W);
	for (int k = 0; k < ecrfc::Alg<ALG>::HSIZE; k++) {
		out[k] = (u8)(st[k / WB] >> (8 * (WB - 1 - k % WB)));
	}
}

// An item's half: Z of the key (klen = 2 clen octets) into out (hash_size octets)
template <typename K256, typename K512> ESM3_FN void z_item(const Prefix &P, const u8 *key, u32 klen, u8 *out, K256 k256, K512 k512)
{
	const TailKey at = {P.tail, P.tail_len, key};
	const u32 rest = P.tail_len + klen;
	if (P.hash_type == SM3) {
		u32 st[8];
		for (int j = 0; j < 8; j++) {
			st[j] = (u32)P.mid[j];
		}
		ecsm3::finish(st, P.absorbed, rest, at);
		ecsm3::digest_bytes(st, out);
	} else if (P.hash_type == 1) {
		sha2_item<224>(P, at, rest, out, k256);
	} else if (P.hash_type == 2) {
		sha2_item<256>(P, at, rest, out, k256);
	} else if (P.hash_type == 3) {
		sha2_item<384>(P, at, rest, out, k512);
	} else {
		sha2_item<512>(P, at, rest, out, k512);
	}
}

}  // namespace ecsm2z
