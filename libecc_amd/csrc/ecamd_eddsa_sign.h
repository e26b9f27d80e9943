// libecc_amd/csrc/ecamd_eddsa_sign.h -- the hashing front end of EdDSA signing per item, as the reference runs it: the key expansion
// of eddsa_derive_priv_key (sig/eddsa.c:611-688), the pre-hash of the PH variants (eddsa_compute_pre_hash, :1049-1077) and the two
// hashes of _eddsa_sign (:1554-1870), r = H(dom || prefix || PH(M)) (:1679-1707) and H(dom || R || A || PH(M)) (:1782-1835), for
// EDDSA25519 / CTX / PH (SHA-512) and EDDSA448 / PH (SHAKE256, 114 octets).  Compiles for the device (ecamd_eddsa_sign.hip: one item
// per lane) and for the host (tests/eddsa_sign_host_shim.cpp).
//
//   dom      dom2(x, y) / dom4(x, y) (:57-118): "SigEd25519 no Ed25519 collisions" or "SigEd448", octet(x), octet(OLEN(y)), y;
//            x = 1 for the PH variants; EDDSA25519 hashes none.  One per call, built on the host (dom_build), at most 289 octets.
//   h        H(secret key octets); clamp (:649-671): 25519 clears the low three bits of octet 0 and bit 7 of octet 31 and sets bit 6
//            of it; 448 clears the low two bits of octet 0, sets bit 7 of octet 55 and clears octet 56
//   a        the first half of h after the clamp (KLEN octets, little-endian), prefix the second half
//   PH(M)    SHA-512(M), or the first 64 octets of SHAKE256(M)
//
// The hashed strings are never assembled.  A hash input is a STREAM: a list of segments, each either octets in memory (dom, the
// message, R, A, a stored PH(M)) or octets packed into 64-bit words held in registers (the prefix, a fresh PH(M)), and
// word(g) returns the eight octets at offset g of the concatenation in the hash's word order (SHA-512 big-endian, Keccak
// little-endian).  The block loop asks for the 16 (17) words of each block with constant word numbers, so the block buffer and the
// Keccak state stay in registers.  A register segment at an arbitrary offset is read through a select over its words (4 or 8) and a
// funnel shift; which word is selected depends on the offset -- |dom|, a per-call value -- and on the block, never on the data.
//
// SECRET DATA: the key octets, h, a and the prefix, r_hash.  No table is indexed by any of them (round constants are indexed by
// the round number), and every branch is on a length or an offset: |dom|, KLEN, the message length, the block number.
#pragma once
#include <stdint.h>
#include "ecamd_rfc6979.h"   // ecrfc::compress<512>, ecrfc::iv<512>, ECR_FN, ECAMD_SHA512_K

// FIPS 202 round constants of Keccak-f[1600]
#define ECAMD_KECCAK_RC                                                                                                                       \
	0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,                    \
	0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,                    \
	0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,                    \
	0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,                    \
	0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull

namespace eced {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

// libecc's ec_alg_type numbers (lib_ecc_types.h:49-55)
enum : int { EDDSA25519 = 9, EDDSA25519CTX = 10, EDDSA25519PH = 11, EDDSA448 = 12, EDDSA448PH = 13 };
enum : int {
	MAX_ADATA = 255,
	MAX_DOM = 32 + 2 + MAX_ADATA,   // dom2 with the longest context
	DOM_BYTES = 296,                // the buffer that holds it (a multiple of 8)
	PH_LEN = 64                     // octets of PH(M), both families (sig/eddsa.c:1653, :1662)
};

template <int ALG> struct Var {
	static_assert(ALG >= EDDSA25519 && ALG <= EDDSA448PH, "an EdDSA ec_alg_type");
	enum : int {
		IS448 = ALG >= EDDSA448,
		KLEN = IS448 ? 57 : 32,       // octets of a key, of an encoded point, of S
		HLEN = 2 * KLEN,              // octets of a hash
		PH = ALG == EDDSA25519PH || ALG == EDDSA448PH,
		PW = IS448 ? 8 : 4            // words of the prefix
	};
};

ECR_FN bool alg_ok(int alg) { return alg >= EDDSA25519 && alg <= EDDSA448PH; }
ECR_FN bool alg_is448(int alg) { return alg >= EDDSA448; }
ECR_FN bool alg_takes_dom(int alg) { return alg != EDDSA25519; }
ECR_FN bool alg_is_ph(int alg) { return alg == EDDSA25519PH || alg == EDDSA448PH; }

// the per-call dom2 / dom4 string
struct Dom {
	u32 len;
	u8 b[DOM_BYTES];
};

// dom(x, y) of sig/eddsa.c:57-85: adata == NULL hashes OLEN(y) and no y (:79).  adata_len <= MAX_ADATA is the caller's check (:64).
inline void dom_build(int alg, const u8 *adata, u32 adata_len, Dom *d)
{
	static const char s2[] = "SigEd25519 no Ed25519 collisions", s4[] = "SigEd448";
	u32 n = 0;
	for (u32 i = 0; i < (u32)DOM_BYTES; i++) {
		d->b[i] = 0;
	}
	if (alg_takes_dom(alg)) {
		const char *s = alg_is448(alg) ? s4 : s2;
		for (; s[n]; n++) {
			d->b[n] = (u8)s[n];
		}
		d->b[n++] = alg_is_ph(alg) ? 1 : 0;
		d->b[n++] = (u8)adata_len;
		for (u32 i = 0; adata && i < adata_len; i++) {
			d->b[n++] = adata[i];
		}
	}
	d->len = n;
}

// a message slot (u32 length, then the bytes) holds its message
ECR_FN bool slot_ok(u32 len, u32 stride) { return len <= stride - 4; }

ECR_FN u64 bswap(u64 v) { return __builtin_bswap64(v); }
ECR_FN u64 load8(const u8 *p)
{
	u64 v;
	__builtin_memcpy(&v, p, 8);
	return v;
}
ECR_FN void store8(u8 *p, u64 v) { __builtin_memcpy(p, &v, 8); }

// ---- segments ----
// octets p[0 .. len) at stream offset off: the eight octets of the stream at g that fall inside (the others 0)
template <bool BE> ECR_FN u64 mem_word(const u8 *p, u32 off, u32 len, u32 g)
{
	if (g + 8 <= off || g >= off + len) {
		return 0;
	}
	if (g >= off && g + 8 <= off + len) {
		const u64 v = load8(p + (g - off));
		return BE ? bswap(v) : v;
	}
	u64 v = 0;
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const u32 pos = g + (u32)j - off;   // below off this wraps and fails the compare
		const u64 byte = pos < len ? p[pos] : 0;
		v |= byte << (BE ? 56 - 8 * j : 8 * j);
	}
	return v;
}

// 8 K octets in the words w[0 .. K) (the hash's word order, zero behind the segment's end) at stream offset off
template <bool BE, int K> ECR_FN u64 reg_word(const u64 *w, u32 off, u32 g)
{
	const int rel = (int)g - (int)off;
	if (rel <= -8 || rel >= 8 * K) {
		return 0;
	}
	const int idx = rel >> 3;          // floor: -1 .. K - 1
	const int sh = 8 * (rel & 7);
	u64 lo = 0, hi = 0;
#pragma unroll
	for (int k = 0; k < K; k++) {
		lo = idx == k ? w[k] : lo;
		hi = idx + 1 == k ? w[k] : hi;
	}
	// (x >> 1) >> (63 - sh): x >> (64 - sh) that is 0 at sh = 0
	return BE ? (lo << sh) | ((hi >> 1) >> (63 - sh)) : (lo >> sh) | ((hi << 1) << (63 - sh));
}

// ---- streams ----
// one run of octets in memory: H(secret key), PH(M)
struct MemStream {
	const u8 *p;
	u32 len;
	template <bool BE> ECR_FN u64 word(u32 g) const { return mem_word<BE>(p, 0, len, g); }
	ECR_FN u32 total() const { return len; }
};

// dom || prefix || M, or dom || prefix || PH(M) with PH(M) in registers (ph != NULL)
template <int PW> struct RStream {
	const u8 *dom;
	u32 dlen;
	const u64 *prefix;
	u32 klen;
	const u8 *msg;
	u32 mlen;
	const u64 *ph;
	template <bool BE> ECR_FN u64 word(u32 g) const
	{
		u64 v = mem_word<BE>(dom, 0, dlen, g) | reg_word<BE, PW>(prefix, dlen, g);
		if (ph) {
			v |= reg_word<BE, PH_LEN / 8>(ph, dlen + klen, g);
		} else {
			v |= mem_word<BE>(msg, dlen + klen, mlen, g);
		}
		return v;
	}
	ECR_FN u32 total() const { return dlen + klen + (ph ? (u32)PH_LEN : mlen); }
};

// dom || R || A || tail, all in memory; tail: M, or the stored PH(M)
struct HStream {
	const u8 *dom;
	u32 dlen;
	const u8 *R, *A;
	u32 klen;
	const u8 *tail;
	u32 tlen;
	template <bool BE> ECR_FN u64 word(u32 g) const
	{
		return mem_word<BE>(dom, 0, dlen, g) | mem_word<BE>(R, dlen, klen, g) | mem_word<BE>(A, dlen + klen, klen, g) |
		       mem_word<BE>(tail, dlen + 2 * klen, tlen, g);
	}
	ECR_FN u32 total() const { return dlen + 2 * klen + tlen; }
};

// ---- SHA-512 of a stream: st = the eight digest words ----
template <class S, typename KT> ECR_FN void sha512_stream(const S &src, u64 *st, KT Kt)
{
	const u32 total = src.total();
	const u32 nb = (total + 1 + 16 + 127) / 128;
	ecrfc::iv<512>(st);
#pragma unroll 1
	for (u32 b = 0; b < nb; b++) {
		u64 w[16];
#pragma unroll
		for (int t = 0; t < 16; t++) {
			const u32 g = 128 * b + 8 * (u32)t;
			u64 v = src.template word<true>(g);
			if ((total & ~7u) == g) {
				v |= 0x80ull << (56 - 8 * (total & 7u));
			}
			if (g == 128 * nb - 8) {
				v |= (u64)total * 8;      // the 128-bit length field: its high word is 0
			}
			w[t] = v;
		}
		ecrfc::compress<512>(st, w, Kt);
	}
}

// ---- SHAKE256 of a stream: s = the state after the last permutation, octet i of the output in s[i / 8] >> 8 (i % 8), i < 136 ----
ECR_FN u64 rotl(u64 x, int r) { return (x << r) | (x >> (64 - r)); }

template <typename RC> ECR_FN void keccak_f(u64 *s, RC rc)
{
	constexpr int rotc[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
	constexpr int piln[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
#pragma unroll 1
	for (int round = 0; round < 24; round++) {
		u64 c[5];
#pragma unroll
		for (int x = 0; x < 5; x++) {
			c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
		}
#pragma unroll
		for (int x = 0; x < 5; x++) {
			const u64 d = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1);
#pragma unroll
			for (int y = 0; y < 25; y += 5) {
				s[y + x] ^= d;
			}
		}
		u64 t = s[1];
#pragma unroll
		for (int i = 0; i < 24; i++) {
			const u64 keep = s[piln[i]];
			s[piln[i]] = rotl(t, rotc[i]);
			t = keep;
		}
#pragma unroll
		for (int y = 0; y < 25; y += 5) {
#pragma unroll
			for (int x = 0; x < 5; x++) {
				c[x] = s[y + x];
			}
#pragma unroll
			for (int x = 0; x < 5; x++) {
				s[y + x] = c[x] ^ (~c[(x + 1) % 5] & c[(x + 2) % 5]);
			}
		}
		s[0] ^= rc[round];
	}
}

template <class S, typename RC> ECR_FN void shake256_stream(const S &src, u64 *s, RC rc)
{
	const u32 total = src.total();
	const u32 nb = total / 136 + 1;
#pragma unroll
	for (int t = 0; t < 25; t++) {
		s[t] = 0;
	}
#pragma unroll 1
	for (u32 b = 0; b < nb; b++) {
#pragma unroll
		for (int t = 0; t < 17; t++) {
			const u32 g = 136 * b + 8 * (u32)t;
			u64 v = src.template word<false>(g);
			if ((total & ~7u) == g) {
				v ^= 0x1full << (8 * (total & 7u));
			}
			if (g == 136 * nb - 8) {
				v ^= 0x80ull << 56;       // at total = 135 mod 136 both fall into one octet: 0x9f
			}
			s[t] ^= v;
		}
		keccak_f(s, rc);
	}
}

// the first `len` octets of a digest (SHA-512: the big-endian words st; SHAKE256: the little-endian lanes s) to memory
template <bool BE> ECR_FN void words_out(const u64 *w, u8 *out, int len)
{
#pragma unroll
	for (int t = 0; 8 * t < len; t++) {
		if (8 * t + 8 <= len) {
			store8(out + 8 * t, BE ? bswap(w[t]) : w[t]);
		} else {
#pragma unroll
			for (int j = 0; 8 * t + j < len; j++) {
				out[8 * t + j] = (u8)(w[t] >> (BE ? 56 - 8 * j : 8 * j));
			}
		}
	}
}

// ---- the four steps ----
// H(sk) and the clamp: a (KLEN octets) to memory, zero-extended to HLEN octets at a_wide unless NULL; prefix: PW words.  KT: the
// SHA-512 round constants (25519) or the Keccak ones (448)
template <int ALG, typename KT> ECR_FN void expand_key(const u8 *sk, u8 *a, u8 *a_wide, u64 *prefix, KT kt)
{
	typedef Var<ALG> V;
	const MemStream src = {sk, (u32)V::KLEN};
	u64 aw[16];
#pragma unroll
	for (int t = 0; t < 16; t++) {
		aw[t] = 0;
	}
	if constexpr (V::IS448) {
		u64 s[25];
		shake256_stream(src, s, kt);
		s[0] &= ~3ull;                            // octet 0: the cofactor's bits (:649)
		s[6] |= 0x80ull << 56;                    // octet 55 (:670)
#pragma unroll
		for (int t = 0; t < 7; t++) {
			aw[t] = s[t];                     // octet 56 = 0 (:669)
			prefix[t] = (s[7 + t] >> 8) | (s[8 + t] << 56);   // octets 57 + 8 t ..
		}
		prefix[7] = (s[14] >> 8) & 0xffull;       // octet 113
	} else {
		u64 st[8];
		sha512_stream(src, st, kt);
		st[0] &= ~(7ull << 56);                   // octet 0 (:649)
		st[3] = (st[3] & ~0x80ull) | 0x40ull;     // octet 31 (:658-659)
#pragma unroll
		for (int t = 0; t < 4; t++) {
			aw[t] = bswap(st[t]);
			prefix[t] = st[4 + t];
		}
	}
	words_out<false>(aw, a, V::KLEN);
	if (a_wide) {
		words_out<false>(aw, a_wide, V::HLEN);
	}
}

// PH(M): 8 words in the hash's word order
template <int ALG, typename KT> ECR_FN void prehash(const u8 *msg, u32 mlen, u64 *ph, KT kt)
{
	const MemStream src = {msg, mlen};
	if constexpr (Var<ALG>::IS448) {
		u64 s[25];
		shake256_stream(src, s, kt);
#pragma unroll
		for (int t = 0; t < 8; t++) {
			ph[t] = s[t];
		}
	} else {
		sha512_stream(src, ph, kt);
	}
}

template <int ALG, class S, typename KT> ECR_FN void hash_out(const S &src, u8 *out, KT kt)
{
	if constexpr (Var<ALG>::IS448) {
		u64 s[25];
		shake256_stream(src, s, kt);
		words_out<false>(s, out, Var<ALG>::HLEN);
	} else {
		u64 st[8];
		sha512_stream(src, st, kt);
		words_out<true>(st, out, Var<ALG>::HLEN);
	}
}

// r_hash = H(dom || prefix || M) (ph == NULL) or H(dom || prefix || PH(M)): HLEN octets
template <int ALG, typename KT>
ECR_FN void r_hash(const u8 *dom, u32 dlen, const u64 *prefix, const u8 *msg, u32 mlen, const u64 *ph, u8 *out, KT kt)
{
	const RStream<Var<ALG>::PW> src = {dom, dlen, prefix, (u32)Var<ALG>::KLEN, msg, mlen, ph};
	hash_out<ALG>(src, out, kt);
}

// hram = H(dom || R || A || tail): HLEN octets
template <int ALG, typename KT> ECR_FN void hram(const u8 *dom, u32 dlen, const u8 *R, const u8 *A, const u8 *tail, u32 tlen, u8 *out, KT kt)
{
	const HStream src = {dom, dlen, R, A, (u32)Var<ALG>::KLEN, tail, tlen};
	hash_out<ALG>(src, out, kt);
}

}  // namespace eced
