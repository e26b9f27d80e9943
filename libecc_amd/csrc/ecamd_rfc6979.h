// libecc_amd/csrc/ecamd_rfc6979.h -- the nonce of deterministic ECDSA (RFC 6979 section 3.2) per item, as the reference runs it
// (__ecdsa_rfc6979_nonce, sig/ecdsa_common.c:48-169): SHA-224 / 256 / 384 / 512 compression on a register-resident state, HMAC over
// it, and the generator.  Compiles for the device (ecamd_rfc6979.hip: one item per lane) and for the host (tests/rfc6979_host_shim.cpp).
//
//   hsize  octets of the digest (28, 32, 48, 64); the hash of the message is also the hash of the HMAC, as in libecc
//   qlen   octets of the generator's order q, qbits its bits
//   V = 01 .. 01, K = 00 .. 00 (hsize octets each)
//   d, e   K = HMAC_K(V || 00 || int2octets(x) || bits2octets(h1)),  V = HMAC_K(V)
//   f, g   K = HMAC_K(V || 01 || int2octets(x) || bits2octets(h1)),  V = HMAC_K(V)
//   h      T = V1 || V2 ..., V = HMAC_K(V) each, until 8 |T| >= qbits; k = the first qlen octets of T >> (8 qlen - qbits);
//          k < q: done (k = 0 is NOT tested here, :149-150; the signing back end flags it as it flags every nonce outside
//          [1, q - 1]); otherwise K = HMAC_K(V || 00), V = HMAC_K(V), and again
//   bits2octets(h1): the digest as a big-endian integer, >> (8 hsize - qbits) when longer than qbits, reduced mod q (one
//          conditional subtraction: the value is below 2^qbits < 2 q), as qlen octets
//   int2octets(x): the qlen octets of the key as the caller gave them (nn_export_to_buf of the imported key, :77)
//
// HMAC: K has hsize <= block octets, so the key is never hashed.  The states after the ipad and the opad block of the current K are
// kept (K changes in d, f and on a retry only), so HMAC_K(V) is two compressions: 18 per item for SHA-256 with a 256-bit q.
//
// The one variable-length input, 00/01 || x || bits2octets(h1) (1 + 2 qlen octets, qlen a run-time value), is laid out once with
// its padding as big-endian words in a per-item word buffer `tb` of TAIL_WORDS words with stride `ts` (the kernel: LDS, word w of
// lane l at [w * 64 + l], no bank conflict; the host: a plain array, ts = 1); T of step h reuses it.  Every address into it depends
// on qlen and the lane only.
//
// SECRET DATA: x, K, V, T and k.  No table is indexed by any of them (the round constants are indexed by the round number), no
// branch depends on them except the RFC's own `k < q` retry, and the buffer is zeroed before the function returns.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECR_FN __host__ __device__ __forceinline__
#else
#define ECR_FN inline
#endif

// FIPS 180-4 round constants
#define ECAMD_SHA256_K                                                                                                                        \
	0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,   \
	0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,   \
	0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,   \
	0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,   \
	0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,   \
	0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2
#define ECAMD_SHA512_K                                                                                                                        \
	0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,                    \
	0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,                    \
	0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,                    \
	0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,                    \
	0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,                    \
	0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,                    \
	0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,                    \
	0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,                    \
	0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,                    \
	0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,                    \
	0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,                    \
	0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,                    \
	0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,                    \
	0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,                    \
	0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,                    \
	0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull

namespace ecrfc {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum : int {
	NL = 17,            // 32-bit limbs of q, of bits2octets(h1) and of k: orders of at most 544 bits
	MAX_QLEN = 66,      // secp521r1
	TAIL_WORDS = 52,    // the word buffer: SHA-384 with qlen 66 pads 48 + 133 octets to two blocks, 256 - 48 = 208 octets of them here
	MAX_RETRIES = 1000  // candidates tried per item (the bound of the typed layer's host loop; no libecc curve rejects half of them)
};

template <int ALG> struct Alg;
template <> struct Alg<224> { typedef u32 W; enum : int { HSIZE = 28, BLOCK = 64, ROUNDS = 64, LENF = 8 }; };
template <> struct Alg<256> { typedef u32 W; enum : int { HSIZE = 32, BLOCK = 64, ROUNDS = 64, LENF = 8 }; };
template <> struct Alg<384> { typedef u64 W; enum : int { HSIZE = 48, BLOCK = 128, ROUNDS = 80, LENF = 16 }; };
template <> struct Alg<512> { typedef u64 W; enum : int { HSIZE = 64, BLOCK = 128, ROUNDS = 80, LENF = 16 }; };

// libecc's hash_alg_type number (SHA224 = 1 .. SHA512 = 4) -> digest octets, 0: not one of the four
ECR_FN int hash_size(int hash_type)
{
	return hash_type == 1 ? 28 : hash_type == 2 ? 32 : hash_type == 3 ? 48 : hash_type == 4 ? 64 : 0;
}
// a message slot (u32 length, then the bytes) holds its message
ECR_FN bool slot_ok(u32 len, u32 stride) { return len <= stride - 4; }

ECR_FN u32 rotr(u32 x, int r) { return (x >> r) | (x << (32 - r)); }
ECR_FN u64 rotr(u64 x, int r) { return (x >> r) | (x << (64 - r)); }
ECR_FN u32 bsig0(u32 a) { return rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22); }
ECR_FN u32 bsig1(u32 e) { return rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25); }
ECR_FN u32 ssig0(u32 w) { return rotr(w, 7) ^ rotr(w, 18) ^ (w >> 3); }
ECR_FN u32 ssig1(u32 w) { return rotr(w, 17) ^ rotr(w, 19) ^ (w >> 10); }
ECR_FN u64 bsig0(u64 a) { return rotr(a, 28) ^ rotr(a, 34) ^ rotr(a, 39); }
ECR_FN u64 bsig1(u64 e) { return rotr(e, 14) ^ rotr(e, 18) ^ rotr(e, 41); }
ECR_FN u64 ssig0(u64 w) { return rotr(w, 1) ^ rotr(w, 8) ^ (w >> 7); }
ECR_FN u64 ssig1(u64 w) { return rotr(w, 19) ^ rotr(w, 61) ^ (w >> 6); }

template <int ALG> ECR_FN void iv(typename Alg<ALG>::W *h)
{
	if (ALG == 256) {
		h[0] = 0x6a09e667; h[1] = 0xbb67ae85; h[2] = 0x3c6ef372; h[3] = 0xa54ff53a; h[4] = 0x510e527f; h[5] = 0x9b05688c; h[6] = 0x1f83d9ab; h[7] = 0x5be0cd19;
	} else if (ALG == 224) {
		h[0] = 0xc1059ed8; h[1] = 0x367cd507; h[2] = 0x3070dd17; h[3] = 0xf70e5939; h[4] = 0xffc00b31; h[5] = 0x68581511; h[6] = 0x64f98fa7; h[7] = 0xbefa4fa4;
	} else if (ALG == 512) {
		h[0] = (typename Alg<ALG>::W)0x6a09e667f3bcc908ull; h[1] = (typename Alg<ALG>::W)0xbb67ae8584caa73bull;
		h[2] = (typename Alg<ALG>::W)0x3c6ef372fe94f82bull; h[3] = (typename Alg<ALG>::W)0xa54ff53a5f1d36f1ull;
		h[4] = (typename Alg<ALG>::W)0x510e527fade682d1ull; h[5] = (typename Alg<ALG>::W)0x9b05688c2b3e6c1full;
		h[6] = (typename Alg<ALG>::W)0x1f83d9abfb41bd6bull; h[7] = (typename Alg<ALG>::W)0x5be0cd19137e2179ull;
	} else {
		h[0] = (typename Alg<ALG>::W)0xcbbb9d5dc1059ed8ull; h[1] = (typename Alg<ALG>::W)0x629a292a367cd507ull;
		h[2] = (typename Alg<ALG>::W)0x9159015a3070dd17ull; h[3] = (typename Alg<ALG>::W)0x152fecd8f70e5939ull;
		h[4] = (typename Alg<ALG>::W)0x67332667ffc00b31ull; h[5] = (typename Alg<ALG>::W)0x8eb44a8768581511ull;
		h[6] = (typename Alg<ALG>::W)0xdb0c2e0d64f98fa7ull; h[7] = (typename Alg<ALG>::W)0x47b5481dbefa4fa4ull;
	}
}

// one compression: st <- st + f(st, w).  w (the block as 16 big-endian words) is used up as the message schedule.  Kt: the round
// constants of the word size (ECAMD_SHA256_K / ECAMD_SHA512_K), indexed by the round number only.
template <int ALG, typename KT> ECR_FN void compress(typename Alg<ALG>::W *st, typename Alg<ALG>::W *w, KT Kt)
{
	typedef typename Alg<ALG>::W W;
	W a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll 1
	for (int r = 0; r < Alg<ALG>::ROUNDS; r += 16) {
#pragma unroll
		for (int t = 0; t < 16; t++) {
			if (r > 0) {
				w[t] = w[t] + ssig0(w[(t + 1) & 15]) + w[(t + 9) & 15] + ssig1(w[(t + 14) & 15]);
			}
			const W t1 = h + bsig1(e) + ((e & f) ^ (~e & g)) + (W)Kt[r + t] + w[t];
			const W t2 = bsig0(a) + ((a & b) ^ (a & c) ^ (b & c));
			h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
		}
	}
	st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// the HMAC of one key: the states after its ipad block and after its opad block
template <int ALG> struct Hmac {
	typedef typename Alg<ALG>::W W;
	enum : int { VW = Alg<ALG>::HSIZE / (int)sizeof(W), WBITS = 8 * (int)sizeof(W) };
	W ist[8], ost[8];

	template <typename KT> ECR_FN void set_key(const W *K, KT Kt)
	{
		const W ipad = (W)0x3636363636363636ull, opad = (W)0x5c5c5c5c5c5c5c5cull;
		W w[16];
#pragma unroll
		for (int t = 0; t < 16; t++) {
			w[t] = (t < VW ? K[t] : (W)0) ^ ipad;
		}
		iv<ALG>(ist);
		compress<ALG>(ist, w, Kt);
#pragma unroll
		for (int t = 0; t < 16; t++) {
			w[t] = (t < VW ? K[t] : (W)0) ^ opad;
		}
		iv<ALG>(ost);
		compress<ALG>(ost, w, Kt);
	}

	// the outer hash over the inner digest `in` (its first VW words): out[0 .. VW - 1] is the HMAC
	template <typename KT> ECR_FN void outer(const W *in, W *out, KT Kt) const
	{
		W w[16];
#pragma unroll
		for (int t = 0; t < 16; t++) {
			w[t] = t < VW ? in[t] : (W)0;
		}
		w[VW] = (W)0x80 << (WBITS - 8);
		w[15] = (W)(8 * (Alg<ALG>::BLOCK + Alg<ALG>::HSIZE));
#pragma unroll
		for (int t = 0; t < 8; t++) {
			out[t] = ost[t];
		}
		compress<ALG>(out, w, Kt);
	}

	// HMAC_K(V) (zero = false) or HMAC_K(V || 00) (zero = true): one inner block
	template <typename KT> ECR_FN void of_v(const W *V, bool zero, W *out, KT Kt) const
	{
		W w[16], in[8];
#pragma unroll
		for (int t = 0; t < 16; t++) {
			w[t] = t < VW ? V[t] : (W)0;
		}
		w[VW] = zero ? (W)0x80 << (WBITS - 16) : (W)0x80 << (WBITS - 8);
		w[15] = (W)(8 * (Alg<ALG>::BLOCK + Alg<ALG>::HSIZE + (zero ? 1 : 0)));
#pragma unroll
		for (int t = 0; t < 8; t++) {
			in[t] = ist[t];
		}
		compress<ALG>(in, w, Kt);
		outer(in, out, Kt);
	}

	// HMAC_K(V || tail) (vw = VW) or HMAC_K(tail) (vw = 0, V not read): the tail's `tlen` octets lie in tb with 0x80 behind them and
	// zeros up to the end of the last block
	template <typename KT> ECR_FN void of_v_tail(const W *V, int vw, const u32 *tb, int ts, u32 tlen, W *out, KT Kt) const
	{
		const u32 total = (u32)vw * (u32)sizeof(W) + tlen;
		const u32 nb = (total + 1 + Alg<ALG>::LENF + Alg<ALG>::BLOCK - 1) / Alg<ALG>::BLOCK;
		W in[8];
#pragma unroll
		for (int t = 0; t < 8; t++) {
			in[t] = ist[t];
		}
#pragma unroll 1
		for (u32 b = 0; b < nb; b++) {
			W w[16];
#pragma unroll
			for (int t = 0; t < 16; t++) {
				const u32 j = 16 * b + (u32)t;
				W v;
				if (t < vw && b == 0) {
					v = V[t < VW ? t : 0];
				} else {
					const u32 m = j - (u32)vw;   // word of the tail
					if (sizeof(W) == 8) {
						v = (W)(((u64)tb[(2 * m) * ts] << 32) | tb[(2 * m + 1) * ts]);
					} else {
						v = (W)tb[m * ts];
					}
				}
				w[t] = (j == 16 * nb - 1) ? (W)(8 * (Alg<ALG>::BLOCK + total)) : v;
			}
			compress<ALG>(in, w, Kt);
		}
		outer(in, out, Kt);
	}
};

// octet `pos` of the word buffer (big-endian inside the words)
ECR_FN void tb_or(u32 *tb, int ts, u32 pos, u32 byte) { tb[(pos >> 2) * ts] |= byte << (8 * (3 - (pos & 3))); }
ECR_FN u32 tb_get(const u32 *tb, int ts, u32 pos) { return (tb[(pos >> 2) * ts] >> (8 * (3 - (pos & 3)))) & 0xffu; }
ECR_FN void tb_zero(u32 *tb, int ts)
{
#pragma unroll 1
	for (int w = 0; w < TAIL_WORDS; w++) {
		tb[w * ts] = 0;
	}
}

// v >>= sh, sh < 32 * NL: by the bits of sh, so that every limb index is a constant (sh depends on the curve and the hash only)
ECR_FN void shr_limbs(u32 *v, u32 sh)
{
#pragma unroll
	for (int k = 0; k < 10; k++) {
		if ((sh >> k) & 1u) {
#pragma unroll
			for (int j = 0; j < NL; j++) {
				if (k < 5) {
					const u32 hi = j + 1 < NL ? v[j + 1 < NL ? j + 1 : 0] : 0u;
					v[j] = (v[j] >> (1 << k)) | (hi << (32 - (1 << k)));
				} else {
					const int src = j + (1 << (k - 5));
					v[j] = src < NL ? v[src < NL ? src : 0] : 0u;
				}
			}
		}
	}
}

// a - b -> d, returns the borrow (1: a < b)
ECR_FN u32 sub_limbs(const u32 *a, const u32 *b, u32 *d)
{
	u32 borrow = 0;
#pragma unroll
	for (int j = 0; j < NL; j++) {
		const u64 t = (u64)a[j] - b[j] - borrow;
		d[j] = (u32)t;
		borrow = (u32)(t >> 63);
	}
	return borrow;
}

// the low qlen octets of v, big-endian, to out
ECR_FN void limbs_to_be(const u32 *v, u8 *out, u32 qlen)
{
#pragma unroll
	for (int l = 0; l < NL; l++) {
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const u32 bp = 4 * l + b;
			if (bp < qlen) {
				out[qlen - 1 - bp] = (u8)(v[l] >> (8 * b));
			}
		}
	}
}

// bits2octets(h1) as limbs: dig has the hash's HSIZE octets
template <int ALG> ECR_FN void bits2octets(const u8 *dig, const u32 *q, u32 qbits, u32 *h)
{
	constexpr int HS = Alg<ALG>::HSIZE;
#pragma unroll
	for (int l = 0; l < NL; l++) {
		h[l] = 0;
		if (4 * l < HS) {
			const u8 *p = dig + (HS - 4 - 4 * l < 0 ? 0 : HS - 4 - 4 * l);
			h[l] = ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | p[3];
		}
	}
	shr_limbs(h, 8u * HS > qbits ? 8u * HS - qbits : 0u);
	u32 d[NL];
	const u32 below = sub_limbs(h, q, d);
#pragma unroll
	for (int l = 0; l < NL; l++) {
		h[l] = below ? h[l] : d[l];
	}
}

// The generator.  priv: qlen octets; dig: HSIZE octets; q: NL little-endian limbs; tb / ts: the word buffer (TAIL_WORDS words).
// k: NL limbs out.  Returns 0, or 1 with k = 0 when MAX_RETRIES candidates were rejected; *retries: the candidates rejected.
template <int ALG, typename KT>
ECR_FN int nonce(const u8 *priv, const u8 *dig, const u32 *q, u32 qbits, u32 *tb, int ts, KT Kt, u32 *k, u32 *retries)
{
	typedef typename Alg<ALG>::W W;
	constexpr int VW = Hmac<ALG>::VW, HS = Alg<ALG>::HSIZE;
	const u32 qlen = (qbits + 7) / 8;
	// 00 || int2octets(x) || bits2octets(h1) || 80
	tb_zero(tb, ts);
	{
		u32 h[NL];
		bits2octets<ALG>(dig, q, qbits, h);
#pragma unroll 1
		for (u32 i = 0; i < qlen; i++) {
			tb_or(tb, ts, 1 + i, priv[i]);
		}
#pragma unroll
		for (int l = 0; l < NL; l++) {
#pragma unroll
			for (int b = 0; b < 4; b++) {
				const u32 bp = 4 * l + b;
				if (bp < qlen) {
					tb_or(tb, ts, 1 + qlen + (qlen - 1 - bp), (h[l] >> (8 * b)) & 0xffu);
				}
			}
		}
		tb_or(tb, ts, 1 + 2 * qlen, 0x80u);
	}
	W K[8], V[8];
#pragma unroll
	for (int t = 0; t < 8; t++) {
		K[t] = 0;
		V[t] = (W)0x0101010101010101ull;
	}
	Hmac<ALG> hm;
	hm.set_key(K, Kt);
	// steps d - g
#pragma unroll 1
	for (u32 c = 0; c < 2; c++) {
		if (c) {
			tb_or(tb, ts, 0, 1u);
		}
		hm.of_v_tail(V, VW, tb, ts, 1 + 2 * qlen, K, Kt);
		hm.set_key(K, Kt);
		hm.of_v(V, false, V, Kt);
	}
	tb_zero(tb, ts);
	// step h
	const u32 rounds = (qlen + HS - 1) / HS;
	u32 tries = 0;
	int status = 1;
	for (;;) {
#pragma unroll 1
		for (u32 r = 0; r < rounds; r++) {
			hm.of_v(V, false, V, Kt);
#pragma unroll
			for (int t = 0; t < VW; t++) {
				const u32 m = r * VW + (u32)t;
				if (sizeof(W) == 8) {
					tb[(2 * m) * ts] = (u32)((u64)V[t] >> 32);
					tb[(2 * m + 1) * ts] = (u32)V[t];
				} else {
					tb[m * ts] = (u32)V[t];
				}
			}
		}
#pragma unroll
		for (int l = 0; l < NL; l++) {
			k[l] = 0;
#pragma unroll
			for (int b = 0; b < 4; b++) {
				const u32 bp = 4 * l + b;
				if (bp < qlen) {
					k[l] |= tb_get(tb, ts, qlen - 1 - bp) << (8 * b);
				}
			}
		}
		shr_limbs(k, 8 * qlen - qbits);
		u32 d[NL];
		if (sub_limbs(k, q, d)) {        // k < q (:149)
			status = 0;
			break;
		}
		if (++tries >= (u32)MAX_RETRIES) {
#pragma unroll
			for (int l = 0; l < NL; l++) {
				k[l] = 0;
			}
			break;
		}
		hm.of_v(V, true, K, Kt);         // K = HMAC_K(V || 00)
		hm.set_key(K, Kt);
		hm.of_v(V, false, V, Kt);
	}
	tb_zero(tb, ts);
	*retries = tries;
	return status;
}

}  // namespace ecrfc
