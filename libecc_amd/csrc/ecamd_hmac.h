// libecc_amd/csrc/ecamd_hmac.h -- HMAC over every fixed-length hash that ec_digest_slots_batch serves, and the nonce of deterministic
// ECDSA (RFC 6979 section 3.2) over that HMAC, per item, as the reference runs them (hash/hmac.c:14-135; __ecdsa_rfc6979_nonce,
// sig/ecdsa_common.c:48-169).  Compiles for the device (ecamd_hmac.hip: one item per lane) and for the host
// (tests/hmac_ht_host_shim.cpp).
//
// THE TRAIT.  echm::Hash<ID> (ID: libecc's hash_alg_type number) has HSIZE, BLOCK (libecc's digest_size and block_size) and
//   hash(env, src, len, dw)   init, absorb, finalize in one walk over the blocks: src(b, t) is word t of block b of the input, four
//                             octets packed little-endian ("memory order", whatever the hash's own word order is), zero behind octet
//                             len - 1; dw receives the digest as HSIZE / 4 words in the same order
// on top of the per-item units that exist: ecrfc::compress (SHA-224 .. 512, and SHA-512/t with ecs5t::init), ecsm3::compress,
// ecrmd::compress, eckk::permute, ecbash::permute and ecsb::g_n.  The input is a FUNCTION of the block and word number, not a buffer:
// inside the unrolled block t is a constant, so the key block, V and the inner digest are read from registers by constant index, and
// only what is long (a message slot, the tail 00 || x || h1) comes from memory.  Every hash has ONE call of its compression function
// or permutation in the code of hash(); the padding (0x80 and the bit count; 0x06 .. 0x80; 0x40; 0x01) is ORed in on the way.
//
//   ID      hash                HSIZE            BLOCK
//   1 .. 4  SHA-224 .. 512      28, 32, 48, 64   64, 64, 128, 128
//   5 .. 8  SHA3-224 .. 512     28, 32, 48, 64   144, 136, 104, 72
//   9, 10   SHA-512/224, /256   28, 32           128
//   11      SM3                 32               64
//   13, 14  Streebog-256, -512  32, 64           64
//   15      RIPEMD-160          20               64
//   17 .. 20 BASH224 .. 512     28, 32, 48, 64   136, 128, 96, 64
// Belt-hash (16) and SHAKE256 (12) are not served.
//
// env: anything with the members k256, k512 (ECAMD_SHA256_K, ECAMD_SHA512_K), keccak_rc, bash_rc, sb_T (Streebog's combined table,
// ecsb::table_entry), sb_C (ECAMD_STREEBOG_C), each indexable, and tick(), called once per compression / permutation / g_N (the
// host shim counts with it; the device's does nothing).
//
// HMAC (hmac_init / hmac_update / hmac_finalize of the reference, in that order):
//   init      a key longer than BLOCK is hashed first (pass 0) and its HSIZE octets are the key; the key is zero-padded to BLOCK
//             octets; the inner context absorbs key ^ 0x36.., the outer one key ^ 0x5c..
//   update    the inner context absorbs the message (pass 1: the stream is the ipad block, then the message)
//   finalize  the inner digest is fed to the outer context (pass 2: the opad block, then HSIZE octets)
// The passes are iterations of one loop around one call of hash().  No midstate is kept: the padded key (BLOCK / 4 words) stays in
// registers and its block is absorbed again in each pass -- for a sponge that costs what restoring 200 octets of state would.
//
// RFC 6979 (nonce<H>): the steps, bits2octets, the 1000-candidate bound and the `k = 0 is not tested here` rule of ecamd_rfc6979.h.
// The key of every HMAC is K (HSIZE <= BLOCK octets: never hashed) and every message is V || tail with a tail of 0, 1 (the octet 00) or
// 1 + 2 qlen octets (00 / 01 || int2octets(x) || bits2octets(h1)), so ONE function serves them all (hmac_vt) and the generator is a
// loop around ONE call of it: a small state machine whose phase says what the MAC replaces (K or V) and what comes next.  T takes V
// HSIZE octets at a time until 8 |T| >= qbits (:142): rounds = ceil(qlen / HSIZE), four with RIPEMD-160 on a 521-bit order.
// The tail and T live in a per-item word buffer `tb` of TB_WORDS words with stride `ts` (the kernel: LDS, word w of lane l at
// [w * 64 + l]; the host: a plain array, ts = 1); every address into it depends on qlen, the phase and the lane only.
//
// SECRET DATA: the HMAC key, x, K, V, T and k.  With Streebog (13, 14) the table look-ups are indexed by state octets that depend on
// them: the entry points refuse those two in secret-scalar mode (include/libecc_amd.h).  No other hash looks anything up by data, and
// no branch depends on a secret except the RFC's own `k < q` retry.  tb is zeroed before nonce() returns.
#pragma once
#include <stdint.h>
#include "ecamd_rfc6979.h"
#include "ecamd_keccak.h"
#include "ecamd_sha512t.h"
#include "ecamd_rmd160.h"
#include "ecamd_sm3.h"
#include "ecamd_streebog.h"
#include "ecamd_bash.h"

#define EHM_FN ECR_FN

namespace echm {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

// libecc's hash_alg_type number -> served here
EHM_FN bool served(int hash_type) { return hash_type >= 1 && hash_type <= 20 && hash_type != 12 && hash_type != 16; }

EHM_FN u32 bswap(u32 x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

// the padding octet `pad` behind octet len - 1 of the input, as it falls into the word at octet position pos
EHM_FN u32 pad_bits(u32 len, u32 pos, u32 pad)
{
	const u32 d = len - pos;
	return d < 4u ? pad << (8u * d) : 0u;
}

// word j of the len octets at p (readable up to the word that holds the last octet), zero behind them
EHM_FN u32 mem_word(const u32 *p, u32 len, u32 j)
{
	const u32 pos = 4u * j;
	if (pos >= len) {
		return 0u;
	}
	const u32 w = p[j], rem = len - pos;
	return rem >= 4u ? w : (w & (0xffffffffu >> (8u * (4u - rem))));
}

// ---- the Merkle-Damgard hashes: 0x80, zeros, the bit count in the last two words of the last block ----
// Core: W (the word), BE (octets big-endian inside a word), HSIZE, BLOCK, init(h), compress(env, h, x)
template <class Core> struct Md {
	typedef typename Core::W W;
	enum : int { HSIZE = Core::HSIZE, BLOCK = Core::BLOCK, BW = BLOCK / 4, DW = HSIZE / 4 };

	template <class Env, class Src> static EHM_FN void hash(const Env &env, const Src &src, u32 len, u32 *dw)
	{
		W h[8];
		Core::init(h);
		const u32 nblocks = (len + 1u + 2u * (u32)sizeof(W) + (u32)BLOCK - 1u) / (u32)BLOCK;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
		for (u32 b = 0; b < nblocks; b++) {
			u32 w[BW];
#pragma unroll
			for (u32 t = 0; t < (u32)BW; t++) {
				w[t] = src(b, t) | pad_bits(len, (u32)BLOCK * b + 4u * t, 0x80u);
			}
			W x[16];
#pragma unroll
			for (int t = 0; t < 16; t++) {
				if constexpr (sizeof(W) == 8) {
					x[t] = (W)(((u64)bswap(w[2 * t]) << 32) | bswap(w[2 * t + 1]));
				} else {
					x[t] = (W)(Core::BE ? bswap(w[t]) : w[t]);
				}
			}
			if (b + 1u == nblocks) {   // (inputs are far below 2^29 octets: the count fits one word, the other one is zero)
				x[Core::BE ? 15 : 14] = (W)((W)len << 3);
			}
			env.tick();
			Core::compress(env, h, x);
		}
#pragma unroll
		for (int i = 0; i < DW; i++) {
			if constexpr (sizeof(W) == 8) {
				dw[i] = bswap((u32)((u64)h[i >> 1] >> ((i & 1) ? 0 : 32)));
			} else {
				dw[i] = Core::BE ? bswap((u32)h[i]) : (u32)h[i];
			}
		}
	}
};

// SHA-224 / 256 / 384 / 512 (ID 1 .. 4) and SHA-512/224, SHA-512/256 (9, 10)
template <int ID> struct Sha2Core {
	enum : int { WIDE = (ID == 1 || ID == 2) ? 0 : 1, HSIZE = ID == 1 ? 28 : ID == 2 ? 32 : ID == 3 ? 48 : ID == 4 ? 64 : ID == 9 ? 28 : 32,
		     BLOCK = WIDE ? 128 : 64 };
	static constexpr bool BE = true;
	typedef typename ecrfc::Alg<WIDE ? 512 : 256>::W W;
	static EHM_FN void init(W *h)
	{
		if constexpr (ID == 9 || ID == 10) {
			ecs5t::init<ID == 9 ? 224 : 256>(h);
		} else {
			ecrfc::iv<ID == 1 ? 224 : ID == 2 ? 256 : ID == 3 ? 384 : 512>(h);
		}
	}
	template <class Env> static EHM_FN void compress(const Env &env, W *h, W *x)
	{
		if constexpr (WIDE) {
			ecrfc::compress<512>(h, x, env.k512);
		} else {
			ecrfc::compress<256>(h, x, env.k256);
		}
	}
};

struct Sm3Core {
	enum : int { HSIZE = 32, BLOCK = 64 };
	static constexpr bool BE = true;
	typedef u32 W;
	static EHM_FN void init(W *h) { ecsm3::init(h); }
	template <class Env> static EHM_FN void compress(const Env &, W *h, W *x) { ecsm3::compress(h, x); }
};

struct Rmd160Core {
	enum : int { HSIZE = 20, BLOCK = 64 };
	static constexpr bool BE = false;
	typedef u32 W;
	static EHM_FN void init(W *h)
	{
		ecrmd::init(h);
		h[5] = h[6] = h[7] = 0;
	}
	template <class Env> static EHM_FN void compress(const Env &, W *h, W *x) { ecrmd::compress(h, x); }
};

// ---- SHA-3: every block XORed into the rate, 0x06 behind the message, 0x80 into the last octet of the last block ----
template <int HS> struct Sha3 {
	enum : int { HSIZE = HS, BLOCK = 200 - 2 * HS, BW = BLOCK / 4, DW = HSIZE / 4, LANES = BLOCK / 8 };

	template <class Env, class Src> static EHM_FN void hash(const Env &env, const Src &src, u32 len, u32 *dw)
	{
		u64 a[25];
#pragma unroll
		for (int k = 0; k < 25; k++) {
			a[k] = 0;
		}
		const u32 nfull = len / (u32)BLOCK;
		// iteration nfull is the rest (possibly empty) with the padding
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
		for (u32 b = 0; b <= nfull; b++) {
#pragma unroll
			for (u32 l = 0; l < (u32)LANES; l++) {
				const u32 pos = (u32)BLOCK * b + 8u * l;
				const u32 lo = src(b, 2u * l) | pad_bits(len, pos, 0x06u), hi = src(b, 2u * l + 1u) | pad_bits(len, pos + 4u, 0x06u);
				a[l] ^= (u64)lo | ((u64)hi << 32);
			}
			if (b == nfull) {
				a[LANES - 1] ^= 0x8000000000000000ull;
			}
			env.tick();
			eckk::permute(a, env.keccak_rc);
		}
#pragma unroll
		for (int i = 0; i < DW; i++) {
			dw[i] = (u32)(a[i >> 1] >> (32 * (i & 1)));
		}
	}
};

// ---- BASH: every block written over the rate, 0x40 behind the message ----
template <int HS> struct Bash {
	enum : int { HSIZE = HS, BLOCK = 192 - 2 * HS, BW = BLOCK / 4, DW = HSIZE / 4, WORDS = BLOCK / 8 };

	template <class Env, class Src> static EHM_FN void hash(const Env &env, const Src &src, u32 len, u32 *dw)
	{
		u64 s[24];
#pragma unroll
		for (int k = 0; k < 23; k++) {
			s[k] = 0;
		}
		s[23] = (u64)HSIZE;
		const u32 nfull = len / (u32)BLOCK;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
		for (u32 b = 0; b <= nfull; b++) {
#pragma unroll
			for (u32 l = 0; l < (u32)WORDS; l++) {
				const u32 pos = (u32)BLOCK * b + 8u * l;
				const u32 lo = src(b, 2u * l) | pad_bits(len, pos, 0x40u), hi = src(b, 2u * l + 1u) | pad_bits(len, pos + 4u, 0x40u);
				s[l] = (u64)lo | ((u64)hi << 32);
			}
			env.tick();
			ecbash::permute(s, env.bash_rc);
		}
#pragma unroll
		for (int i = 0; i < DW; i++) {
			dw[i] = (u32)(s[i >> 1] >> (32 * (i & 1)));
		}
	}
};

// ---- Streebog: g_N per block with N and Sigma, 0x01 behind the message, then g_0 over N and over Sigma ----
template <int HS> struct Streebog {
	enum : int { HSIZE = HS, BLOCK = 64, BW = 16, DW = HSIZE / 4 };

	template <class Env, class Src> static EHM_FN void hash(const Env &env, const Src &src, u32 len, u32 *dw)
	{
		u64 h[8], N[8], S[8], M[8], NN[8];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			h[j] = HS == 32 ? 0x0101010101010101ull : 0ull;
			N[j] = 0;
			S[j] = 0;
		}
		const u32 nfull = len / 64u;
		// iterations 0 .. nfull: the blocks of the message, the last one the rest (possibly empty) with its padding; nfull + 1 and
		// nfull + 2: g_0 over N and over Sigma
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
		for (u32 b = 0; b <= nfull + 2u; b++) {
			const bool msg = b <= nfull;
#pragma unroll
			for (u32 j = 0; j < 8; j++) {
				const u32 pos = 64u * b + 8u * j;
				const u32 lo = src(b, 2u * j) | pad_bits(len, pos, 0x01u), hi = src(b, 2u * j + 1u) | pad_bits(len, pos + 4u, 0x01u);
				M[j] = msg ? ((u64)lo | ((u64)hi << 32)) : (b == nfull + 1u ? N[j] : S[j]);
				NN[j] = msg ? N[j] : 0ull;
			}
			env.tick();
			ecsb::g_n(env.sb_T, env.sb_C, h, M, NN);
			if (msg) {
				u64 bits[8] = {b < nfull ? (u64)512 : (u64)(8u * (len & 63u)), 0, 0, 0, 0, 0, 0, 0};
				ecsb::add512(N, bits);
				ecsb::add512(S, M);
			}
		}
#pragma unroll
		for (int i = 0; i < DW; i++) {
			const int wd = (HS == 32 ? 8 : 0) + i;
			dw[i] = (u32)(h[wd >> 1] >> (32 * (wd & 1)));
		}
	}
};

template <int ID> struct Hash;
template <> struct Hash<1> : Md<Sha2Core<1>> {};
template <> struct Hash<2> : Md<Sha2Core<2>> {};
template <> struct Hash<3> : Md<Sha2Core<3>> {};
template <> struct Hash<4> : Md<Sha2Core<4>> {};
template <> struct Hash<5> : Sha3<28> {};
template <> struct Hash<6> : Sha3<32> {};
template <> struct Hash<7> : Sha3<48> {};
template <> struct Hash<8> : Sha3<64> {};
template <> struct Hash<9> : Md<Sha2Core<9>> {};
template <> struct Hash<10> : Md<Sha2Core<10>> {};
template <> struct Hash<11> : Md<Sm3Core> {};
template <> struct Hash<13> : Streebog<32> {};
template <> struct Hash<14> : Streebog<64> {};
template <> struct Hash<15> : Md<Rmd160Core> {};
template <> struct Hash<17> : Bash<28> {};
template <> struct Hash<18> : Bash<32> {};
template <> struct Hash<19> : Bash<48> {};
template <> struct Hash<20> : Bash<64> {};

// F(ID) for every served number, in `case`s of a switch over a hash_type
#define ECHM_FOR_EACH_HASH(F) \
	F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(13) F(14) F(15) F(17) F(18) F(19) F(20)

EHM_FN int hash_size(int hash_type)
{
	switch (hash_type) {
#define ECHM_CASE(ID) case ID: return Hash<ID>::HSIZE;
		ECHM_FOR_EACH_HASH(ECHM_CASE)
#undef ECHM_CASE
	default: return 0;
	}
}
EHM_FN int block_size(int hash_type)
{
	switch (hash_type) {
#define ECHM_CASE(ID) case ID: return Hash<ID>::BLOCK;
		ECHM_FOR_EACH_HASH(ECHM_CASE)
#undef ECHM_CASE
	default: return 0;
	}
}

// the plain hash of len octets held as words (the host shim checks the traits with it)
template <class H, class Env> EHM_FN void hash_words(const Env &env, const u32 *msg, u32 len, u32 *dw)
{
	H::hash(env, [&](u32 b, u32 t) -> u32 { return mem_word(msg, len, b * (u32)H::BW + t); }, len, dw);
}

// HMAC of mlen octets under a key of klen octets, both held as words (readable up to the word that holds the last octet); mac: the
// HSIZE / 4 words of the result
template <class H, class Env> EHM_FN void hmac_words(const Env &env, const u32 *key, u32 klen, const u32 *msg, u32 mlen, u32 *mac)
{
	constexpr u32 BW = (u32)H::BW, DW = (u32)H::DW, BLOCK = (u32)H::BLOCK, HS = (u32)H::HSIZE;
	const bool long_key = klen > BLOCK;
	u32 kb[BW], dg[DW];
#pragma unroll
	for (u32 t = 0; t < BW; t++) {
		kb[t] = mem_word(key, long_key ? 0u : klen, t);
	}
#pragma unroll
	for (u32 t = 0; t < DW; t++) {
		dg[t] = 0;
	}
	// pass 0 (long keys only): the key's digest becomes the key; 1: the inner hash; 2: the outer hash
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 pass = long_key ? 0u : 1u; pass < 3u; pass++) {
		const u32 padw = pass == 1u ? 0x36363636u : 0x5c5c5c5cu;
		const u32 len = pass == 0u ? klen : BLOCK + (pass == 1u ? mlen : HS);
		u32 out[DW];
		H::hash(env, [&](u32 b, u32 t) -> u32 {
			if (pass == 0u) {
				return mem_word(key, klen, b * BW + t);
			}
			if (b == 0u) {
				return kb[t] ^ padw;
			}
			if (pass == 1u) {
				return mem_word(msg, mlen, (b - 1u) * BW + t);
			}
			return (b == 1u && t < DW) ? dg[t < DW ? t : 0u] : 0u;
		}, len, out);
		if (pass == 0u) {
#pragma unroll
			for (u32 t = 0; t < BW; t++) {
				kb[t] = t < DW ? out[t < DW ? t : 0u] : 0u;
			}
		} else {
#pragma unroll
			for (u32 t = 0; t < DW; t++) {
				dg[t] = out[t];
			}
		}
	}
#pragma unroll
	for (u32 t = 0; t < DW; t++) {
		mac[t] = dg[t];
	}
}

// the words of a digest as its octets
template <int DW> EHM_FN void words_to_bytes(const u32 *dw, u8 *out)
{
#pragma unroll
	for (int k = 0; k < 4 * DW; k++) {
		out[k] = (u8)(dw[k >> 2] >> (8 * (k & 3)));
	}
}

// One pair of slots (a little-endian u32 length, then the octets; strides multiples of 4) -> HSIZE octets at out; a key or a message
// that does not fit its slot gives zeros.
template <class H, class Env> EHM_FN void slot_hmac(const Env &env, const u8 *kslot, u32 kstride, const u8 *mslot, u32 stride, u8 *out)
{
	const u32 *kw = (const u32 *)kslot, *mw = (const u32 *)mslot;
	const u32 klen = kw[0], mlen = mw[0];
	u32 mac[H::DW];
	if (klen > kstride - 4u || mlen > stride - 4u) {
#pragma unroll
		for (int t = 0; t < H::DW; t++) {
			mac[t] = 0;
		}
	} else {
		hmac_words<H>(env, kw + 1, klen, mw + 1, mlen, mac);
	}
	words_to_bytes<H::DW>(mac, out);
}

// ---- RFC 6979 section 3.2 over the HMAC above ----
enum : int {
	// the word buffer: 00 / 01 || x || bits2octets(h1) is 1 + 2 * 66 = 133 octets; T sits behind word 0 (which stays zero: the
	// retry's tail 00) and is less than qlen + HSIZE <= 130 octets
	TB_WORDS = 34
};

// octet `pos` of the word buffer (memory order)
EHM_FN void tb_or(u32 *tb, int ts, u32 pos, u32 byte) { tb[(pos >> 2) * ts] |= byte << (8u * (pos & 3u)); }
EHM_FN u32 tb_get(const u32 *tb, int ts, u32 pos) { return (tb[(pos >> 2) * ts] >> (8u * (pos & 3u))) & 0xffu; }
EHM_FN void tb_zero(u32 *tb, int ts)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (int w = 0; w < TB_WORDS; w++) {
		tb[w * ts] = 0;
	}
}

// HMAC_K(V || the first tlen octets of tb), tlen <= 4 * TB_WORDS: K, V and mac are HSIZE / 4 words
template <class H, class Env> EHM_FN void hmac_vt(const Env &env, const u32 *K, const u32 *V, const u32 *tb, int ts, u32 tlen, u32 *mac)
{
	constexpr u32 BW = (u32)H::BW, DW = (u32)H::DW, BLOCK = (u32)H::BLOCK, HS = (u32)H::HSIZE;
	static_assert(DW <= BW, "the key is never hashed and V lies in the first block behind it");
	u32 dg[DW];
#pragma unroll
	for (u32 t = 0; t < DW; t++) {
		dg[t] = 0;
	}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (u32 pass = 0; pass < 2u; pass++) {
		const u32 padw = pass == 0u ? 0x36363636u : 0x5c5c5c5cu;
		const u32 tl = pass == 0u ? tlen : 0u;
		u32 out[DW];
		H::hash(env, [&](u32 b, u32 t) -> u32 {
			if (b == 0u) {
				return (t < DW ? K[t < DW ? t : 0u] : 0u) ^ padw;
			}
			if (b == 1u && t < DW) {
				return pass == 0u ? V[t < DW ? t : 0u] : dg[t < DW ? t : 0u];
			}
			const u32 m = (b - 1u) * BW + t - DW;   // word of the tail
			if (4u * m >= tl) {
				return 0u;
			}
			const u32 w = tb[m * ts], rem = tl - 4u * m;
			return rem >= 4u ? w : (w & (0xffffffffu >> (8u * (4u - rem))));
		}, BLOCK + HS + tl, out);
#pragma unroll
		for (u32 t = 0; t < DW; t++) {
			dg[t] = out[t];
		}
	}
#pragma unroll
	for (u32 t = 0; t < DW; t++) {
		mac[t] = dg[t];
	}
}

// bits2octets(h1) as limbs: dig has HS octets (ecrfc::bits2octets for any digest length)
template <int HS> EHM_FN void bits2octets(const u8 *dig, const u32 *q, u32 qbits, u32 *h)
{
	constexpr int NL = ecrfc::NL;
#pragma unroll
	for (int l = 0; l < NL; l++) {
		h[l] = 0;
		if (4 * l < HS) {
			const u8 *p = dig + (HS - 4 - 4 * l < 0 ? 0 : HS - 4 - 4 * l);
			h[l] = ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | p[3];
		}
	}
	ecrfc::shr_limbs(h, 8u * HS > qbits ? 8u * HS - qbits : 0u);
	u32 d[NL];
	const u32 below = ecrfc::sub_limbs(h, q, d);
#pragma unroll
	for (int l = 0; l < NL; l++) {
		h[l] = below ? h[l] : d[l];
	}
}

// The generator.  priv: qlen octets; dig: HSIZE octets; q: NL little-endian limbs; tb / ts: the word buffer (TB_WORDS words).
// k: NL limbs out.  Returns 0, or 1 with k = 0 when MAX_RETRIES candidates were rejected; *retries: the candidates rejected.
template <class H, class Env> EHM_FN int nonce(const Env &env, const u8 *priv, const u8 *dig, const u32 *q, u32 qbits, u32 *tb, int ts, u32 *k, u32 *retries)
{
	constexpr int NL = ecrfc::NL;
	constexpr u32 DW = (u32)H::DW, HS = (u32)H::HSIZE;
	const u32 qlen = (qbits + 7u) / 8u;
	// 00 || int2octets(x) || bits2octets(h1)
	tb_zero(tb, ts);
	{
		u32 h[NL];
		bits2octets<(int)HS>(dig, q, qbits, h);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
		for (u32 i = 0; i < qlen; i++) {
			tb_or(tb, ts, 1u + i, priv[i]);
		}
#pragma unroll
		for (int l = 0; l < NL; l++) {
#pragma unroll
			for (int b = 0; b < 4; b++) {
				const u32 bp = 4u * l + b;
				if (bp < qlen) {
					tb_or(tb, ts, 1u + qlen + (qlen - 1u - bp), (h[l] >> (8 * b)) & 0xffu);
				}
			}
		}
	}
	u32 K[DW], V[DW];
#pragma unroll
	for (u32 t = 0; t < DW; t++) {
		K[t] = 0;
		V[t] = 0x01010101u;
	}
	// phase: what the next HMAC is
	//   0  d: K = HMAC_K(V || 00 || x || h1)     1  e: V = HMAC_K(V)     2  f: K = HMAC_K(V || 01 || x || h1)     3  g: V = HMAC_K(V)
	//   4  h: V = HMAC_K(V), appended to T; with the last one the candidate is tested
	//   5  retry: K = HMAC_K(V || 00)            6  retry: V = HMAC_K(V)
	enum : u32 { PH_D = 0, PH_E = 1, PH_F = 2, PH_G = 3, PH_T = 4, PH_RK = 5, PH_RV = 6, PH_DONE = 7 };
	const u32 rounds = (qlen + HS - 1u) / HS;
	u32 phase = PH_D, r = 0, tries = 0;
	int status = 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	while (phase != PH_DONE) {
		const bool to_k = phase == PH_D || phase == PH_F || phase == PH_RK;
		const u32 tlen = (phase == PH_D || phase == PH_F) ? 1u + 2u * qlen : (phase == PH_RK ? 1u : 0u);
		u32 mac[DW];
		hmac_vt<H>(env, K, V, tb, ts, tlen, mac);
#pragma unroll
		for (u32 t = 0; t < DW; t++) {
			K[t] = to_k ? mac[t] : K[t];
			V[t] = to_k ? V[t] : mac[t];
		}
		if (phase == PH_E) {
			tb_or(tb, ts, 0, 1u);
			phase = PH_F;
		} else if (phase == PH_G) {
			tb_zero(tb, ts);
			r = 0;
			phase = PH_T;
		} else if (phase == PH_RV) {
			r = 0;
			phase = PH_T;
		} else if (phase != PH_T) {
			phase++;   // d -> e, f -> g, retry K -> retry V
		} else {
#pragma unroll
			for (u32 t = 0; t < DW; t++) {
				tb[(1u + r * DW + t) * ts] = V[t];
			}
			if (++r == rounds) {
				// k = the first qlen octets of T >> (8 qlen - qbits)
#pragma unroll
				for (int l = 0; l < NL; l++) {
					k[l] = 0;
#pragma unroll
					for (int b = 0; b < 4; b++) {
						const u32 bp = 4u * l + b;
						if (bp < qlen) {
							k[l] |= tb_get(tb, ts, 4u + qlen - 1u - bp) << (8 * b);
						}
					}
				}
				ecrfc::shr_limbs(k, 8u * qlen - qbits);
				u32 d[NL];
				if (ecrfc::sub_limbs(k, q, d)) {        // k < q (:149)
					status = 0;
					phase = PH_DONE;
				} else if (++tries >= (u32)ecrfc::MAX_RETRIES) {
#pragma unroll
					for (int l = 0; l < NL; l++) {
						k[l] = 0;
					}
					phase = PH_DONE;
				} else {
					phase = PH_RK;
				}
			}
		}
	}
	tb_zero(tb, ts);
	*retries = tries;
	return status;
}

}  // namespace echm
