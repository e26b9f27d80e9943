// tests/bip0340_nonce_ht_host_shim.cpp -- libecc_amd/csrc/ecamd_bip0340_nonce_ht.h compiled for the host: the generator that
// k_bip0340_nonce_ht runs per lane and the tag hashes the host layer computes per call, behind a C interface for ctypes
// (tests/sighash_ht_ref.py).  With -DBIP_HT_MAIN it is a stand-alone program that walks every served hash once per order size, for a
// run under the address and undefined-behaviour sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../libecc_amd/csrc/ecamd_bip0340_nonce_ht.h"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

static const u32 K256[64] = {ECAMD_SHA256_K};
static const u64 K512[80] = {ECAMD_SHA512_K};
static const u64 KECCAK_RC[24] = {ECAMD_KECCAK_RC};
static const u64 BASH_RC[24] = {ECAMD_BASH_RC};
static const u8 SB_PI[256] = {ECAMD_STREEBOG_PI};
static const u64 SB_A[64] = {ECAMD_STREEBOG_A};
static const u64 SB_C[96] = {ECAMD_STREEBOG_C};
static u64 SB_T[ecsb::TABLE_WORDS];

// the unit's constants, and a counter of the compression / permutation / g_N calls
struct HostEnv {
	const u32 *k256;
	const u64 *k512, *keccak_rc, *bash_rc, *sb_T, *sb_C;
	u32 *calls;
	void tick() const { ++*calls; }
};

static HostEnv host_env(u32 *calls)
{
	static bool built = false;
	if (!built) {
		for (u32 e = 0; e < (u32)ecsb::TABLE_WORDS; e++) {
			SB_T[e] = ecsb::table_entry(SB_PI, SB_A, e >> 8, e & 255u);
		}
		built = true;
	}
	*calls = 0;
	return HostEnv{K256, K512, KECCAK_RC, BASH_RC, SB_T, SB_C, calls};
}

template <int ID>
static int nonce_id(const u8 *priv, const u8 *Y, u32 clen, const u8 *aux, const u8 *msg, u32 mlen, const u8 *q_be, u32 qbits, u8 *k_out, u32 *calls_out)
{
	typedef echm::Hash<ID> H;
	const u32 qlen = (qbits + 7) / 8;
	u32 calls, q[ecbipht::NL], k[ecbipht::NL], tb[ecbipht::PRE_WORDS], ta[H::DW], tn[H::DW];
	for (int l = 0; l < ecbipht::NL; l++) {
		q[l] = 0;
	}
	for (u32 i = 0; i < qlen; i++) {
		q[i / 4] |= (u32)q_be[qlen - 1 - i] << (8 * (i % 4));
	}
	const HostEnv env = host_env(&calls);
	ecbipht::tag_hash<H>(env, "BIP0340/aux", 11, ta);
	ecbipht::tag_hash<H>(env, "BIP0340/nonce", 13, tn);
	calls = 0;
	const int st = ecbipht::nonce<H>(env, priv, Y, clen, aux, ta, tn, msg, mlen, q, qbits, tb, 1, k);
	ecrfc::limbs_to_be(k, k_out, qlen);
	for (int w = 0; w < ecbipht::PRE_WORDS; w++) {
		if (tb[w]) {
			return -2;   // the word buffer must come back zeroed
		}
	}
	if (calls_out) {
		*calls_out = calls;
	}
	return st;
}

template <int ID> static int tag_id(const char *tag, u32 len, u8 *out)
{
	typedef echm::Hash<ID> H;
	u32 calls, dw[H::DW];
	const HostEnv env = host_env(&calls);
	ecbipht::tag_hash<H>(env, tag, len, dw);
	echm::words_to_bytes<H::DW>(dw, out);
	return H::HSIZE;
}

extern "C" {

// the generator: priv, aux and k_out qlen octets, Y 2 clen octets, q_be the order's qlen octets; returns its status (0 / 1), -1 for a
// hash that is not served, -2 when the word buffer did not come back zeroed; calls (may be NULL): compression / permutation / g_N calls
int bh_nonce(int hash_type, const u8 *priv, const u8 *Y, u32 clen, const u8 *aux, const u8 *msg, u32 mlen, const u8 *q_be, u32 qbits, u8 *k_out,
	     u32 *calls)
{
	if (qbits == 0 || (qbits + 7) / 8 > (u32)ecbipht::MAX_QLEN || clen == 0 || clen > (u32)ecbipht::MAX_CLEN) {
		return -1;
	}
	switch (hash_type) {
#define BH_CASE(ID) case ID: return nonce_id<ID>(priv, Y, clen, aux, msg, mlen, q_be, qbits, k_out, calls);
		ECHM_FOR_EACH_HASH(BH_CASE)
#undef BH_CASE
	default: return -1;
	}
}

// H(tag) into out, the digest length returned
int bh_tag(int hash_type, const char *tag, u32 len, u8 *out)
{
	if (len > 55) {
		return -1;
	}
	switch (hash_type) {
#define BH_CASE(ID) case ID: return tag_id<ID>(tag, len, out);
		ECHM_FOR_EACH_HASH(BH_CASE)
#undef BH_CASE
	default: return -1;
	}
}

}  // extern "C"

#ifdef BIP_HT_MAIN
int main()
{
	static const int ids[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 17, 18, 19, 20};
	// secp521r1's and secp192r1's orders: hsize < qlen for every hash, and qlen 24 beside hsize 20 .. 64
	static const char *Q521 = "01fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffa51868783bf2f966b7fcc0148f709a5d03bb5c9b8899c47aebb6fb71e91386409";
	static const char *Q192 = "ffffffffffffffffffffffff99def836146bc9b1b4d22831";
	unsigned acc = 0;
	for (int id : ids) {
		const u32 B = (u32)echm::block_size(id);
		for (const char *qh : {Q521, Q192}) {
			const u32 qlen = (u32)strlen(qh) / 2, clen = qlen;
			std::vector<u8> q(qlen), priv(qlen, 0), aux(qlen, (u8)(0xa0 + id)), Y(2 * clen, (u8)id), kout(qlen);
			for (u32 i = 0; i < qlen; i++) {
				unsigned v;
				sscanf(qh + 2 * i, "%2x", &v);
				q[i] = (u8)v;
			}
			priv[qlen - 1] = 5;
			for (u32 ml : {0u, 1u, 3u, B - 1, B, B + 1, 2 * B + 5}) {
				std::vector<u8> msg(ml);   // an exact-size copy: a read past the end is an error
				for (u32 i = 0; i < ml; i++) {
					msg[i] = (u8)(i * 13 + 1);
				}
				Y[2 * clen - 1] = (u8)(ml & 1);
				if (bh_nonce(id, priv.data(), Y.data(), clen, aux.data(), msg.data(), ml, q.data(), qlen == 66 ? 521 : 192, kout.data(), nullptr) != 0) {
					return 1;
				}
				acc += kout[qlen - 1];
			}
		}
	}
	printf("bip0340_nonce_ht host walk done (%u)\n", acc);
	return 0;
}
#endif
