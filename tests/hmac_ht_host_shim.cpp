// tests/hmac_ht_host_shim.cpp -- libecc_amd/csrc/ecamd_hmac.h compiled for the host: the traits, HMAC and the RFC 6979 generator that
// k_hmac_slots and k_rfc6979_nonce_ht run per lane, behind a C interface for ctypes (tests/hmac_ht_ref.py).  With -DHMAC_HT_MAIN it is
// a stand-alone program that walks every served hash over key and message lengths around the block size and over the generator, for
// a run under the address and undefined-behaviour sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../libecc_amd/csrc/ecamd_hmac.h"

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

// octets as words the unit may read up to the one that holds the last octet
static std::vector<u32> words_of(const u8 *p, u32 len)
{
	std::vector<u32> w((len + 3) / 4 + 1, 0);
	if (len) {
		memcpy(w.data(), p, len);
	}
	return w;
}

template <int ID> static int hash_id(const u8 *msg, u32 len, u8 *out)
{
	typedef echm::Hash<ID> H;
	u32 calls, dw[H::DW];
	const HostEnv env = host_env(&calls);
	const std::vector<u32> m = words_of(msg, len);
	echm::hash_words<H>(env, m.data(), len, dw);
	echm::words_to_bytes<H::DW>(dw, out);
	return H::HSIZE;
}

template <int ID> static int hmac_id(const u8 *key, u32 klen, const u8 *msg, u32 mlen, u8 *out, u32 *calls_out)
{
	typedef echm::Hash<ID> H;
	u32 calls, mac[H::DW];
	const HostEnv env = host_env(&calls);
	const std::vector<u32> k = words_of(key, klen), m = words_of(msg, mlen);
	echm::hmac_words<H>(env, k.data(), klen, m.data(), mlen, mac);
	echm::words_to_bytes<H::DW>(mac, out);
	if (calls_out) {
		*calls_out = calls;
	}
	return H::HSIZE;
}

template <int ID> static int slot_id(const u8 *kslot, u32 kstride, const u8 *mslot, u32 stride, u8 *out)
{
	typedef echm::Hash<ID> H;
	u32 calls;
	const HostEnv env = host_env(&calls);
	std::vector<u32> k(kstride / 4 + 1, 0), m(stride / 4 + 1, 0);
	memcpy(k.data(), kslot, kstride);
	memcpy(m.data(), mslot, stride);
	echm::slot_hmac<H>(env, (const u8 *)k.data(), kstride, (const u8 *)m.data(), stride, out);
	return H::HSIZE;
}

template <int ID> static int nonce_id(const u8 *priv, const u8 *dig, const u8 *q_be, u32 qbits, u8 *k_out, u32 *retries, u32 *calls_out)
{
	typedef echm::Hash<ID> H;
	const u32 qlen = (qbits + 7) / 8;
	u32 calls, q[ecrfc::NL], k[ecrfc::NL], tb[echm::TB_WORDS];
	const HostEnv env = host_env(&calls);
	for (int l = 0; l < ecrfc::NL; l++) {
		q[l] = 0;
	}
	for (u32 i = 0; i < qlen; i++) {
		q[i / 4] |= (u32)q_be[qlen - 1 - i] << (8 * (i % 4));
	}
	const int st = echm::nonce<H>(env, priv, dig, q, qbits, tb, 1, k, retries);
	ecrfc::limbs_to_be(k, k_out, qlen);
	for (int w = 0; w < echm::TB_WORDS; w++) {
		if (tb[w]) {
			return -2;   // the word buffer must come back zeroed
		}
	}
	if (calls_out) {
		*calls_out = calls;
	}
	return st;
}

#define HH_SWITCH(CALL) \
	switch (hash_type) { \
		ECHM_FOR_EACH_HASH(CALL) \
	default: return -1; \
	}

extern "C" {

// {digest octets, block octets}; 0: the number is not served
int hh_sizes(int hash_type, int *out)
{
	out[0] = echm::hash_size(hash_type);
	out[1] = echm::block_size(hash_type);
	return out[0] ? 0 : -1;
}

int hh_hash(int hash_type, const u8 *msg, u32 len, u8 *out)
{
#define HH_CASE(ID) case ID: return hash_id<ID>(msg, len, out);
	HH_SWITCH(HH_CASE)
#undef HH_CASE
}

// the MAC into out, the digest length returned; calls (may be NULL): the compression / permutation / g_N calls it took
int hh_hmac(int hash_type, const u8 *key, u32 klen, const u8 *msg, u32 mlen, u8 *out, u32 *calls)
{
#define HH_CASE(ID) case ID: return hmac_id<ID>(key, klen, msg, mlen, out, calls);
	HH_SWITCH(HH_CASE)
#undef HH_CASE
}

int hh_slot_hmac(int hash_type, const u8 *kslot, u32 kstride, const u8 *mslot, u32 stride, u8 *out)
{
#define HH_CASE(ID) case ID: return slot_id<ID>(kslot, kstride, mslot, stride, out);
	HH_SWITCH(HH_CASE)
#undef HH_CASE
}

// the generator: priv and k_out qlen octets, dig the hash's digest, q_be the order's qlen octets; returns its status (0 / 1)
int hh_nonce(int hash_type, const u8 *priv, const u8 *dig, const u8 *q_be, u32 qbits, u8 *k_out, u32 *retries, u32 *calls)
{
	if (qbits == 0 || (qbits + 7) / 8 > (u32)ecrfc::MAX_QLEN) {
		return -1;
	}
#define HH_CASE(ID) case ID: return nonce_id<ID>(priv, dig, q_be, qbits, k_out, retries, calls);
	HH_SWITCH(HH_CASE)
#undef HH_CASE
}

}  // extern "C"

#ifdef HMAC_HT_MAIN
int main()
{
	static const int ids[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 17, 18, 19, 20};
	// secp521r1's and secp192r1's orders: the longest T, and qlen > hsize
	static const char *Q521 = "01fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffa51868783bf2f966b7fcc0148f709a5d03bb5c9b8899c47aebb6fb71e91386409";
	static const char *Q192 = "ffffffffffffffffffffffff99def836146bc9b1b4d22831";
	unsigned acc = 0;
	for (int id : ids) {
		int sz[2];
		if (hh_sizes(id, sz)) {
			return 1;
		}
		const u32 B = (u32)sz[1];
		const u32 lens[] = {0, 1, B - 1, B, B + 1, 2 * B + 3};
		std::vector<u8> key(2 * B + 3), msg(2 * B + 3);
		for (size_t i = 0; i < key.size(); i++) {
			key[i] = (u8)(i * 7 + id);
			msg[i] = (u8)(i * 13 + 1);
		}
		u8 out[64];
		for (u32 kl : lens) {
			for (u32 ml : lens) {
				std::vector<u8> k(key.begin(), key.begin() + kl), m(msg.begin(), msg.begin() + ml);   // exact-size copies: a read past the end is an error
				if (hh_hmac(id, k.data(), kl, m.data(), ml, out, nullptr) != sz[0]) {
					return 1;
				}
				acc += out[0];
			}
		}
		for (const char *qh : {Q521, Q192}) {
			const u32 qlen = (u32)strlen(qh) / 2;
			std::vector<u8> q(qlen), priv(qlen, 0), kout(qlen), dig((size_t)sz[0], (u8)id);
			for (u32 i = 0; i < qlen; i++) {
				unsigned v;
				sscanf(qh + 2 * i, "%2x", &v);
				q[i] = (u8)v;
			}
			priv[qlen - 1] = 5;
			u32 retries;
			if (hh_nonce(id, priv.data(), dig.data(), q.data(), qlen == 66 ? 521 : 192, kout.data(), &retries, nullptr) != 0) {
				return 1;
			}
			acc += kout[qlen - 1];
		}
	}
	printf("hmac_ht host walk done (%u)\n", acc);
	return 0;
}
#endif
