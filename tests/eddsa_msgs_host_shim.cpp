// Host build of libecc_amd/csrc/ecamd_eddsa_msgs.h (and through it ecamd_eddsa_sign.h; g++, no HIP): the per-item steps of EdDSA over a
// packed, ragged message array -- what k_eddsa_vhram_msgs, k_eddsa_expand_r_msgs and k_eddsa_hram_msgs run per lane -- for
// tests/test_eddsa_msgs_host.py.  With -DEDDSA_MSGS_MAIN: a stand-alone program (for -fsanitize=address,undefined) that walks the items
// of a binary stream over a packed array allocated with no slack before its first and behind its last octet.  Test infrastructure, not
// product code.
#include <stdint.h>
#include <string.h>
#include "../libecc_amd/csrc/ecamd_eddsa_msgs.h"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

static const u64 k512[80] = {ECAMD_SHA512_K};
static const u64 krc[24] = {ECAMD_KECCAK_RC};

#define EDM_FOR_ALG(CALL)                                  \
	switch (alg) {                                     \
	case eced::EDDSA25519: CALL(eced::EDDSA25519)      \
	case eced::EDDSA25519CTX: CALL(eced::EDDSA25519CTX) \
	case eced::EDDSA25519PH: CALL(eced::EDDSA25519PH)  \
	case eced::EDDSA448: CALL(eced::EDDSA448)          \
	case eced::EDDSA448PH: CALL(eced::EDDSA448PH)      \
	default: return -1;                                \
	}

template <int ALG> static const u64 *table() { return eced::Var<ALG>::IS448 ? krc : k512; }

template <int ALG> static int vhram(const eced::Dom &d, const u8 *R, const u8 *A, const u8 *msgs, u64 off0, u64 off1, u64 total, u8 *out)
{
	const u64 offs[2] = {off0, off1};
	u32 mlen, bad;
	const u8 *msg = eced_msgs::message<ALG>(msgs, total, offs, 0, d.len, &mlen, &bad);
	if (bad) {
		memset(out, 0, eced::Var<ALG>::HLEN);
		return 1;
	}
	eced_msgs::verify_hram<ALG>(d.b, d.len, R, A, msg, mlen, out, table<ALG>());
	return 0;
}

template <int ALG>
static int sign_hashes(const eced::Dom &d, const u8 *sk, const u8 *R, const u8 *A, const u8 *msgs, u64 off0, u64 off1, u64 total, u8 *a, u8 *r_hash,
		       u8 *hram)
{
	typedef eced::Var<ALG> V;
	const u64 offs[2] = {off0, off1};
	u64 prefix[V::PW];
	u8 ph[eced::PH_LEN];
	eced::expand_key<ALG>(sk, a, nullptr, prefix, table<ALG>());
	u32 mlen, bad;
	const u8 *msg = eced_msgs::message<ALG>(msgs, total, offs, 0, d.len, &mlen, &bad);
	eced_msgs::sign_r_hash<ALG>(d.b, d.len, prefix, msg, mlen, ph, r_hash, table<ALG>());
	// the second kernel: the message again, or the stored PH(M)
	const u8 *tail = V::PH ? ph : eced_msgs::message<ALG>(msgs, total, offs, 0, d.len, &mlen, &bad);
	eced::hram<ALG>(d.b, d.len, R, A, tail, V::PH ? (u32)eced::PH_LEN : mlen, hram, table<ALG>());
	return (int)bad;
}

extern "C" int edm_item_ok(int alg, u64 off0, u64 off1, u64 total, u32 dlen)
{
#define CALL(ALG) return eced_msgs::item_ok<ALG>(off0, off1, total, dlen) ? 1 : 0;
	EDM_FOR_ALG(CALL)
#undef CALL
}

// returns the item's `bad` octet, -1 for an unknown alg
extern "C" int edm_vhram(int alg, const u8 *adata, u32 adata_len, const u8 *R, const u8 *A, const u8 *msgs, u64 off0, u64 off1, u64 total, u8 *out)
{
	eced::Dom d;
	eced::dom_build(alg, adata, adata_len, &d);
#define CALL(ALG) return vhram<ALG>(d, R, A, msgs, off0, off1, total, out);
	EDM_FOR_ALG(CALL)
#undef CALL
}

extern "C" int edm_sign_hashes(int alg, const u8 *adata, u32 adata_len, const u8 *sk, const u8 *R, const u8 *A, const u8 *msgs, u64 off0, u64 off1,
			       u64 total, u8 *a, u8 *r_hash, u8 *hram)
{
	eced::Dom d;
	eced::dom_build(alg, adata, adata_len, &d);
#define CALL(ALG) return sign_hashes<ALG>(d, sk, R, A, msgs, off0, off1, total, a, r_hash, hram);
	EDM_FOR_ALG(CALL)
#undef CALL
}

#ifdef EDDSA_MSGS_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>

// stdin: a u32 count n, then the batch -- u32 alg, u32 adata_len, adata, n x (sk, R, A: klen octets each), n + 1 u64 offsets, the packed
// array of offsets[n] octets.  The array is copied into a heap block of EXACTLY offsets[n] octets (nothing readable before its first or
// behind its last octet: the sanitizer's red zones lie there), so are the keys and every output.  stdout: per item the hex of the
// verifier's hram, then of a, r_hash and the signer's hram.
static bool rd(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

static void hex(const std::vector<u8> &v)
{
	for (u8 b : v) {
		printf("%02x", b);
	}
	printf("\n");
}

int main(void)
{
	u32 n, alg, al;
	if (!rd(&n, 4) || !rd(&alg, 4) || !rd(&al, 4) || al > 255 || !eced::alg_ok((int)alg)) {
		return 2;
	}
	std::vector<u8> adata(al);
	const size_t kl = eced::alg_is448((int)alg) ? 57 : 32, hl = 2 * kl;
	std::vector<u8> keys((size_t)n * 3 * kl);
	std::vector<u64> offs((size_t)n + 1);
	if (!rd(adata.data(), al) || !rd(keys.data(), keys.size()) || !rd(offs.data(), offs.size() * 8)) {
		return 2;
	}
	u8 *arr = (u8 *)malloc(offs[n] ? (size_t)offs[n] : 1);
	if (!arr || !rd(arr, (size_t)offs[n])) {
		return 2;
	}
	if (offs[n] == 0) {   // an empty array: no octet of it may be read at all
		free(arr);
		arr = nullptr;
	}
	for (u32 i = 0; i < n; i++) {
		const u8 *k = keys.data() + (size_t)i * 3 * kl;
		std::vector<u8> sk(k, k + kl), R(k + kl, k + 2 * kl), A(k + 2 * kl, k + 3 * kl), vh(hl), a(kl), rh(hl), sh(hl);
		const int b1 = edm_vhram((int)alg, adata.data(), al, R.data(), A.data(), arr, offs[i], offs[i + 1], offs[n], vh.data());
		const int b2 = edm_sign_hashes((int)alg, adata.data(), al, sk.data(), R.data(), A.data(), arr, offs[i], offs[i + 1], offs[n], a.data(),
					       rh.data(), sh.data());
		if (b1 != 0 || b2 != 0) {
			return 3;
		}
		hex(vh);
		hex(a);
		hex(rh);
		hex(sh);
	}
	free(arr);
	fprintf(stderr, "host walk done (%u items)\n", n);
	return 0;
}
#endif
