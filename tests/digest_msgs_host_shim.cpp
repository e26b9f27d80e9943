// tests/digest_msgs_host_shim.cpp -- libecc_amd/csrc/ecamd_digest_msgs.h compiled for the host: item_ok and the three-segment digest that
// k_digest_msgs runs per lane, behind a C interface for ctypes (tests/digest_msgs_ref.py).  With -DDIGEST_MSGS_MAIN it is a stand-alone
// program for a run under the address and undefined-behaviour sanitizers: it reads cases from standard input and hashes each with the
// message array malloc'ed at EXACTLY round_up(total, 4) octets and the message ending at the array's last octet, so that a read below
// the array or past what the unit may read is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../libecc_amd/csrc/ecamd_digest_msgs.h"

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

struct HostEnv {
	const u32 *k256;
	const u64 *k512, *keccak_rc, *bash_rc, *sb_T, *sb_C;
	void tick() const {}
};

static HostEnv host_env()
{
	static bool built = false;
	if (!built) {
		for (u32 e = 0; e < (u32)ecsb::TABLE_WORDS; e++) {
			SB_T[e] = ecsb::table_entry(SB_PI, SB_A, e >> 8, e & 255u);
		}
		built = true;
	}
	return HostEnv{K256, K512, KECCAK_RC, BASH_RC, SB_T, SB_C};
}

// msgs: 4-byte aligned, readable up to round_up(total, 4)
template <int ID> static int digest_id(const u32 *cp, u32 cpl, const u8 *ip, u32 ipl, const u32 *msgs, u64 off0, u64 off1, u64 total, u8 *out)
{
	return echm_msgs::digest<echm::Hash<ID>>(host_env(), cp, cpl, ip, ipl, msgs, off0, off1, total, out);
}

static int digest_any(int hash_type, const u32 *cp, u32 cpl, const u8 *ip, u32 ipl, const u32 *msgs, u64 off0, u64 off1, u64 total, u8 *out)
{
	switch (hash_type) {
#define DM_CASE(ID) case ID: return digest_id<ID>(cp, cpl, ip, ipl, msgs, off0, off1, total, out);
		ECHM_FOR_EACH_HASH(DM_CASE)
#undef DM_CASE
	default: return -1;
	}
}

extern "C" {

int dm_item_ok(u64 off0, u64 off1, u64 total, u32 cpl, u32 ipl)
{
	return echm_msgs::item_ok(off0, off1, total, cpl, ipl) ? 1 : 0;
}

// the item msgs[off0 .. off1) of an array of `total` octets (any alignment: copied into aligned words here); the status, or -1
int dm_digest(int hash_type, const u8 *cp, u32 cpl, const u8 *ip, u32 ipl, const u8 *msgs, u64 off0, u64 off1, u64 total, u8 *out)
{
	if (cpl > 256 || ipl > 256) {
		return -1;
	}
	u32 cpw[64] = {0};
	if (cpl) {
		memcpy(cpw, cp, cpl);
	}
	std::vector<u32> w((size_t)((total + 3) / 4));
	if (total) {
		memcpy(w.data(), msgs, (size_t)total);
	}
	return digest_any(hash_type, cpw, cpl, ip, ipl, w.data(), off0, off1, total, out);
}

}  // extern "C"

#ifdef DIGEST_MSGS_MAIN
// stdin: per case six little-endian u32 (hash_type, call prefix length, item prefix length, lead, message length, 0), then the octets of
// the call prefix, the item prefix and the message.  The array holds `lead` octets in front of the message and ends with the message's
// last octet.  stdout: one digest per case, in hex.
int main()
{
	u32 hd[6];
	unsigned long cases = 0;
	while (fread(hd, 4, 6, stdin) == 6) {
		const int id = (int)hd[0];
		const u32 cpl = hd[1], ipl = hd[2], lead = hd[3], mlen = hd[4];
		if (cpl > 256 || ipl > 256 || echm::hash_size(id) == 0) {
			return 2;
		}
		// exact-size allocations: the call prefix in whole words up to its last octet, the item prefix to the octet, the array to
		// round_up(total, 4)
		const size_t cpw = (cpl + 3) / 4;
		const u64 total = (u64)lead + mlen;
		u32 *cp = (u32 *)calloc(cpw ? cpw : 1, 4);
		u8 *ip = (u8 *)malloc(ipl ? ipl : 1);
		u32 *arr = (u32 *)malloc(total ? (size_t)((total + 3) / 4) * 4 : 1);
		if (!cp || !ip || !arr) {
			return 3;
		}
		memset(arr, 0xee, total ? (size_t)((total + 3) / 4) * 4 : 1);
		if (fread(cp, 1, cpl, stdin) != cpl || fread(ip, 1, ipl, stdin) != ipl || fread((u8 *)arr + lead, 1, mlen, stdin) != mlen) {
			return 3;
		}
		u8 out[64];
		if (digest_any(id, cp, cpl, ip, ipl, arr, lead, total, total, out) != 0) {
			return 4;
		}
		for (int k = 0; k < echm::hash_size(id); k++) {
			printf("%02x", out[k]);
		}
		printf("\n");
		// an unusable item reads nothing: there is no array at all
		if (digest_any(id, cp, cpl, ip, ipl, nullptr, total + 1, total, total, out) != 1 || digest_any(id, cp, cpl, ip, ipl, nullptr, 0, total + 1, total, out) != 1) {
			return 5;
		}
		free(cp);
		free(ip);
		free(arr);
		cases++;
	}
	fprintf(stderr, "digest_msgs host walk done (%lu cases)\n", cases);
	return 0;
}
#endif
