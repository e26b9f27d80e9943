// libecc_amd/csrc/ecamd_hmac.hip -- k_hmac_slots<ID>: HMAC of a batch of (key slot, message slot) pairs, and k_rfc6979_nonce_ht<ID>:
// the nonce of deterministic ECDSA (RFC 6979 section 3.2) for the hashes k_rfc6979_nonce (ecamd_rfc6979.hip) does not have, one item
// per lane.  ID is libecc's hash_alg_type number; the steps are ecamd_hmac.h's.  This file is the launch geometry, the constants, the
// LDS and the stores.
//
// Both kernels keep all hash state in registers: the padded key or K, V, the inner digest, the block on its way in and the hash's own
// state.  The code of a kernel holds ONE copy of its compression function or permutation (ecamd_hmac.h says how), so the unrolled
// sponges stay within the instruction cache's reach.  Memory in the loops: the slots (k_hmac_slots), the lane's column of the word
// buffer in LDS (the nonce kernel: 34 words per lane, word w of lane l at [w * 64 + l], no bank conflict).  With Streebog each
// workgroup first builds the 16 KiB table in LDS as k_streebog_slots does and walks a grid-stride loop over the items.  Private keys
// are read octet by octet (qlen = 66 and 29 are no multiple of a word).  Registers and scratch as the compiler reports them:
// profiles/r20_hmac_ht.md.
//
// Lanes of a wave whose candidate was rejected run the RFC's retry while the others wait; the wave ends with its last lane.
//
// SECRET DATA: keys, K, V, T, k.  Only Streebog's look-ups are indexed by them; the host layer refuses 13 and 14 in secret-scalar
// mode.  Every other instantiation is the same code in both modes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_hmac.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__constant__ u32 c_hm_k256[64] = {ECAMD_SHA256_K};
__constant__ u64 c_hm_k512[80] = {ECAMD_SHA512_K};
__constant__ u64 c_hm_keccak_rc[24] = {ECAMD_KECCAK_RC};
__constant__ u64 c_hm_bash_rc[24] = {ECAMD_BASH_RC};
__constant__ u8 c_hm_sb_pi[256] = {ECAMD_STREEBOG_PI};
__constant__ u64 c_hm_sb_a[64] = {ECAMD_STREEBOG_A};
__constant__ u64 c_hm_sb_c[96] = {ECAMD_STREEBOG_C};

// what echm::Hash<ID>::hash reads its constants through
struct HmEnv {
	const u32 *k256;
	const u64 *k512, *keccak_rc, *bash_rc, *sb_T, *sb_C;
	__device__ __forceinline__ void tick() const {}
};

template <int ID> static constexpr bool is_streebog = ID == 13 || ID == 14;

// Streebog's table into LDS (32 entries per lane); every lane of the workgroup comes through here
template <int ID> __device__ __forceinline__ HmEnv hm_env(u64 *sT)
{
	if constexpr (is_streebog<ID>) {
		for (u32 e = threadIdx.x; e < (u32)ecsb::TABLE_WORDS; e += 64) {
			sT[e] = ecsb::table_entry(c_hm_sb_pi, c_hm_sb_a, e >> 8, e & 255u);
		}
		__syncthreads();
	}
	return HmEnv{c_hm_k256, c_hm_k512, c_hm_keccak_rc, c_hm_bash_rc, sT, c_hm_sb_c};
}

template <int ID> __global__ __launch_bounds__(64) void k_hmac_slots(const u8 *keys, u32 kstride, const u8 *msgs, u32 stride, u32 n, u8 *macs)
{
	typedef echm::Hash<ID> H;
	__shared__ u64 sT[is_streebog<ID> ? ecsb::TABLE_WORDS : 1];
	const HmEnv env = hm_env<ID>(sT);
	for (u32 i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64) {
		echm::slot_hmac<H>(env, keys + (size_t)i * kstride, kstride, msgs + (size_t)i * stride, stride, macs + (size_t)i * H::HSIZE);
	}
}

template <int ID> __global__ __launch_bounds__(64) void k_rfc6979_nonce_ht(EcamdRfc6979Args A)
{
	typedef echm::Hash<ID> H;
	__shared__ u64 sT[is_streebog<ID> ? ecsb::TABLE_WORDS : 1];
	__shared__ u32 sB[echm::TB_WORDS * 64];
	const HmEnv env = hm_env<ID>(sT);
	for (u32 i = blockIdx.x * 64 + threadIdx.x; i < A.n; i += gridDim.x * 64) {
		u32 k[ecrfc::NL];
		int st = 1;
		// a message slot whose length word does not fit the stride has no digest: no nonce either
		const bool slot_bad = A.slots != nullptr && !ecrfc::slot_ok(*(const u32 *)(A.slots + (size_t)i * A.stride), A.stride);
		if (slot_bad) {
#pragma unroll
			for (int l = 0; l < ecrfc::NL; l++) {
				k[l] = 0;
			}
		} else {
			u32 q[ecrfc::NL];
#pragma unroll
			for (int l = 0; l < ecrfc::NL; l++) {
				q[l] = A.q[l];
			}
			u32 retries;
			st = echm::nonce<H>(env, A.privs + (size_t)i * A.qlen, A.digests + (size_t)i * H::HSIZE, q, A.qbits, sB + threadIdx.x, 64, k, &retries);
		}
		ecrfc::limbs_to_be(k, A.nonces + (size_t)i * A.qlen, A.qlen);
		A.status[i] = (u8)st;
	}
}

// at most 2048 workgroups for the kernels that fill an LDS table first (k_streebog_slots' bound); one per 64 items otherwise
static uint32_t hm_grid(int hash_type, uint32_t n)
{
	const uint32_t groups = (n + 63) / 64;
	return (hash_type == 13 || hash_type == 14) && groups > 2048u ? 2048u : groups;
}

int ecamd_hmac_served(int hash_type)
{
	return echm::served(hash_type) ? 1 : 0;
}

hipError_t ecamd_launch_hmac_slots(int hash_type, const uint8_t *keys, uint32_t kstride, const uint8_t *msgs, uint32_t stride, uint32_t n, uint8_t *macs,
				   hipStream_t s)
{
	if (!echm::served(hash_type) || kstride < 4 || (kstride & 3u) || stride < 4 || (stride & 3u)) {
		return hipErrorInvalidValue;
	}
	if (n == 0) {
		return hipSuccess;
	}
	const dim3 grid(hm_grid(hash_type, n)), block(64);
	switch (hash_type) {
#define HM_CASE(ID) \
	case ID: hipLaunchKernelGGL(k_hmac_slots<ID>, grid, block, 0, s, keys, kstride, msgs, stride, n, macs); break;
		ECHM_FOR_EACH_HASH(HM_CASE)
#undef HM_CASE
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t ecamd_launch_rfc6979_nonce_ht(int hash_type, const EcamdRfc6979Args &a, hipStream_t s)
{
	if (hash_type >= 1 && hash_type <= 4) {
		return ecamd_launch_rfc6979_nonce(hash_type, a, s);   // k_rfc6979_nonce: the bytes and the speed of ec_rfc6979_nonce_batch
	}
	if (!echm::served(hash_type)) {
		return hipErrorInvalidValue;
	}
	if (a.n == 0) {
		return hipSuccess;
	}
	if (a.qlen == 0 || a.qlen > (uint32_t)ecrfc::MAX_QLEN || a.qlen != (a.qbits + 7) / 8 || (a.slots && (a.stride < 4 || (a.stride & 3u)))) {
		return hipErrorInvalidValue;
	}
	const dim3 grid(hm_grid(hash_type, a.n)), block(64);
	switch (hash_type) {
#define HM_CASE(ID) \
	case ID: hipLaunchKernelGGL(k_rfc6979_nonce_ht<ID>, grid, block, 0, s, a); break;
		HM_CASE(5) HM_CASE(6) HM_CASE(7) HM_CASE(8) HM_CASE(9) HM_CASE(10) HM_CASE(11) HM_CASE(13) HM_CASE(14) HM_CASE(15) HM_CASE(17) HM_CASE(18)
		HM_CASE(19) HM_CASE(20)
#undef HM_CASE
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
