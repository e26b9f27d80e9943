// libecc_amd/csrc/ecamd_digest_msgs.hip -- k_digest_msgs<ID>: the digests of a packed, ragged message array, one item per lane, for every
// hash of ecamd_hmac.h's trait.  ID is libecc's hash_alg_type number; the steps are ecamd_digest_msgs.h's.  This file is the launch
// geometry, the constants, the LDS and the stores, as ecamd_hmac.hip has them.
//
// A lane walks the blocks of call_prefix || item_prefix || message with all hash state in registers; the call prefix is read from the
// kernel's arguments, the item prefix octet by octet, the message as aligned words of the array.  There is no midstate: the call
// prefix is absorbed again by every item.  The code of a kernel holds ONE copy of its compression function or permutation
// (echm::Hash<ID>::hash).  Lanes of a wave have different trip counts and the wave ends with its longest message.  With Streebog each
// workgroup first builds the 16 KiB table in LDS and walks a grid-stride loop over the items (at most 2048 workgroups).  Registers,
// scratch and LDS as the compiler reports them: profiles/r22_digest_msgs.md.
//
// Nothing here is secret.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_digest_msgs.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__constant__ u32 c_dm_k256[64] = {ECAMD_SHA256_K};
__constant__ u64 c_dm_k512[80] = {ECAMD_SHA512_K};
__constant__ u64 c_dm_keccak_rc[24] = {ECAMD_KECCAK_RC};
__constant__ u64 c_dm_bash_rc[24] = {ECAMD_BASH_RC};
__constant__ u8 c_dm_sb_pi[256] = {ECAMD_STREEBOG_PI};
__constant__ u64 c_dm_sb_a[64] = {ECAMD_STREEBOG_A};
__constant__ u64 c_dm_sb_c[96] = {ECAMD_STREEBOG_C};

// what echm::Hash<ID>::hash reads its constants through
struct DmEnv {
	const u32 *k256;
	const u64 *k512, *keccak_rc, *bash_rc, *sb_T, *sb_C;
	__device__ __forceinline__ void tick() const {}
};

template <int ID> static constexpr bool dm_streebog = ID == 13 || ID == 14;

template <int ID> __global__ __launch_bounds__(64) void k_digest_msgs(EcamdDigestMsgsArgs A)
{
	typedef echm::Hash<ID> H;
	__shared__ u64 sT[dm_streebog<ID> ? ecsb::TABLE_WORDS : 1];
	if constexpr (dm_streebog<ID>) {   // Streebog's table into LDS (32 entries per lane); every lane of the workgroup comes through here
		for (u32 e = threadIdx.x; e < (u32)ecsb::TABLE_WORDS; e += 64) {
			sT[e] = ecsb::table_entry(c_dm_sb_pi, c_dm_sb_a, e >> 8, e & 255u);
		}
		__syncthreads();
	}
	const DmEnv env{c_dm_k256, c_dm_k512, c_dm_keccak_rc, c_dm_bash_rc, sT, c_dm_sb_c};
	for (u32 i = blockIdx.x * 64 + threadIdx.x; i < A.n; i += gridDim.x * 64) {
		const u64 off0 = A.offsets[i], off1 = A.offsets[i + 1];
		const int st = echm_msgs::digest<H>(env, A.call_prefix, A.call_prefix_len, A.item_prefixes + (size_t)i * A.item_prefix_stride,
						    A.item_prefix_len, A.msgs, off0, off1, A.msgs_len, A.digests + (size_t)i * H::HSIZE);
		if (A.status) {
			A.status[i] = (u8)st;
		}
	}
}

hipError_t ecamd_launch_digest_msgs(int hash_type, const EcamdDigestMsgsArgs &a, hipStream_t s)
{
	if (!echm::served(hash_type) || a.call_prefix_len > (uint32_t)echm_msgs::MAX_PREFIX || a.item_prefix_len > (uint32_t)echm_msgs::MAX_PREFIX ||
	    ((uintptr_t)a.msgs & 3u) || ((uintptr_t)a.offsets & 7u)) {
		return hipErrorInvalidValue;
	}
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!a.offsets || !a.digests || (a.item_prefix_len && !a.item_prefixes)) {
		return hipErrorInvalidValue;
	}
	// at most 2048 workgroups for the kernels that fill an LDS table first (k_streebog_slots' bound); one per 64 items otherwise
	const uint32_t groups = (a.n + 63) / 64;
	const dim3 grid((hash_type == 13 || hash_type == 14) && groups > 2048u ? 2048u : groups), block(64);
	switch (hash_type) {
#define DM_CASE(ID) \
	case ID: hipLaunchKernelGGL(k_digest_msgs<ID>, grid, block, 0, s, a); break;
		ECHM_FOR_EACH_HASH(DM_CASE)
#undef DM_CASE
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
