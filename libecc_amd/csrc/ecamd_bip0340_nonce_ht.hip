// libecc_amd/csrc/ecamd_bip0340_nonce_ht.hip -- k_bip0340_nonce_ht<ID>: BIP0340's tagged-hash nonce (_bip0340_sign, sig/bip0340.c:213-294)
// for the hashes k_bip0340_nonce (ecamd_detnonce.hip) does not have, one item per lane.  ID is libecc's hash_alg_type number; the
// steps are ecamd_bip0340_nonce_ht.h's.  This file is the launch geometry, the constants, the LDS and the stores.
//
// The hash state, the block on its way in, the mask and the digest stay in registers; the code of a kernel holds ONE copy of its
// compression function or permutation.  Memory in the loops: the lane's column of the word buffer in LDS (66 words per lane, word w
// of lane l at [w * 64 + l], no bank conflict) and the message, read from the item's slot where it lies behind the fixed fields.
// With Streebog each workgroup first builds the 16 KiB table in LDS as k_streebog_slots does and walks a grid-stride loop over the
// items.  Registers, LDS and scratch as the compiler reports them: profiles/r21_sighash_ht.md.
//
// SECRET DATA: x, d, t, the nonce hash's state, k.  Only Streebog's look-ups are indexed by them; the host layer refuses 13 and 14 in
// secret-scalar mode.  Every other instantiation is the same code in both modes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_bip0340_nonce_ht.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__constant__ u32 c_bn_k256[64] = {ECAMD_SHA256_K};
__constant__ u64 c_bn_k512[80] = {ECAMD_SHA512_K};
__constant__ u64 c_bn_keccak_rc[24] = {ECAMD_KECCAK_RC};
__constant__ u64 c_bn_bash_rc[24] = {ECAMD_BASH_RC};
__constant__ u8 c_bn_sb_pi[256] = {ECAMD_STREEBOG_PI};
__constant__ u64 c_bn_sb_a[64] = {ECAMD_STREEBOG_A};
__constant__ u64 c_bn_sb_c[96] = {ECAMD_STREEBOG_C};

// what echm::Hash<ID>::hash reads its constants through
struct BnEnv {
	const u32 *k256;
	const u64 *k512, *keccak_rc, *bash_rc, *sb_T, *sb_C;
	__device__ __forceinline__ void tick() const {}
};

template <int ID> static constexpr bool bn_streebog = ID == 13 || ID == 14;

template <int ID> __global__ __launch_bounds__(64) void k_bip0340_nonce_ht(EcamdBip0340NonceHtArgs A)
{
	typedef echm::Hash<ID> H;
	constexpr u32 HS = (u32)H::HSIZE, DW = (u32)H::DW;
	__shared__ u64 sT[bn_streebog<ID> ? ecsb::TABLE_WORDS : 1];
	__shared__ u32 sB[ecbipht::PRE_WORDS * 64];
	if constexpr (bn_streebog<ID>) {
		// Streebog's table into LDS (32 entries per lane); every lane of the workgroup comes through here
		for (u32 e = threadIdx.x; e < (u32)ecsb::TABLE_WORDS; e += 64) {
			sT[e] = ecsb::table_entry(c_bn_sb_pi, c_bn_sb_a, e >> 8, e & 255u);
		}
		__syncthreads();
	}
	const BnEnv env{c_bn_k256, c_bn_k512, c_bn_keccak_rc, c_bn_bash_rc, sT, c_bn_sb_c};
	for (u32 i = blockIdx.x * 64 + threadIdx.x; i < A.n; i += gridDim.x * 64) {
		u32 k[ecbipht::NL];
#pragma unroll
		for (int l = 0; l < ecbipht::NL; l++) {
			k[l] = 0;
		}
		int st = 1;
		const u8 *slot = A.slots + (size_t)i * A.stride;
		const u32 len = *(const u32 *)slot;
		// a slot that does not hold the fixed fields or does not fit the stride, a key that did not import: no nonce
		if (ecbipht::slot_ok(len, A.stride, HS, A.clen) && A.kst[i] == 0) {
			u32 q[ecbipht::NL], ta[DW], tn[DW];
#pragma unroll
			for (int l = 0; l < ecbipht::NL; l++) {
				q[l] = A.q[l];
			}
#pragma unroll
			for (u32 t = 0; t < DW; t++) {
				ta[t] = A.tag_aux[t];
				tn[t] = A.tag_nonce[t];
			}
			const u32 fixed = ecbipht::fixed_len(HS, A.clen);
			st = ecbipht::nonce<H>(env, A.privs + (size_t)i * A.qlen, A.keys + (size_t)i * 2 * A.clen, A.clen, A.aux + (size_t)i * A.qlen, ta, tn,
					       slot + 4 + fixed, len - fixed, q, A.qbits, sB + threadIdx.x, 64, k);
		}
		ecrfc::limbs_to_be(k, A.nonces + (size_t)i * A.qlen, A.qlen);
		A.status[i] = (u8)st;
	}
}

hipError_t ecamd_launch_bip0340_nonce_ht(int hash_type, const EcamdBip0340NonceHtArgs &a, hipStream_t s)
{
	if (!echm::served(hash_type) || (hash_type >= 1 && hash_type <= 4)) {   // 1 .. 4: k_bip0340_nonce, with its own arguments
		return hipErrorInvalidValue;
	}
	if (a.n == 0) {
		return hipSuccess;
	}
	if (a.qlen == 0 || a.qlen > (uint32_t)ecbipht::MAX_QLEN || a.qlen != (a.qbits + 7) / 8 || a.clen == 0 || a.clen > (uint32_t)ecbipht::MAX_CLEN ||
	    a.stride < 4 || (a.stride & 3u)) {
		return hipErrorInvalidValue;
	}
	// at most 2048 workgroups for the kernels that fill an LDS table first (k_streebog_slots' bound); one per 64 items otherwise
	const uint32_t groups = (a.n + 63) / 64;
	const dim3 grid((hash_type == 13 || hash_type == 14) && groups > 2048u ? 2048u : groups), block(64);
	switch (hash_type) {
#define BN_CASE(ID) \
	case ID: hipLaunchKernelGGL(k_bip0340_nonce_ht<ID>, grid, block, 0, s, a); break;
		BN_CASE(5) BN_CASE(6) BN_CASE(7) BN_CASE(8) BN_CASE(9) BN_CASE(10) BN_CASE(11) BN_CASE(13) BN_CASE(14) BN_CASE(15) BN_CASE(17) BN_CASE(18)
		BN_CASE(19) BN_CASE(20)
#undef BN_CASE
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
