// libecc_amd/csrc/ecamd_eddsa_msgs.hip -- EdDSA's hashes for a batch whose messages lie in one packed, ragged array (ec_eddsa_verify_msgs_batch,
// ec_eddsa_verify_msgs_all_batch, ec_eddsa_sign_msgs_batch), one item per lane.  The steps are ecamd_eddsa_msgs.h's and
// ecamd_eddsa_sign.h's; this file is the launch geometry, the constants and the stores.
//
//   k_eddsa_vhram_msgs<ALG>     a verifier's hram = H(dom || R || A || M-or-PH(M)): R and A are read where the caller's signatures and
//                               keys lie, the message at msgs + offsets[i]; a fresh PH(M) stays in registers.  hram and a `bad` octet
//                               per item.
//   k_eddsa_expand_r_msgs<ALG>  k_eddsa_expand_r with the message from the array: h = H(sk), clamp, PH(M), r_hash; the same stores
//   k_eddsa_hram_msgs<ALG>      k_eddsa_hram likewise: PH(M) is read from scratch, R is copied into the signature
//   k_eddsa_msgs_all_fin        the whole-batch bit: 1 unless an item is bad or the combination's verdict octet is set
// Lanes of a wave absorb as many blocks as their own message needs; the wave ends with its longest.  A message starts at any octet:
// the 8-octet loads of its interior are unaligned when offsets[i] is no multiple of 8.  dom is the call's and is read from the kernel
// arguments.  Registers and scratch as the compiler reports them: profiles/r23_eddsa_msgs.md.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_eddsa_msgs.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__constant__ u64 c_edm_k512[80] = {ECAMD_SHA512_K};
__constant__ u64 c_edm_rc[24] = {ECAMD_KECCAK_RC};

template <int ALG> static __device__ __forceinline__ const u64 *edm_table()
{
	return eced::Var<ALG>::IS448 ? (const u64 *)c_edm_rc : (const u64 *)c_edm_k512;
}

template <int ALG> __global__ __launch_bounds__(64) void k_eddsa_vhram_msgs(EcamdEddsaMsgsArgs M)
{
	typedef eced::Var<ALG> V;
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= M.e.n) {
		return;
	}
	u32 mlen, bad;
	const u8 *msg = eced_msgs::message<ALG>(M.msgs, M.msgs_len, M.offsets, i, M.e.dom_len, &mlen, &bad);
	M.e.bad[i] = (u8)bad;
	u8 *out = M.e.hram + (size_t)i * V::HLEN;
	if (bad) {
		for (int b = 0; b < V::HLEN; b++) {
			out[b] = 0;
		}
		return;
	}
	eced_msgs::verify_hram<ALG>(M.e.dom, M.e.dom_len, M.vsigs + (size_t)i * 2 * V::KLEN, M.e.A + (size_t)i * V::KLEN, msg, mlen, out, edm_table<ALG>());
}

template <int ALG> __global__ __launch_bounds__(64) void k_eddsa_expand_r_msgs(EcamdEddsaMsgsArgs M)
{
	typedef eced::Var<ALG> V;
	const EcamdEddsaSignArgs &A = M.e;
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const u64 *kt = edm_table<ALG>();
	u64 prefix[V::PW];
	eced::expand_key<ALG>(A.sk + (size_t)i * V::KLEN, A.a + (size_t)i * V::KLEN, A.a_wide ? A.a_wide + (size_t)i * V::HLEN : nullptr, prefix, kt);
	u32 mlen, bad;
	const u8 *msg = eced_msgs::message<ALG>(M.msgs, M.msgs_len, M.offsets, i, A.dom_len, &mlen, &bad);
	A.bad[i] = (u8)bad;
	eced_msgs::sign_r_hash<ALG>(A.dom, A.dom_len, prefix, msg, mlen, V::PH ? A.ph + (size_t)i * eced::PH_LEN : nullptr, A.r_hash + (size_t)i * V::HLEN, kt);
}

template <int ALG> __global__ __launch_bounds__(64) void k_eddsa_hram_msgs(EcamdEddsaMsgsArgs M)
{
	typedef eced::Var<ALG> V;
	const EcamdEddsaSignArgs &A = M.e;
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const u8 *R = A.R + (size_t)i * V::KLEN;
	const u8 *tail;
	u32 tlen;
	if constexpr (V::PH) {
		tail = A.ph + (size_t)i * eced::PH_LEN;
		tlen = eced::PH_LEN;
	} else {
		u32 bad;
		tail = eced_msgs::message<ALG>(M.msgs, M.msgs_len, M.offsets, i, A.dom_len, &tlen, &bad);
	}
	eced::hram<ALG>(A.dom, A.dom_len, R, A.A + (size_t)i * V::KLEN, tail, tlen, A.hram + (size_t)i * V::HLEN, edm_table<ALG>());
	u8 *sig = A.sigs + (size_t)i * 2 * V::KLEN;
	for (int b = 0; b < V::KLEN; b++) {
		sig[b] = R[b];
	}
}

__global__ __launch_bounds__(256) void k_eddsa_msgs_all_fin(const u8 *flags, u32 n, u8 *all_valid)
{
	int any = 0;
	for (u32 i = threadIdx.x; i < n; i += 256) {
		any |= flags[i];
	}
	any = __syncthreads_or(any);
	if (threadIdx.x == 0) {
		all_valid[0] = any ? 0 : 1;
	}
}

#define EDM_DISPATCH(KERNEL)                                                                                    \
	switch (alg) {                                                                                          \
	case eced::EDDSA25519: hipLaunchKernelGGL(KERNEL<eced::EDDSA25519>, grid, block, 0, s, a); break;       \
	case eced::EDDSA25519CTX: hipLaunchKernelGGL(KERNEL<eced::EDDSA25519CTX>, grid, block, 0, s, a); break; \
	case eced::EDDSA25519PH: hipLaunchKernelGGL(KERNEL<eced::EDDSA25519PH>, grid, block, 0, s, a); break;   \
	case eced::EDDSA448: hipLaunchKernelGGL(KERNEL<eced::EDDSA448>, grid, block, 0, s, a); break;           \
	case eced::EDDSA448PH: hipLaunchKernelGGL(KERNEL<eced::EDDSA448PH>, grid, block, 0, s, a); break;       \
	default: return hipErrorInvalidValue;                                                                   \
	}

static bool edm_args_ok(int alg, const EcamdEddsaMsgsArgs &a)
{
	return eced::alg_ok(alg) && a.e.dom_len <= (uint32_t)eced::MAX_DOM && a.offsets && !((uintptr_t)a.offsets & 7u) && (a.msgs || !a.msgs_len);
}

hipError_t ecamd_launch_eddsa_vhram_msgs(int alg, const EcamdEddsaMsgsArgs &a, hipStream_t s)
{
	if (a.e.n == 0) {
		return hipSuccess;
	}
	if (!edm_args_ok(alg, a) || !a.vsigs || !a.e.A || !a.e.hram || !a.e.bad) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.e.n + 63) / 64), block(64);
	EDM_DISPATCH(k_eddsa_vhram_msgs)
	return hipGetLastError();
}

hipError_t ecamd_launch_eddsa_expand_msgs(int alg, const EcamdEddsaMsgsArgs &a, hipStream_t s)
{
	if (a.e.n == 0) {
		return hipSuccess;
	}
	if (!edm_args_ok(alg, a) || !a.e.sk || !a.e.a || !a.e.r_hash || !a.e.bad || (eced::alg_is_ph(alg) && !a.e.ph)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.e.n + 63) / 64), block(64);
	EDM_DISPATCH(k_eddsa_expand_r_msgs)
	return hipGetLastError();
}

hipError_t ecamd_launch_eddsa_hram_msgs(int alg, const EcamdEddsaMsgsArgs &a, hipStream_t s)
{
	if (a.e.n == 0) {
		return hipSuccess;
	}
	if (!edm_args_ok(alg, a) || !a.e.R || !a.e.A || !a.e.hram || !a.e.sigs || (eced::alg_is_ph(alg) && !a.e.ph)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.e.n + 63) / 64), block(64);
	EDM_DISPATCH(k_eddsa_hram_msgs)
	return hipGetLastError();
}

hipError_t ecamd_launch_eddsa_msgs_all_fin(const uint8_t *flags, uint32_t n, uint8_t *all_valid, hipStream_t s)
{
	if (!flags || !all_valid) {
		return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_eddsa_msgs_all_fin, dim3(1), dim3(256), 0, s, flags, n, all_valid);
	return hipGetLastError();
}
