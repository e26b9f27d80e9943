// libecc_amd/csrc/ecamd_eddsa_sign.hip -- the hashing front end of one-call EdDSA signing (ec_eddsa_sign_msg_batch) for a batch, one
// item per lane: eddsa_derive_priv_key (sig/eddsa.c:611-688) and the two hashes of _eddsa_sign (:1679-1707, :1782-1835).  The steps
// are ecamd_eddsa_sign.h's; this file is the launch geometry, the slot check and the stores.
//
//   k_eddsa_expand_r<ALG>  h = H(sk), clamp, PH(M) for the PH variants, r_hash = H(dom || prefix || M-or-PH(M)).  The prefix and a fresh
//                          PH(M) stay in registers; a and r_hash go to the context's secret scratch, PH(M) (public) beside them for
//                          the second hash.  Without slots: the key expansion alone (ec_eddsa_pub_key_batch).
//   k_eddsa_hram<ALG>      hram = H(dom || R || A || M-or-PH(M)); PH(M) is READ from scratch, not recomputed.  R is copied into the
//                          signature.
//   k_eddsa_sign_fin       S into the signature; status; zero bytes for a rejected item.
// Lanes of a wave absorb as many blocks as their own message needs (the block loop's bound is the lane's); dom is the call's and
// is read from the kernel arguments.  25519: 3 compressions per item for a short message in the first kernel, 1 in the second.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_eddsa_sign.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__constant__ u64 c_eds_k512[80] = {ECAMD_SHA512_K};
__constant__ u64 c_eds_rc[24] = {ECAMD_KECCAK_RC};

template <int ALG> static __device__ __forceinline__ const u64 *eds_table()
{
	return eced::Var<ALG>::IS448 ? (const u64 *)c_eds_rc : (const u64 *)c_eds_k512;
}

// the lane's message: NULL slots or a length that does not fit give an empty one and *bad = 1
static __device__ __forceinline__ const u8 *eds_message(const u8 *slots, u32 stride, u32 i, u32 *mlen, u32 *bad)
{
	const u8 *slot = slots + (size_t)i * stride;
	const u32 len = *(const u32 *)slot;
	*bad = eced::slot_ok(len, stride) ? 0u : 1u;
	*mlen = *bad ? 0u : len;
	return slot + 4;
}

template <int ALG> __global__ __launch_bounds__(64) void k_eddsa_expand_r(EcamdEddsaSignArgs A)
{
	typedef eced::Var<ALG> V;
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const u64 *kt = eds_table<ALG>();
	u64 prefix[V::PW];
	eced::expand_key<ALG>(A.sk + (size_t)i * V::KLEN, A.a + (size_t)i * V::KLEN, A.a_wide ? A.a_wide + (size_t)i * V::HLEN : nullptr, prefix, kt);
	if (!A.slots) {
		return;
	}
	u32 mlen, bad;
	const u8 *msg = eds_message(A.slots, A.stride, i, &mlen, &bad);
	A.bad[i] = (u8)bad;
	u8 *out = A.r_hash + (size_t)i * V::HLEN;
	if constexpr (V::PH) {
		u64 ph[eced::PH_LEN / 8];
		eced::prehash<ALG>(msg, mlen, ph, kt);
		if constexpr (V::IS448) {
			eced::words_out<false>(ph, A.ph + (size_t)i * eced::PH_LEN, eced::PH_LEN);
		} else {
			eced::words_out<true>(ph, A.ph + (size_t)i * eced::PH_LEN, eced::PH_LEN);
		}
		eced::r_hash<ALG>(A.dom, A.dom_len, prefix, nullptr, 0, ph, out, kt);
	} else {
		eced::r_hash<ALG>(A.dom, A.dom_len, prefix, msg, mlen, nullptr, out, kt);
	}
}

template <int ALG> __global__ __launch_bounds__(64) void k_eddsa_hram(EcamdEddsaSignArgs A)
{
	typedef eced::Var<ALG> V;
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
		tail = eds_message(A.slots, A.stride, i, &tlen, &bad);
	}
	eced::hram<ALG>(A.dom, A.dom_len, R, A.A + (size_t)i * V::KLEN, tail, tlen, A.hram + (size_t)i * V::HLEN, eds_table<ALG>());
	u8 *sig = A.sigs + (size_t)i * 2 * V::KLEN;
	for (int b = 0; b < V::KLEN; b++) {
		sig[b] = R[b];
	}
}

template <int KLEN> __global__ __launch_bounds__(64) void k_eddsa_sign_fin(EcamdEddsaSignArgs A)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const bool rej = (A.bad[i] | A.stR[i] | (A.stA ? A.stA[i] : 0)) != 0;
	u8 *sig = A.sigs + (size_t)i * 2 * KLEN;
	const u8 *S = A.S + (size_t)i * KLEN;
	for (int b = 0; b < KLEN; b++) {
		sig[KLEN + b] = rej ? (u8)0 : S[b];
		if (rej) {
			sig[b] = 0;
		}
	}
	A.status[i] = rej ? 1 : 0;
}

#define EDS_DISPATCH(KERNEL)                                                                                    \
	switch (alg) {                                                                                          \
	case eced::EDDSA25519: hipLaunchKernelGGL(KERNEL<eced::EDDSA25519>, grid, block, 0, s, a); break;       \
	case eced::EDDSA25519CTX: hipLaunchKernelGGL(KERNEL<eced::EDDSA25519CTX>, grid, block, 0, s, a); break; \
	case eced::EDDSA25519PH: hipLaunchKernelGGL(KERNEL<eced::EDDSA25519PH>, grid, block, 0, s, a); break;   \
	case eced::EDDSA448: hipLaunchKernelGGL(KERNEL<eced::EDDSA448>, grid, block, 0, s, a); break;           \
	case eced::EDDSA448PH: hipLaunchKernelGGL(KERNEL<eced::EDDSA448PH>, grid, block, 0, s, a); break;       \
	default: return hipErrorInvalidValue;                                                                   \
	}

static bool eds_args_ok(int alg, const EcamdEddsaSignArgs &a)
{
	return eced::alg_ok(alg) && a.dom_len <= (uint32_t)eced::MAX_DOM && (!a.slots || (a.stride >= 4 && !(a.stride & 3u) && a.stride <= 4096));
}

hipError_t ecamd_launch_eddsa_expand(int alg, const EcamdEddsaSignArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!eds_args_ok(alg, a) || !a.sk || !a.a || (a.slots && (!a.r_hash || !a.bad || (eced::alg_is_ph(alg) && !a.ph)))) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	EDS_DISPATCH(k_eddsa_expand_r)
	return hipGetLastError();
}

hipError_t ecamd_launch_eddsa_hram(int alg, const EcamdEddsaSignArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!eds_args_ok(alg, a) || !a.R || !a.A || !a.hram || !a.sigs || (eced::alg_is_ph(alg) ? !a.ph : !a.slots)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	EDS_DISPATCH(k_eddsa_hram)
	return hipGetLastError();
}

hipError_t ecamd_launch_eddsa_sign_fin(int alg, const EcamdEddsaSignArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!eced::alg_ok(alg) || !a.bad || !a.stR || !a.S || !a.sigs || !a.status) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	if (eced::alg_is448(alg)) {
		hipLaunchKernelGGL(k_eddsa_sign_fin<57>, grid, block, 0, s, a);
	} else {
		hipLaunchKernelGGL(k_eddsa_sign_fin<32>, grid, block, 0, s, a);
	}
	return hipGetLastError();
}
