// libecc_amd/csrc/ecamd_sigfam_kernels.h -- the kernels of batched ECGDSA, ECRDSA and SM2 around their multiplications (included
// at the end of ecamd_kernels.hip: they live on the saturated Montgomery words of ecamd_field.h, modulus q in a constant slot).
//
//   k_sig_prep   the verification front end, beside k_ecdsa_prep: ranges of r and s, e by the scheme's rule, the multipliers of
//                G and Y, the flag byte and the COMPARISON TARGET r* (ecamd_sigfam.h) in the layout of a signature array -- item
//                i's target lies where its r would -- so that k_ecdsa_fin and the interleaved secp256r1 loop compare W'.x with
//                it unchanged.  One inversion per group of items for ECGDSA (r) and ECRDSA (e), none for SM2.
//   k_sig_sign   the signing back end, beside k_ecdsa_sign: r and s from [k]G by the scheme's rule
#pragma once
#include "ecamd_sigfam.h"

template <int NW> struct SigfamOps {
	typedef Fe<NW> F;
	enum { WORDS = NW };
	int qs;
	__device__ __forceinline__ F mul(const F &a, const F &b) const { return fe_mul<NW>(a, b, qs); }
	__device__ __forceinline__ F add(const F &a, const F &b) const { return fe_add<NW>(a, b, qs); }
	__device__ __forceinline__ F sub(const F &a, const F &b) const { return fe_sub<NW>(a, b, qs); }
	__device__ __forceinline__ F neg(const F &a) const { return fe_sub<NW>(fe_zero<NW>(), a, qs); }
	__device__ __forceinline__ F zero() const { return fe_zero<NW>(); }
	__device__ __forceinline__ F r2() const { return fe_const<NW>(ConstTab<NW>::get(qs).r2); }
	__device__ __forceinline__ bool is_zero(const F &a) const { return fe_is_zero<NW>(a); }
	__device__ __forceinline__ bool lt_q(const F &a) const { return fe_lt_p<NW>(a, qs); }
	__device__ __forceinline__ F load_be(const u8 *p, int len) const { return fe_load_be<NW>(p, len); }
	__device__ __forceinline__ F load_le(const u8 *p, int len) const { return fe_load_le<NW>(p, len); }
	__device__ __forceinline__ F shr(F a, int n) const
	{
		ecrecover::shift_right<NW>(a.v, n);
		return a;
	}
};

#define ECAMD_SIG_PREP_K 8   // items per shared inversion: 8 x NW x 64 words of LDS for the prefix products (34 KB at 17 words)

template <int NW> __global__ __launch_bounds__(64) void k_sig_prep(EcamdSigPrepArgs S)
{
	constexpr int KP = ECAMD_SIG_PREP_K;
	const EcamdEcdsaPrepArgs &A = S.p;
	const u32 t = blockIdx.x * 64 + threadIdx.x;
	const u32 first = t * KP;
	if (first >= A.n) {
		return;
	}
	if (A.only != nullptr) {
		// redo pass: nothing to do unless one of the lane's items is marked
		bool any = false;
		for (int k = 0; k < KP; k++) {
			any = any | (first + k < A.n && A.only[first + k] == ECAMD_STATUS_REDO);
		}
		if (!any) {
			return;
		}
	}
	const int alg = S.alg;
	const int qs = A.qslot;
	const int qlen = (int)A.qlen, hlen = (int)A.hlen, qbits = (int)A.qbits;
	const SigfamOps<NW> ops{qs};
	const Fe<NW> one = fe_const<NW>(ConstTab<NW>::get(qs).one);
	const bool inverts = ecsigfam::verify_inverts(alg);   // wave-uniform
	__shared__ u32 pre[KP * NW * 64];   // entry k = d_0 ... d_k (Montgomery form), d the scheme's divisor
	u32 okmask = 0;
	Fe<NW> inv = one;
	if (inverts) {
		Fe<NW> acc = one;
#pragma unroll 1
		for (int k = 0; k < KP; k++) {
			const u32 i = first + k;
			if (i < A.n) {
				const u8 *sig = A.sigs + (size_t)i * 2 * qlen;
				const Fe<NW> r = fe_load_be<NW>(sig, qlen), sv = fe_load_be<NW>(sig + qlen, qlen);
				const bool ok = ecsigfam::verify_ranges(ops, r, sv);
				okmask |= ok ? (1u << k) : 0u;
				if (ok) {
					const Fe<NW> e = alg == ecsigfam::ALG_ECRDSA
								 ? ecsigfam::digest_e(ops, alg, A.digests + (size_t)i * hlen, hlen, qlen, qbits)
								 : fe_zero<NW>();
					acc = fe_mul<NW>(acc, fe_to_mont<NW>(ecsigfam::verify_divisor(ops, alg, r, e), qs), qs);
				}
			}
			prefix_put<NW>(pre, k, acc);
		}
		// (d_0 ... d_last)^-1 = x^(q-2) (q prime): the unique inverse, equal to nn_modinv's
		inv = fe_inv<NW>(acc, qs);
	}
#pragma unroll 1
	for (int k = KP - 1; k >= 0; k--) {
		const u32 i = first + k;
		if (i >= A.n) {
			continue;
		}
		const u8 *sig = A.sigs + (size_t)i * 2 * qlen;
		const Fe<NW> r = fe_load_be<NW>(sig, qlen), sv = fe_load_be<NW>(sig + qlen, qlen);
		bool ok = inverts ? (((okmask >> k) & 1u) != 0) : ecsigfam::verify_ranges(ops, r, sv);
		const Fe<NW> e = ecsigfam::digest_e(ops, alg, A.digests + (size_t)i * hlen, hlen, qlen, qbits);
		Fe<NW> dinv = one;
		if (inverts && ok) {
			dinv = (k > 0) ? fe_mul<NW>(inv, prefix_get<NW>(pre, k - 1), qs) : inv;   // Montgomery form of 1 / d_k
			inv = fe_mul<NW>(inv, fe_to_mont<NW>(ecsigfam::verify_divisor(ops, alg, r, e), qs), qs);
		}
		Fe<NW> u = fe_zero<NW>(), v = fe_zero<NW>(), tg = fe_zero<NW>();
		if (ok) {
			ok = ecsigfam::verify_uv(ops, alg, r, sv, e, dinv, u, v, tg);
		}
		fe_store_be<NW>(A.u1 + (size_t)i * qlen, qlen, ok ? u : fe_zero<NW>());
		fe_store_be<NW>(A.u2 + (size_t)i * qlen, qlen, ok ? v : fe_zero<NW>());
		fe_store_be<NW>(S.target + (size_t)i * 2 * qlen, qlen, ok ? tg : fe_zero<NW>());
		A.flags[i] = ok ? 0 : 1;
	}
}

// One item per lane.  status 1: what sign_key_ok refuses, k not in [1, q - 1], [k]G not a finite point, or one of the
// reference's restart conditions (ecsigfam::sign_rs), which a fixed nonce cannot get past.
template <int NW> __global__ __launch_bounds__(64) void k_sig_sign(EcamdSigSignArgs S)
{
	const EcamdEcdsaSignArgs &A = S.a;
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int alg = S.alg;
	const int qs = A.qslot;
	const int qlen = (int)A.qlen, clen = (int)A.clen;
	const SigfamOps<NW> ops{qs};
	const CurveK<NW> &Q = ConstTab<NW>::get(qs);
	u32 qw[NW];
#pragma unroll
	for (int j = 0; j < NW; j++) {
		qw[j] = Q.p[j];
	}
	const Fe<NW> x = fe_load_be<NW>(A.privs + (size_t)i * qlen, qlen);
	const Fe<NW> kk = fe_load_be<NW>(A.nonces + (size_t)i * qlen, qlen);
	bool ok = ecsigfam::sign_key_ok(ops, alg, x) & !fe_is_zero<NW>(kk) & fe_lt_p<NW>(kk, qs) & (A.stkG[i] == 0);
	// [k]G.x mod q: x < p <= (jmax + 1) q, so jmax conditional subtractions
	Fe<NW> wx = fe_load_be<NW>(A.kG + (size_t)i * 2 * clen, clen);
	for (u32 j = 0; j < A.jmax; j++) {
		wx = fe_cond_sub<NW>(wx.v, 0u, qw);
	}
	const Fe<NW> e = ecsigfam::digest_e(ops, alg, A.digests + (size_t)i * A.hlen, (int)A.hlen, qlen, (int)A.qbits);
	Fe<NW> xinv = fe_const<NW>(Q.one);
	if (ecsigfam::sign_inverts(alg)) {   // wave-uniform
		Fe<NW> onep = fe_zero<NW>();
		onep.v[0] = 1;
		const Fe<NW> d = ok ? fe_add<NW>(x, onep, qs) : onep;
		xinv = fe_inv<NW>(fe_to_mont<NW>(d, qs), qs);   // Montgomery form of 1 / (1 + x)
	}
	Fe<NW> r = fe_zero<NW>(), sv = fe_zero<NW>();
	if (ok) {
		ok = ecsigfam::sign_rs(ops, alg, x, kk, e, wx, xinv, r, sv);
	}
	u8 *sig = A.sigs + (size_t)i * 2 * qlen;
	fe_store_be<NW>(sig, qlen, ok ? r : fe_zero<NW>());
	fe_store_be<NW>(sig + qlen, qlen, ok ? sv : fe_zero<NW>());
	A.status[i] = ok ? 0 : 1;
}

hipError_t ecamd_launch_sig_prep(int nw, const EcamdSigPrepArgs &a, hipStream_t s)
{
	if (a.p.n == 0) {
		return hipSuccess;
	}
	if (!ecsigfam::alg_known(a.alg)) {
		return hipErrorInvalidValue;
	}
	const uint32_t lanes = (a.p.n + ECAMD_SIG_PREP_K - 1) / ECAMD_SIG_PREP_K;
	const dim3 grid((lanes + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_sig_prep<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t ecamd_launch_sig_sign(int nw, const EcamdSigSignArgs &a, hipStream_t s)
{
	if (a.a.n == 0) {
		return hipSuccess;
	}
	if (!ecsigfam::alg_known(a.alg)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.a.n + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_sig_sign<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
