// libecc_amd/csrc/ecamd_recover_kernels.h -- the kernels of batched ECDSA public-key recovery around its two scalar
// multiplications (included at the end of ecamd_kernels.hip: they live on the saturated Montgomery words of ecamd_field.h and
// read the constant slots of that translation unit).
//
// Replaces __ecdsa_public_key_from_sig (sig/ecdsa_common.c:867-1049 of the reference), per item:
//   k_recover_prep   r, s in [1, q - 1] (:903-913); e (:934-942); r as a field element, fp_set_nn's r < p (:949, fp/fp.c:204-220);
//                    u = -(e / r), v = s / r mod q (:976-985), one inversion per group of items (Montgomery's trick)
//   k_y_from_x       (unchanged) aff_pt_y_from_x (:950); an r that is no abscissa "restarts" with r + 2q, which the comparison
//                    at :921 or fp_set_nn then refuses whatever its value: such an item returns -1
//   k_recover_point  (x, y1) as the affine point the variable-base pipeline takes
//   [u]G, [v](x, y1) the existing pipelines (:988-990); (x, y2) = -(x, y1), so [v](x, y2) is not computed
//   k_recover_fin    Y1 = [u]G + [v]R, Y2 = [u]G - [v]R (:990-994) as two chords with one shared denominator
//                    (ecamd_recover.h), the denominators of a lane's items inverted together
//   k_recover_redo   the items k_recover_fin marked (a summand at infinity, x_A = x_B) on the complete formulas
#pragma once
#include "ecamd_recover.h"

template <int NW> struct RecoverOps {
	int slot;
	__device__ __forceinline__ Fe<NW> mul(const Fe<NW> &a, const Fe<NW> &b) const { return fe_mul<NW>(a, b, slot); }
	__device__ __forceinline__ Fe<NW> sqr(const Fe<NW> &a) const { return fe_sqr<NW>(a, slot); }
	__device__ __forceinline__ Fe<NW> add(const Fe<NW> &a, const Fe<NW> &b) const { return fe_add<NW>(a, b, slot); }
	__device__ __forceinline__ Fe<NW> sub(const Fe<NW> &a, const Fe<NW> &b) const { return fe_sub<NW>(a, b, slot); }
	__device__ __forceinline__ Fe<NW> neg(const Fe<NW> &a) const { return fe_sub<NW>(fe_zero<NW>(), a, slot); }
};

// The prefix products of Montgomery's trick, K per lane, in LDS (word-major, lane-minor: no bank conflicts).  Kept in registers they
// spill to scratch (K x NW words per lane); a lane only reads what it wrote itself, so no barrier is needed.
template <int NW> static __device__ __forceinline__ void prefix_put(u32 *lds, int k, const Fe<NW> &a)
{
#pragma unroll
	for (int w = 0; w < NW; w++) {
		lds[(k * NW + w) * 64 + threadIdx.x] = a.v[w];
	}
}
template <int NW> static __device__ __forceinline__ Fe<NW> prefix_get(const u32 *lds, int k)
{
	Fe<NW> a;
#pragma unroll
	for (int w = 0; w < NW; w++) {
		a.v[w] = lds[(k * NW + w) * 64 + threadIdx.x];
	}
	return a;
}

// e = (OS2I(h) >> max(0, 8 |h| - |q|)) mod q (:934-942) through ecrecover::digest_window / shift_right
template <int NW> static __device__ __forceinline__ Fe<NW> recover_e(const u8 *dg, int hlen, int qlen, int qbits, int qs)
{
	int rshift = 0;
	const int elen = ecrecover::digest_window(hlen, qlen, qbits, &rshift);
	Fe<NW> e = fe_load_be<NW>(dg, elen);
	ecrecover::shift_right<NW>(e.v, rshift);
	u32 qw[NW];
#pragma unroll
	for (int j = 0; j < NW; j++) {
		qw[j] = ConstTab<NW>::get(qs).p[j];
	}
	return fe_cond_sub<NW>(e.v, 0u, qw);   // e < 2^|q| < 2q: one conditional subtraction is nn_mod
}

// One lane prepares KP consecutive items and shares one inversion mod q among them, as k_ecdsa_prep does; NW = words of q.
template <int NW> __global__ __launch_bounds__(64) void k_recover_prep(EcamdRecoverPrepArgs A)
{
	constexpr int KP = ecdsa_prep_items(NW);
	const u32 t = blockIdx.x * 64 + threadIdx.x;
	const u32 first = t * KP;
	if (first >= A.n) {
		return;
	}
	const int qs = A.qslot;
	const int qlen = (int)A.qlen, clen = (int)A.clen, hlen = (int)A.hlen;
	const RecoverOps<NW> ops{qs};
	const Fe<NW> one = fe_const<NW>(ConstTab<NW>::get(qs).one);
	__shared__ u32 pre[KP * NW * 64];   // entry k = r_0 ... r_k (Montgomery form)
	u32 okmask = 0;
	Fe<NW> acc = one;
#pragma unroll
	for (int k = 0; k < KP; k++) {
		const u32 i = first + k;
		if (i < A.n) {
			const u8 *sig = A.sigs + (size_t)i * 2 * qlen;
			const Fe<NW> r = fe_load_be<NW>(sig, qlen), sv = fe_load_be<NW>(sig + qlen, qlen);
			const bool ok = !fe_is_zero<NW>(r) & !fe_is_zero<NW>(sv) & fe_lt_p<NW>(r, qs) & fe_lt_p<NW>(sv, qs);
			okmask |= ok ? (1u << k) : 0u;
			acc = fe_mul<NW>(acc, ok ? fe_to_mont<NW>(r, qs) : one, qs);
		}
		prefix_put<NW>(pre, k, acc);
	}
	// (r_0 ... r_last)^-1 = x^(q-2) (q prime): the unique inverse, equal to nn_modinv's (:981)
	Fe<NW> inv = fe_inv<NW>(acc, qs);
#pragma unroll
	for (int k = KP - 1; k >= 0; k--) {
		const u32 i = first + k;
		if (i >= A.n) {
			continue;
		}
		const bool ok = (okmask >> k) & 1u;
		const u8 *sig = A.sigs + (size_t)i * 2 * qlen;
		const Fe<NW> r = fe_load_be<NW>(sig, qlen), sv = fe_load_be<NW>(sig + qlen, qlen);
		const Fe<NW> rm = ok ? fe_to_mont<NW>(r, qs) : one;
		const Fe<NW> rinv = (k > 0) ? fe_mul<NW>(inv, prefix_get<NW>(pre, k - 1), qs) : inv;   // Montgomery form of 1 / r_k
		inv = fe_mul<NW>(inv, rm, qs);
		const Fe<NW> e = recover_e<NW>(A.digests + (size_t)i * hlen, hlen, qlen, (int)A.qbits, qs);
		Fe<NW> u, v;
		ecrecover::recover_uv(ops, e, sv, rinv, u, v);   // plain * Montgomery = plain
		// fp_set_nn refuses r >= p (q > p: secp224k1)
		const bool good = ok & !ecrecover::be_geq(sig, qlen, A.p_be, clen);
		fe_store_be<NW>(A.u + (size_t)i * qlen, qlen, good ? u : fe_zero<NW>());
		fe_store_be<NW>(A.v + (size_t)i * qlen, qlen, good ? v : fe_zero<NW>());
		u8 *x = A.x + (size_t)i * clen;
		for (int b = 0; b < clen; b++) {
			const int src = qlen - clen + b;
			x[b] = (good && src >= 0) ? sig[src] : (u8)0;
		}
		A.flags[i] = good ? 0 : 1;
	}
}

// R = (x, y1) for the variable-base multiplication; (0, 0) -- not on any curve with b != 0 -- for the items that have none
__global__ __launch_bounds__(256) void k_recover_point(EcamdRecoverPointArgs A)
{
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	const u32 plen = 2 * A.clen;
	if (t >= (size_t)A.n * plen) {
		return;
	}
	const u32 i = (u32)(t / plen), b = (u32)(t % plen);
	const bool good = (A.flags[i] | A.yst[i]) == 0;
	const u8 *src = b < A.clen ? A.x + (size_t)i * A.clen + b : A.y1 + (size_t)i * A.clen + (b - A.clen);
	A.R[t] = good ? *src : (u8)0;
}

template <int NW> static __device__ __forceinline__ void recover_store_none(const EcamdRecoverFinArgs &A, u32 i, u8 st)
{
	const int plen = 2 * (int)A.clen;
	u8 *o1 = A.out1 + (size_t)i * plen, *o2 = A.out2 + (size_t)i * plen;
	for (int b = 0; b < plen; b++) {
		o1[b] = 0;
		o2[b] = 0;
	}
	A.st1[i] = st;
	A.st2[i] = st;
}

#define ECAMD_RECOVER_FIN_K 8
// One lane finishes ECAMD_RECOVER_FIN_K consecutive items: the denominators x_B - x_A of its items are inverted together.
template <int NW> __global__ __launch_bounds__(64) void k_recover_fin(EcamdRecoverFinArgs A)
{
	constexpr int KF = ECAMD_RECOVER_FIN_K;
	const u32 t = blockIdx.x * 64 + threadIdx.x;
	const u32 first = t * KF;
	if (first >= A.n) {
		return;
	}
	const int slot = A.slot, clen = (int)A.clen;
	const RecoverOps<NW> ops{slot};
	const Fe<NW> one = fe_const<NW>(ConstTab<NW>::get(slot).one);
	__shared__ u32 pre[KF * NW * 64];
	u32 fast = 0, none = 0, errs = 0;   // per item: on the shared-denominator path / without a key from this kernel / of those, the reference's -1
	Fe<NW> acc = one;
#pragma unroll
	for (int k = 0; k < KF; k++) {
		const u32 i = first + k;
		if (i < A.n) {
			const u32 sa = A.stA[i], sb = A.stB[i];
			const bool err = (A.flags[i] | A.yst[i]) != 0 || sa == ecrecover::ST_ERR || sb == ecrecover::ST_ERR;
			const Fe<NW> xa = fe_load_be<NW>(A.A + (size_t)i * 2 * clen, clen), xb = fe_load_be<NW>(A.B + (size_t)i * 2 * clen, clen);
			const bool redo = ecrecover::recover_needs_redo(sa, sb, fe_eq<NW>(xa, xb));
			const bool go = !err & !redo;
			fast |= go ? (1u << k) : 0u;
			none |= go ? 0u : (1u << k);
			errs |= err ? (1u << k) : 0u;
			acc = fe_mul<NW>(acc, go ? fe_to_mont<NW>(fe_sub<NW>(xb, xa, slot), slot) : one, slot);
		}
		prefix_put<NW>(pre, k, acc);
	}
	// no key from this kernel: the reference returns -1 (ECAMD_ERR), or the item waits for k_recover_redo
	for (int k = 0; k < KF; k++) {
		if ((none >> k) & 1u) {
			recover_store_none<NW>(A, first + k, ((errs >> k) & 1u) ? (u8)ecrecover::ST_ERR : (u8)ecrecover::ST_REDO);
		}
	}
	if (fast == 0) {
		return;
	}
	Fe<NW> inv = fe_inv<NW>(acc, slot);
#pragma unroll
	for (int k = KF - 1; k >= 0; k--) {
		if (!((fast >> k) & 1u)) {
			continue;   // entry k == entry k - 1: the item took no part in the product
		}
		const u32 i = first + k;
		const u8 *pa = A.A + (size_t)i * 2 * clen, *pb = A.B + (size_t)i * 2 * clen;
		const Fe<NW> xa = fe_to_mont<NW>(fe_load_be<NW>(pa, clen), slot), ya = fe_to_mont<NW>(fe_load_be<NW>(pa + clen, clen), slot);
		const Fe<NW> xb = fe_to_mont<NW>(fe_load_be<NW>(pb, clen), slot), yb = fe_to_mont<NW>(fe_load_be<NW>(pb + clen, clen), slot);
		const Fe<NW> dinv = (k > 0) ? fe_mul<NW>(inv, prefix_get<NW>(pre, k - 1), slot) : inv;
		inv = fe_mul<NW>(inv, fe_sub<NW>(xb, xa, slot), slot);
		Fe<NW> x1, y1, x2, y2;
		ecrecover::recover_sums(ops, xa, ya, xb, yb, dinv, x1, y1, x2, y2);
		u8 *o1 = A.out1 + (size_t)i * 2 * clen, *o2 = A.out2 + (size_t)i * 2 * clen;
		fe_store_be<NW>(o1, clen, fe_from_mont<NW>(x1, slot));
		fe_store_be<NW>(o1 + clen, clen, fe_from_mont<NW>(y1, slot));
		fe_store_be<NW>(o2, clen, fe_from_mont<NW>(x2, slot));
		fe_store_be<NW>(o2 + clen, clen, fe_from_mont<NW>(y2, slot));
		A.st1[i] = (u8)ecrecover::ST_OK;
		A.st2[i] = (u8)ecrecover::ST_OK;
	}
}

// the unique representative of W (or zero bytes) and its status
template <int NW> static __device__ __forceinline__ void recover_store_pt(u8 *out, u8 *status, const Pt<NW> &W, int clen, int slot)
{
	if (fe_is_zero<NW>(W.Z)) {
		for (int b = 0; b < 2 * clen; b++) {
			out[b] = 0;
		}
		*status = (u8)ecrecover::ST_INF;
		return;
	}
	const Fe<NW> zi = fe_inv<NW>(W.Z, slot);
	fe_store_be<NW>(out, clen, fe_from_mont<NW>(fe_mul<NW>(W.X, zi, slot), slot));
	fe_store_be<NW>(out + clen, clen, fe_from_mont<NW>(fe_mul<NW>(W.Y, zi, slot), slot));
	*status = (u8)ecrecover::ST_OK;
}

// The marked items alone (every other lane exits at once): prj_pt_add of the reference's complete formulas on A and +-B, either
// of which may be the point at infinity; an "exceptional pair" (curves/prj_pt.c:1058-1060) is the reference's -1 for the item.
template <int NW> __global__ __launch_bounds__(64) void k_recover_redo(EcamdRecoverFinArgs A)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n || A.st1[i] != ECAMD_STATUS_REDO) {
		return;
	}
	const int slot = A.slot, clen = (int)A.clen;
	const Fe<NW> one = fe_const<NW>(ConstTab<NW>::get(slot).one);
	Pt<NW> P = pt_infinity<NW>(slot), Q = P;
	if (A.stA[i] == ecrecover::ST_OK) {
		const u8 *pa = A.A + (size_t)i * 2 * clen;
		P.X = fe_to_mont<NW>(fe_load_be<NW>(pa, clen), slot);
		P.Y = fe_to_mont<NW>(fe_load_be<NW>(pa + clen, clen), slot);
		P.Z = one;
	}
	if (A.stB[i] == ecrecover::ST_OK) {
		const u8 *pb = A.B + (size_t)i * 2 * clen;
		Q.X = fe_to_mont<NW>(fe_load_be<NW>(pb, clen), slot);
		Q.Y = fe_to_mont<NW>(fe_load_be<NW>(pb + clen, clen), slot);
		Q.Z = one;
	}
	const Pt<NW> W1 = pt_add<NW>(Q, P, slot);
	Q.Y = fe_sub<NW>(fe_zero<NW>(), Q.Y, slot);
	const Pt<NW> W2 = pt_add<NW>(Q, P, slot);
	if ((fe_is_zero<NW>(W1.Z) && fe_is_zero<NW>(W1.Y)) || (fe_is_zero<NW>(W2.Z) && fe_is_zero<NW>(W2.Y))) {
		recover_store_none<NW>(A, i, (u8)ecrecover::ST_ERR);
		return;
	}
	recover_store_pt<NW>(A.out1 + (size_t)i * 2 * clen, A.st1 + i, W1, clen, slot);
	recover_store_pt<NW>(A.out2 + (size_t)i * 2 * clen, A.st2 + i, W2, clen, slot);
}

hipError_t ecamd_launch_recover_prep(int qnw, const EcamdRecoverPrepArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	const uint32_t kp = (uint32_t)ecdsa_prep_items(qnw);
	const uint32_t lanes = (a.n + kp - 1) / kp;
	const dim3 grid((lanes + 63) / 64), block(64);
	switch (qnw) {
#define X(N) case N: hipLaunchKernelGGL(k_recover_prep<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t ecamd_launch_recover_point(const EcamdRecoverPointArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	const size_t bytes = (size_t)a.n * 2 * a.clen;
	hipLaunchKernelGGL(k_recover_point, dim3((unsigned)((bytes + 255) / 256)), dim3(256), 0, s, a);
	return hipGetLastError();
}

hipError_t ecamd_launch_recover_fin(int nw, const EcamdRecoverFinArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	const uint32_t lanes = (a.n + ECAMD_RECOVER_FIN_K - 1) / ECAMD_RECOVER_FIN_K;
	const dim3 grid((lanes + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_recover_fin<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t ecamd_launch_recover_redo(int nw, const EcamdRecoverFinArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_recover_redo<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
