// libecc_amd/csrc/ecamd_recover.h -- the field-level steps of ECDSA public-key recovery.
//
// Replaces the arithmetic of __ecdsa_public_key_from_sig (sig/ecdsa_common.c:867-1049 of the reference) around its
// multiplications:
//   e = OS2I(h) >> max(0, 8 |h| - |q|) mod q                       :934-942
//   u = -(e r^-1) mod q, v = s r^-1 mod q                          :976-985
//   Y1 = [v](x, y1) + [u]G, Y2 = [v](x, y2) + [u]G                 :988-994  (three prj_pt_mul, two prj_pt_add)
// (x, y2) = -(x, y1), so with A = [u]G and B = [v](x, y1) the two keys are A + B and A - B: ONE variable-base and ONE
// fixed-base multiplication per item.  Both sums are chords through A with the same denominator x_B - x_A, whose inverse
// the caller shares among a group of items (Montgomery's trick); given it a sum costs 2M + 1S.  The chord does not exist
// where A or B is the point at infinity or x_A = x_B (A = +-B: a doubling and the point at infinity): recover_needs_redo
// marks those items for the complete formulas (k_recover_redo).
//
// Everything here is written against an `Ops` policy (mul, sqr, add, sub, neg on one modulus), so the same text runs on
// the device over the saturated Montgomery words of ecamd_field.h and on the host in tests/recover_host_shim.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECR_FN __host__ __device__ __forceinline__
#else
#define ECR_FN inline
#endif

namespace ecrecover {

// status bytes of a point result, as include/libecc_amd.h and ecamd_internal.h number them
enum : uint32_t { ST_OK = 0, ST_ERR = 1, ST_INF = 2, ST_REDO = 0xFE };

// The digest as the reference reads it (:934-942): the leading elen = min(|h|, qlen) bytes, shifted right by *rshift bits
// (0 .. 7) -- the same integer as OS2I(h) >> (8 |h| - |q|) when 8 |h| > |q|, and the whole digest otherwise.  The result is
// below 2^|q| < 2 q: one conditional subtraction of q is nn_mod.
ECR_FN int digest_window(int hlen, int qlen, int qbits, int *rshift)
{
	const int elen = hlen < qlen ? hlen : qlen;
	*rshift = (8 * hlen > qbits) ? (8 * elen - qbits) : 0;
	return elen;
}

// little-endian 32-bit words shifted right by 0 .. 31 bits
template <int NW> ECR_FN void shift_right(uint32_t (&v)[NW], int rshift)
{
	if (rshift > 0) {
#pragma unroll
		for (int j = 0; j < NW; j++) {
			const uint32_t hi = (j + 1 < NW) ? v[j + 1] : 0u;
			v[j] = (v[j] >> rshift) | (hi << (32 - rshift));
		}
	}
}

// big-endian comparison a >= b of byte strings of different lengths (r against p: qlen and clen differ on secp224k1)
ECR_FN bool be_geq(const uint8_t *a, int alen, const uint8_t *b, int blen)
{
	const int len = alen > blen ? alen : blen;
	int gt = 0, lt = 0;   // decided at the first differing byte from the top
	for (int k = 0; k < len; k++) {
		const int ia = k - (len - alen), ib = k - (len - blen);
		const uint32_t x = ia >= 0 ? a[ia] : 0u, y = ib >= 0 ? b[ib] : 0u;
		const int undecided = !(gt | lt);
		gt |= undecided & (x > y);
		lt |= undecided & (x < y);
	}
	return !lt;
}

// u = -(e r^-1), v = s r^-1 (mod q); rinv is r^-1 in whatever form makes ops.mul(plain, rinv) a plain residue
template <class Ops, class F> ECR_FN void recover_uv(const Ops &ops, const F &e, const F &s, const F &rinv, F &u, F &v)
{
	u = ops.neg(ops.mul(e, rinv));
	v = ops.mul(s, rinv);
}

// an item leaves the shared-denominator path when a summand is the point at infinity or the chord is vertical / a tangent
ECR_FN bool recover_needs_redo(uint32_t stA, uint32_t stB, bool same_x)
{
	return stA != ST_OK || stB != ST_OK || same_x;
}

// A + B and A - B for finite A = (xa, ya), B = (xb, yb) with xa != xb, given dinv = 1 / (xb - xa): 2M + 1S each
template <class Ops, class F>
ECR_FN void recover_sums(const Ops &ops, const F &xa, const F &ya, const F &xb, const F &yb, const F &dinv, F &x1, F &y1, F &x2, F &y2)
{
	const F sx = ops.add(xa, xb);
	// A + B: lambda = (yb - ya) / (xb - xa)
	const F l1 = ops.mul(ops.sub(yb, ya), dinv);
	x1 = ops.sub(ops.sqr(l1), sx);
	y1 = ops.sub(ops.mul(l1, ops.sub(xa, x1)), ya);
	// A - B = A + (xb, -yb): lambda = (-yb - ya) / (xb - xa)
	const F l2 = ops.mul(ops.neg(ops.add(yb, ya)), dinv);
	x2 = ops.sub(ops.sqr(l2), sx);
	y2 = ops.sub(ops.mul(l2, ops.sub(xa, x2)), ya);
}

}  // namespace ecrecover
