// libecc_amd/csrc/ecamd_schnorr.h -- the per-item steps of BIP0340 and ECFSDSA around their multiplications and their hash.
//
// The two Schnorr-type schemes with a POINT commitment: the signature carries the commitment itself (BIP0340: its x, ECFSDSA: both
// coordinates), the hash comes BEFORE the multiplications, and the verifier compares the point it computes with the signature's
// bytes (paths relative to the reference's src/):
//
//   scheme                        r (bytes)            hash input                          verify                                  sign (nonce k)
//   BIP0340 sig/bip0340.c:383-560 R.x, clen            H(tag) || H(tag) || r || Y.x || m   Y: unique representative (infinity      R = [k]G; R.y odd: k <- q - k;
//           :161-371                                                                       fails), then the one with an even y;    Y.y odd: d <- q - d (0 < d < q);
//                                                                                          r < p, s < q; e = H mod q;              e = H mod q, s = k + e d
//                                                                                          R = [s]G + [q - e]Y finite, y even,
//                                                                                          R.x = r
//   ECFSDSA sig/ecfsdsa.c:404-607 W.x || W.y, 2 clen   r || m                              W.x, W.y < p, W on the curve, s in      W = [k]G, e = H mod q,
//           :120-386                                                                       [1, q - 1]; e = H mod q;                s = k + e x != 0 (x < q)
//                                                                                          W' = [s]G + [q - e]Y finite, = W
// e is the WHOLE digest as a big-endian integer mod q (nn_init_from_buf + nn_mod), whatever its size beside q's.  BIP0340 does not
// refuse s = 0 (bip0340.c:430-431 compares with q only).
//
// A message slot is a little-endian u32 length, then the hash input; the fields the device writes are blanks counted in the length:
//   BIP0340   H(tag) (hsize) || H(tag) (hsize) || r (clen) || Y.x (clen) || m
//   ECFSDSA   W.x || W.y (2 clen) || m
// Verification overwrites r (W) with the signature's own bytes and fills Y.x; signing fills both.
//
// Written against the `Ops` policy of ecamd_sigfam.h (one modulus q, Montgomery radix R of its word size), so the same text runs in
// the kernels (ecamd_schnorr_kernels.h) and on the host in tests/schnorr_items_host_shim.cpp.
#pragma once
#include "ecamd_sighash.h"

namespace ecschnorr {

// libecc's ec_alg_type numbers (lib_ecc_types.h), as include/libecc_amd.h exports them
enum : int { ALG_ECFSDSA = 5, ALG_BIP0340 = 20 };

ESF_FN bool alg_known(int alg)
{
	return alg == ALG_ECFSDSA || alg == ALG_BIP0340;
}

// bytes of the commitment in a signature: BIP0340_R_LEN (sig/bip0340.h), ECFSDSA_R_LEN (sig/ecfsdsa.h)
ESF_FN int r_len(int alg, int clen)
{
	return alg == ALG_BIP0340 ? clen : 2 * clen;
}

// ---- slot geometry: offsets inside the hash input (the slot's bytes after its length word) ----
ESF_FN int r_off(int alg, int hsize)
{
	return alg == ALG_BIP0340 ? 2 * hsize : 0;
}
// the blank for the key's x; -1: the scheme does not hash the key
ESF_FN int x_off(int alg, int hsize, int clen)
{
	return alg == ALG_BIP0340 ? 2 * hsize + clen : -1;
}
// the fixed fields in front of the message: the least a slot's length can be
ESF_FN int fixed_len(int alg, int hsize, int clen)
{
	return alg == ALG_BIP0340 ? 2 * hsize + 2 * clen : 2 * clen;
}
ESF_FN bool slot_ok(int alg, uint32_t len, uint32_t stride, int hsize, int clen)
{
	return stride >= 4u && len >= (uint32_t)fixed_len(alg, hsize, clen) && len <= stride - 4u;
}

// ---- bytes: big-endian strings of equal length ----
ESF_FN bool be_lt(const uint8_t *a, const uint8_t *b, int len)
{
	int lt = 0, decided = 0;   // no early exit: lanes stay together
	for (int i = 0; i < len; i++) {
		const int l = a[i] < b[i], g = a[i] > b[i];
		lt |= l & ~decided & 1;
		decided |= l | g;
	}
	return lt != 0;
}
ESF_FN bool be_eq(const uint8_t *a, const uint8_t *b, int len)
{
	uint32_t diff = 0;
	for (int i = 0; i < len; i++) {
		diff |= (uint32_t)(a[i] ^ b[i]);
	}
	return diff == 0;
}
ESF_FN bool be_is_odd(const uint8_t *a, int len)
{
	return (a[len - 1] & 1) != 0;
}

// ---- ranges ----
// a coordinate of the key or of the commitment: fp_import_from_buf refuses a value >= p
ESF_FN bool coord_ok(const uint8_t *c, const uint8_t *p_be, int clen)
{
	return be_lt(c, p_be, clen);
}
// s as loaded (any value below R): BIP0340 s < q (bip0340.c:430-431), ECFSDSA 0 < s < q (ecfsdsa.c:468-470)
template <class Ops> ESF_FN bool verify_s_ok(const Ops &ops, int alg, const typename Ops::F &s)
{
	return ops.lt_q(s) & (alg == ALG_BIP0340 || !ops.is_zero(s));
}
// the private key as loaded: BIP0340 0 < x < q (bip0340.c:229-232), ECFSDSA x < q (ecfsdsa.c:295-299)
template <class Ops> ESF_FN bool sign_key_ok(const Ops &ops, int alg, const typename Ops::F &x)
{
	return ops.lt_q(x) & (alg == ALG_ECFSDSA || !ops.is_zero(x));
}
// the nonce as loaded: k in [1, q - 1] (nn_get_random_mod's contract; BIP0340: H_nonce mod q, zero fails, bip0340.c:292-294)
template <class Ops> ESF_FN bool nonce_ok(const Ops &ops, const typename Ops::F &k)
{
	return ops.lt_q(k) & !ops.is_zero(k);
}

// ---- the even-y flip ----
// of a key (bip0340.c:542-547): out = the y of the representative with an even y; y < p, p odd, so an odd y is not 0 and p - y is
// a reduced, even value
ESF_FN void lift_y(uint8_t *out, const uint8_t *y, const uint8_t *p_be, int clen)
{
	const bool odd = be_is_odd(y, clen);
	int borrow = 0;
	for (int b = clen - 1; b >= 0; b--) {
		const int d = (int)p_be[b] - (int)y[b] - borrow;
		out[b] = odd ? (uint8_t)(d & 0xff) : y[b];
		borrow = d < 0;
	}
}
// of a scalar that goes with a point whose y is odd (_bip0340_set_scalar, bip0340.c:74-101): q - v, 0 stays 0
template <class Ops> ESF_FN typename Ops::F flip_scalar(const Ops &ops, const typename Ops::F &v, bool odd)
{
	return odd ? ops.neg(v) : v;
}

// ---- e and q - e from a digest ----
template <class Ops> ESF_FN typename Ops::F digest_e(const Ops &ops, const uint8_t *dg, int hsize)
{
	return ecsigfam::wide_mod(ops, dg, hsize, false);
}
// nn_mod_neg: (q - e) mod q, 0 for e = 0 (bip0340.c:541, ecfsdsa.c:594)
template <class Ops> ESF_FN typename Ops::F neg_e(const Ops &ops, const typename Ops::F &e)
{
	return ops.neg(e);
}

// ---- the signing formulas ----  x, k: plain, in range; e plain
// BIP0340: s = (k' + e d') mod q with k' = k or q - k by the parity of R.y, d' = x or q - x by the parity of Y.y (bip0340.c:235,
// :308, :342-343).  Never fails: the reference exports s as it is.
template <class Ops>
ESF_FN typename Ops::F bip0340_s(const Ops &ops, const typename Ops::F &x, const typename Ops::F &k, const typename Ops::F &e, bool y_odd,
				 bool r_odd)
{
	const typename Ops::F d = flip_scalar(ops, x, y_odd), kk = flip_scalar(ops, k, r_odd);
	return ops.add(kk, ops.mul(ops.mul(e, ops.r2()), d));
}
// ECFSDSA: s = (k + e x) mod q; false where s = 0 (ecfsdsa.c:326-350)
template <class Ops>
ESF_FN bool ecfsdsa_s(const Ops &ops, const typename Ops::F &x, const typename Ops::F &k, const typename Ops::F &e, typename Ops::F &s)
{
	s = ops.add(k, ops.mul(ops.mul(e, ops.r2()), x));
	return !ops.is_zero(s);
}

// ---- the acceptance tests on the affine bytes of a FINITE sum (x || y, 2 clen) against the signature's commitment ----
ESF_FN bool bip0340_accept(const uint8_t *W, const uint8_t *r, int clen)
{
	return !be_is_odd(W + clen, clen) & be_eq(W, r, clen);   // bip0340.c:558-564
}
ESF_FN bool ecfsdsa_accept(const uint8_t *W, const uint8_t *r, int clen)
{
	return be_eq(W, r, 2 * clen);                            // ecfsdsa.c:602-611
}
ESF_FN bool accept(int alg, const uint8_t *W, const uint8_t *r, int clen)
{
	return alg == ALG_BIP0340 ? bip0340_accept(W, r, clen) : ecfsdsa_accept(W, r, clen);
}

}  // namespace ecschnorr
