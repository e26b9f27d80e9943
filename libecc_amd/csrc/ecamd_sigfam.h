// libecc_amd/csrc/ecamd_sigfam.h -- the mod-q steps of ECGDSA, ECRDSA and SM2 around their multiplications.
//
// The three schemes have the shape of ECDSA: verification is range checks, a little algebra mod q that yields two public
// multipliers, W' = [u]G + [v]Y, and a comparison of W'.x mod q; signing is [k]G and algebra with the private key
// (paths relative to the reference's src/):
//
//   scheme                       e from the digest bytes                     verify: u, v          accept iff              sign (nonce k)
//   ECGDSA sig/ecgdsa.c:500-612  big-endian, leftmost |q| bits, mod q        e/r, s/r              W'.x mod q = r          r = [k]G.x mod q, s = x (k r - e)
//          :181-376              (ECDSA's rule)
//   ECRDSA sig/ecrdsa.c:498-614  BYTE-REVERSED (default build), the whole    s/e, -r/e             W'.x mod q = r          r = [k]G.x mod q, s = r x + k e
//          :196-378              digest mod q, 0 becomes 1
//   SM2    sig/sm2.c:610-715     big-endian, the whole digest mod q          s, t = r + s (t != 0) (e + W'.x) mod q = r    r = e + [k]G.x, s = (k - r x) / (1 + x)
//          :310-483
//
// The back ends of ECDSA verification test W'.x = r* (mod q) for a value r* they read where the signature's r lies; here r* is
// the COMPARISON TARGET the front end writes: r for ECGDSA and ECRDSA, (r - e) mod q for SM2.  r >= q is flagged as rejected
// for all three: _ecrdsa_verify_init (:446-450) compares s with q twice and never r, and such an r is only refused by the final
// comparison (r' < q <= r) -- a back end that tries the candidates r + j q < p would accept r + q if it were handed on.
//
// Everything is written against an `Ops` policy on ONE modulus q with the Montgomery radix R of its word size:
//   F, WORDS                 an element: WORDS little-endian 32-bit words v[]; R = 2^(32 WORDS)
//   mul(a, b)                a b / R mod q; one operand may be any value below R, the other is below q
//   add, sub, neg            on values below q
//   zero(), r2()             0, R^2 mod q
//   is_zero(a), lt_q(a)      a == 0, a < q (a: any value below R)
//   load_be / load_le        up to 4 NW bytes as a big- / little-endian integer, not reduced
//   shr(a, n)                a >> n, n in 0 .. 31
// so the same text runs in the kernels over the saturated words of ecamd_field.h (ecamd_sigfam_kernels.h) and on the host in
// tests/sig_family_host_shim.cpp.  "plain" below is a residue below q, "Montgomery form of a" is a R mod q; mul(plain,
// Montgomery form) is plain.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ESF_FN __host__ __device__ __forceinline__
#else
#define ESF_FN inline
#endif

namespace ecsigfam {

// libecc's ec_alg_type numbers (lib_ecc_types.h), as include/libecc_amd.h exports them
enum : int { ALG_ECDSA = 1, ALG_ECGDSA = 6, ALG_ECRDSA = 7, ALG_SM2 = 8 };

ESF_FN bool alg_known(int alg)
{
	return alg == ALG_ECGDSA || alg == ALG_ECRDSA || alg == ALG_SM2;
}

// a value below R reduced to a plain residue: (a R) / R
template <class Ops> ESF_FN typename Ops::F reduce(const Ops &ops, const typename Ops::F &a)
{
	typename Ops::F one = ops.zero();
	one.v[0] = 1;
	return ops.mul(ops.mul(a, ops.r2()), one);
}

// The integer of hlen (1 .. 128) digest bytes, big-endian or little-endian (= the bytes reversed, then big-endian), mod q.
// Horner over chunks of one element's bytes (the chunk base is R) from the top: acc <- acc R + chunk, in Montgomery form so
// that each step is one multiplication by R^2 for the shift, one for the chunk and an addition; the result is plain.
template <class Ops> ESF_FN typename Ops::F wide_mod(const Ops &ops, const uint8_t *dg, int hlen, bool little_endian)
{
	typedef typename Ops::F F;
	constexpr int cb = 4 * Ops::WORDS;
	const int nchunks = (hlen + cb - 1) / cb;
	const F r2 = ops.r2();
	F acc = ops.zero();   // Montgomery form of the value so far
	for (int c = nchunks - 1; c >= 0; c--) {
		// chunk c holds the integer's bits [8 cb c, 8 cb (c + 1))
		const int lo = c * cb, hi = (lo + cb < hlen) ? lo + cb : hlen;
		const F chunk = little_endian ? ops.load_le(dg + lo, hi - lo) : ops.load_be(dg + (hlen - hi), hi - lo);
		acc = ops.add(ops.mul(acc, r2), ops.mul(chunk, r2));
	}
	F one = ops.zero();
	one.v[0] = 1;
	return ops.mul(acc, one);
}

// e of the scheme (plain).  ECGDSA: ecgdsa.c:551-563 (the leading min(hlen, qlen) bytes shifted right so that |q| bits stay
// when the digest is longer than q -- below 2^|q|, any multiple of q taken off by reduce()).  ECRDSA: ecrdsa.c:545-556.
// SM2: sm2.c:663-666.
template <class Ops> ESF_FN typename Ops::F digest_e(const Ops &ops, int alg, const uint8_t *dg, int hlen, int qlen, int qbits)
{
	typedef typename Ops::F F;
	if (alg == ALG_ECGDSA) {
		const int elen = hlen < qlen ? hlen : qlen;
		const int rshift = (8 * hlen > qbits) ? (8 * elen - qbits) : 0;   // 0 .. 7
		return reduce(ops, ops.shr(ops.load_be(dg, elen), rshift));
	}
	F e = wide_mod(ops, dg, hlen, alg == ALG_ECRDSA);
	if (alg == ALG_ECRDSA && ops.is_zero(e)) {
		e.v[0] = 1;   // "If h is equal to 0, set it to 1" (ecrdsa.c:553-556, :312-315)
	}
	return e;
}

// r and s of a signature as loaded (any value below R): both in [1, q - 1]
template <class Ops> ESF_FN bool verify_ranges(const Ops &ops, const typename Ops::F &r, const typename Ops::F &s)
{
	return !ops.is_zero(r) & !ops.is_zero(s) & ops.lt_q(r) & ops.lt_q(s);
}

// does the scheme's verification divide at all (SM2 does not)
ESF_FN bool verify_inverts(int alg)
{
	return alg != ALG_SM2;
}

// the value the verification divides by (plain, non-zero for an item in range): r for ECGDSA, e for ECRDSA
template <class Ops>
ESF_FN typename Ops::F verify_divisor(const Ops &, int alg, const typename Ops::F &r, const typename Ops::F &e)
{
	return alg == ALG_ECGDSA ? r : e;
}

// The multipliers of G and Y and the comparison target for an item whose r and s are in range; dinv is the Montgomery form of
// 1 / verify_divisor (unused for SM2).  Returns false where the scheme rejects here (SM2: t = 0, sm2.c:656-660).
template <class Ops>
ESF_FN bool verify_uv(const Ops &ops, int alg, const typename Ops::F &r, const typename Ops::F &s, const typename Ops::F &e,
		      const typename Ops::F &dinv, typename Ops::F &u, typename Ops::F &v, typename Ops::F &target)
{
	if (alg == ALG_ECGDSA) {
		u = ops.mul(e, dinv);   // ecgdsa.c:566-572
		v = ops.mul(s, dinv);
		target = r;
		return true;
	}
	if (alg == ALG_ECRDSA) {
		u = ops.mul(s, dinv);   // ecrdsa.c:557-570
		v = ops.neg(ops.mul(r, dinv));
		target = r;
		return true;
	}
	u = s;                          // sm2.c:656-672
	v = ops.add(r, s);
	target = ops.sub(r, e);         // (e + W'.x) mod q == r  <=>  W'.x mod q == (r - e) mod q
	return !ops.is_zero(v);
}

// ---- signing ----
// the private key as loaded: what ec_key_pair_import_from_priv_key_buf and the scheme's signing accept.  x < q for ECGDSA
// (ecgdsa.c:48, :227-231; its public key [1/x]G also needs x != 0) and ECRDSA (ecrdsa.c:86, :240-244; x = 0 signs); x < q - 1
// for SM2 (sm2.c:72-75: 1 + x must be invertible), and x != 0: the public key [0]G has no affine form for Z (sm2.c:195), so
// _ec_sign returns -1.
template <class Ops> ESF_FN bool sign_key_ok(const Ops &ops, int alg, const typename Ops::F &x)
{
	typedef typename Ops::F F;
	if (!ops.lt_q(x)) {
		return false;
	}
	if (alg == ALG_ECGDSA) {
		return !ops.is_zero(x);
	}
	if (alg == ALG_SM2) {
		F one = ops.zero();
		one.v[0] = 1;
		return !ops.is_zero(x) & !ops.is_zero(ops.add(x, one));
	}
	return true;
}

// does the scheme's signing divide (SM2 only: by 1 + x)
ESF_FN bool sign_inverts(int alg)
{
	return alg == ALG_SM2;
}

// (r, s) from x, k (both plain, in range), e and wx = [k]G.x mod q (plain); xinv: Montgomery form of 1 / (1 + x), SM2 only.
// Returns false where the reference restarts, which a fixed nonce cannot get past: r = 0 (ecgdsa.c:312, ecrdsa.c:288,
// sm2.c:401) or s = 0 (ecgdsa.c:340, ecrdsa.c:338, sm2.c:448).  SM2's step 7 ("r + k = q") adds q, not k, in the reference
// (sm2.c:407-411: r + q == q, that is r = 0 again), so r + k = q does NOT restart there and does not here.
template <class Ops>
ESF_FN bool sign_rs(const Ops &ops, int alg, const typename Ops::F &x, const typename Ops::F &k, const typename Ops::F &e,
		    const typename Ops::F &wx, const typename Ops::F &xinv, typename Ops::F &r, typename Ops::F &s)
{
	typedef typename Ops::F F;
	const F r2 = ops.r2();
	if (alg == ALG_ECGDSA) {
		r = wx;
		const F kr = ops.mul(ops.mul(k, r2), r);                      // k r
		s = ops.mul(ops.mul(x, r2), ops.add(kr, ops.neg(e)));         // x (k r + (-e))  (ecgdsa.c:271-272, :326-328)
	} else if (alg == ALG_ECRDSA) {
		r = wx;
		const F rx = ops.mul(ops.mul(r, r2), x), ke = ops.mul(ops.mul(k, r2), e);
		s = ops.add(rx, ke);                                          // ecrdsa.c:325-327
	} else {
		r = ops.add(e, wx);                                           // sm2.c:393-397
		const F rx = ops.mul(ops.mul(r, r2), x);
		s = ops.mul(ops.sub(k, rx), xinv);                            // sm2.c:439-443
	}
	return !ops.is_zero(r) & !ops.is_zero(s);
}

}  // namespace ecsigfam
