// libecc_amd/csrc/ecamd_sighash.h -- the mod-q and byte-level steps of ECSDSA, ECOSDSA and ECKCDSA around their multiplications
// and their hash of the commitment.
//
// These schemes hash AFTER the multiplication: the verifier computes W' = [u]G + [v]Y, hashes its affine coordinates and
// compares the digest with the signature's r as a BYTE STRING; the signer hashes W = [k]G and derives e from the digest
// (paths relative to the reference's src/):
//
//   scheme                               r (bytes)                       verify: e, u (of G), v (of Y)            accept iff              sign (nonce k)
//   ECSDSA  sig/ecsdsa_common.c:474-607  H(Wx || Wy || m), |H| bytes     e = -(OS2I(r) mod q), e != 0; s, e       H(W'x || W'y || m) = r  e = OS2I(r) mod q != 0,
//           :180-371                                                                                                                     s = k + e x != 0
//   ECOSDSA (same file, optimized)       H(Wx || m), |H| bytes           as ECSDSA                                H(W'x || m) = r         as ECSDSA
//   ECKCDSA sig/eckcdsa.c:589-800        the last r_len bytes of H(Wx),  e = OS2I(r XOR h') mod q (0 allowed);    last r_len bytes of     s = x (k - e) != 0
//           :340-471                     r_len = min(|H|, qlen)          e, s       (Y = [1/x]G)                   H(W'x) = r
// h' is the last r_len bytes of the caller's h = H(z || m) (the reference shifts whole bytes: buf_lshift, eckcdsa.c:136-160).
// s is in [1, q - 1] for all three (ecsdsa_common.c:475-478, eckcdsa.c:679-683); r is never range-checked: it is a byte string.
//
// Written against the `Ops` policy of ecamd_sigfam.h (one modulus q, Montgomery radix R of its word size), so the same text runs
// in the kernels (ecamd_sighash_kernels.h) and on the host in tests/sig_hashed_host_shim.cpp.
#pragma once
#include "ecamd_sigfam.h"

namespace echsig {

// libecc's ec_alg_type numbers (lib_ecc_types.h), as include/libecc_amd.h exports them
enum : int { ALG_ECKCDSA = 2, ALG_ECSDSA = 3, ALG_ECOSDSA = 4 };

ESF_FN bool alg_known(int alg)
{
	return alg == ALG_ECKCDSA || alg == ALG_ECSDSA || alg == ALG_ECOSDSA;
}

// digest bytes of libecc's hash types 1 .. 4 (SHA-224 / 256 / 384 / 512); 0 for any other
ESF_FN int hash_size(int hash_type)
{
	return hash_type == 1 ? 28 : hash_type == 2 ? 32 : hash_type == 3 ? 48 : hash_type == 4 ? 64 : 0;
}

// bytes of r in a signature: ECSDSA_R_LEN (sig/ecsdsa.h:28), ECKCDSA_R_LEN (sig/eckcdsa.h:28)
ESF_FN int r_len(int alg, int hsize, int qlen)
{
	return (alg == ALG_ECKCDSA && qlen < hsize) ? qlen : hsize;
}

// bytes of the blank in front of the message that the device fills with the commitment's coordinates (ecsdsa_common.c:509-518);
// ECKCDSA hashes FE2OS(W'x) alone, in a slot the device builds
ESF_FN int blank_len(int alg, int clen)
{
	return alg == ALG_ECSDSA ? 2 * clen : clen;
}

// a message slot (little-endian u32 length, then the hash input) is usable: the blank is counted in the length and the input
// fits the stride
ESF_FN bool slot_ok(int alg, uint32_t len, uint32_t stride, int clen)
{
	return len >= (uint32_t)blank_len(alg, clen) && len <= stride - 4u;
}

// ECKCDSA: e = OS2I(r XOR h') mod q (eckcdsa.c:427-433, :727-733); r: rl bytes, h: the whole digest of hsize bytes
template <class Ops> ESF_FN typename Ops::F kcdsa_e(const Ops &ops, const uint8_t *r, int rl, const uint8_t *h, int hsize)
{
	typename Ops::F a = ops.load_be(r, rl);
	const typename Ops::F b = ops.load_be(h + (hsize - rl), rl);
#pragma unroll
	for (int j = 0; j < (int)Ops::WORDS; j++) {
		a.v[j] ^= b.v[j];
	}
	return ecsigfam::reduce(ops, a);   // rl <= qlen bytes: below R
}

// ECSDSA / ECOSDSA: OS2I(r) mod q over all hsize bytes of r, which may be longer than q (ecsdsa_common.c:323-324, :486-487)
template <class Ops> ESF_FN typename Ops::F sdsa_e(const Ops &ops, const uint8_t *r, int hsize)
{
	return ecsigfam::wide_mod(ops, r, hsize, false);
}

// The verification front end for one item.  sig: r (r_len bytes) then s (qlen bytes); h: ECKCDSA's H(z || m), unused otherwise.
// u multiplies G, v multiplies Y.  Returns false where the scheme rejects before its multiplications.
template <class Ops>
ESF_FN bool verify_uv(const Ops &ops, int alg, const uint8_t *sig, int hsize, int qlen, const uint8_t *h, typename Ops::F &u,
		      typename Ops::F &v)
{
	typedef typename Ops::F F;
	const int rl = r_len(alg, hsize, qlen);
	const F s = ops.load_be(sig + rl, qlen);
	u = ops.zero();
	v = ops.zero();
	if (ops.is_zero(s) | !ops.lt_q(s)) {
		return false;
	}
	if (alg == ALG_ECKCDSA) {
		u = kcdsa_e(ops, sig, rl, h, hsize);   // W' = [s]Y + [e]G (eckcdsa.c:736-741)
		v = s;
		return true;
	}
	const F e = ops.neg(sdsa_e(ops, sig, hsize));   // W' = [s]G + [e]Y, e = -r mod q (ecsdsa_common.c:486-497)
	if (ops.is_zero(e)) {
		return false;
	}
	u = s;
	v = e;
	return true;
}

// the verdict's byte comparison: the last rl bytes of the digest of the commitment against r
ESF_FN bool digest_matches(const uint8_t *dg, int hsize, const uint8_t *r, int rl)
{
	uint32_t diff = 0;
	for (int b = 0; b < rl; b++) {
		diff |= (uint32_t)(dg[hsize - rl + b] ^ r[b]);
	}
	return diff == 0;
}

// The private key as loaded from qlen bytes (any value below R), as the recording of the reference shows it
// (tests/golden/sig_hashed.json, family x_edge).  ECKCDSA's key pair imports for 0 < x < q only (Y = [1/x]G, eckcdsa.c:53-63).
// ECSDSA and ECOSDSA have no range check, neither on import (ecsdsa_common.c:30-58) nor in signing: the reference signs with
// x = 0 and with any x >= q that fits qlen bytes, s = (k + e x) mod q with x taken as it is.
template <class Ops> ESF_FN bool sign_key_ok(const Ops &ops, int alg, const typename Ops::F &x)
{
	return alg != ALG_ECKCDSA || (!ops.is_zero(x) & ops.lt_q(x));
}

// s from x (as sign_key_ok admits it), k (in range, plain) and dg, the digest of the commitment W = [k]G (hsize bytes); h as in verify_uv.  r of the
// signature is the last r_len bytes of dg.  Returns false where the reference fails (ECSDSA: e = 0 or s = 0,
// ecsdsa_common.c:333, :366) or restarts (ECKCDSA: s = 0, eckcdsa.c:460-464), which a fixed nonce cannot get past.
template <class Ops>
ESF_FN bool sign_s(const Ops &ops, int alg, const typename Ops::F &x, const typename Ops::F &k, const uint8_t *dg, int hsize, int qlen,
		   const uint8_t *h, typename Ops::F &s)
{
	typedef typename Ops::F F;
	const F r2 = ops.r2();
	if (alg == ALG_ECKCDSA) {
		const int rl = r_len(alg, hsize, qlen);
		const F e = kcdsa_e(ops, dg + (hsize - rl), rl, h, hsize);
		s = ops.mul(ops.mul(x, r2), ops.sub(k, e));             // x (k - e)  (eckcdsa.c:452-454)
		return !ops.is_zero(s);
	}
	const F e = sdsa_e(ops, dg, hsize);
	s = ops.add(k, ops.mul(ops.mul(e, r2), x));                     // k + e x  (ecsdsa_common.c:341-347)
	return !ops.is_zero(e) & !ops.is_zero(s);
}

}  // namespace echsig
