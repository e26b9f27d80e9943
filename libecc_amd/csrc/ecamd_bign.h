// libecc_amd/csrc/ecamd_bign.h -- the mod-q and byte-level steps of BIGN / DBIGN (STB 34.101.45) around their multiplications and
// the BelT-hash of the commitment (ecamd_belt.h).  Paths relative to the reference's src/: sig/bign_common.c:742-962
// (verification), :468-690 (signing), :345-374 (the key rule), sig/bign_common.h:34-37 (the lengths).
//
//   qlen = ceil(|q| / 8), l = qlen / 2 (integer division); a signature is s0 (l bytes) || s1 (qlen bytes)
//   EVERYTHING IS LITTLE-ENDIAN: s0, s1, the digest read as a number, the coordinates of W in the hash input
//   hbar = the whole digest, little-endian, mod q (it may be longer than q)
//   verify:  s1 < q (s0 has no range check); u = s1 + hbar (0 is legal), v = s0 + 2^(8l); W = [u]G + [v]Y, finite;
//            t = the first min(l, 32) bytes of belt-hash(OID || first 2l bytes of LE(W.x) || LE(W.y) || digest), zero-padded
//            to l bytes; accept iff t = s0 over all l bytes (l = 33 on a 521-bit order: byte 32 of s0 must be 0)
//   sign:    x < q; W = [k]G; s0 = t as above; s1 = k - hbar - (s0 + 2^(8l)) x.  No restart, no test of s1.
// BIGN and DBIGN differ in where the nonce comes from only: these steps take it as given (DBIGN's generator is ecamd_dbign_nonce.h).
//
// Written against the `Ops` policy of ecamd_sigfam.h, so the same text runs in the kernels (ecamd_bign_kernels.h) and on the host
// in tests/bign_host_shim.cpp.
#pragma once
#include "ecamd_sigfam.h"

namespace ecbign {

// libecc's ec_alg_type numbers (lib_ecc_types.h) and its hash_alg_type number of BELT_HASH, as include/libecc_amd.h exports them
enum : int { ALG_BIGN = 18, ALG_DBIGN = 19, HASH_BELT = 16, MAX_OID = 64, MAX_DIGEST = 128, DIGEST_BT = 32 /* belt-hash's digest */ };

ESF_FN bool alg_known(int alg)
{
	return alg == ALG_BIGN || alg == ALG_DBIGN;
}

// digest bytes of a hash the device computes for the message: libecc's types 1 .. 4 (SHA-2) and 16 (belt-hash); 0 for any other
ESF_FN int hash_size(int hash_type)
{
	return hash_type == 1 ? 28 : hash_type == 2 ? 32 : hash_type == 3 ? 48 : hash_type == 4 ? 64 : hash_type == HASH_BELT ? 32 : 0;
}

ESF_FN int s0_len(int qlen) { return qlen / 2; }
ESF_FN int sig_len(int qlen) { return qlen / 2 + qlen; }
// bytes of t that come from the BelT digest; the rest of its l bytes are zero
ESF_FN int t_len(int qlen) { return s0_len(qlen) < 32 ? s0_len(qlen) : 32; }
// bytes of belt-hash's input and the stride of its slot (a multiple of 4 that holds the length word too)
ESF_FN uint32_t belt_input_len(uint32_t oid_len, int qlen, uint32_t hsize) { return oid_len + 2u * (uint32_t)s0_len(qlen) + hsize; }
ESF_FN uint32_t belt_stride(uint32_t oid_len, int qlen, uint32_t hsize) { return (4u + belt_input_len(oid_len, qlen, hsize) + 3u) & ~3u; }

// a message slot (little-endian u32 length, then the message) is usable: it fits the stride
ESF_FN bool slot_ok(uint32_t len, uint32_t stride)
{
	return stride >= 4u && len <= stride - 4u;
}

template <class Ops> ESF_FN typename Ops::F hbar(const Ops &ops, const uint8_t *dg, int hsize)
{
	return ecsigfam::wide_mod(ops, dg, hsize, true);
}

// v = (s0 + 2^(8l)) mod q from the first nb bytes of s0 (the caller knows the other l - nb to be zero).  8l < |q| - 1 for every
// order of 18 bits or more, so both terms are below q.
template <class Ops> ESF_FN typename Ops::F s0_v(const Ops &ops, const uint8_t *s0, int nb, int qlen)
{
	typedef typename Ops::F F;
	const int l = s0_len(qlen);
	F pw = ops.zero();
#pragma unroll
	for (int j = 0; j < (int)Ops::WORDS; j++) {
		pw.v[j] = (j == ((8 * l) >> 5)) ? (1u << ((8 * l) & 31)) : 0u;
	}
	return ops.add(ops.load_le(s0, nb), pw);
}

// The verification front end for one item: u multiplies G, v multiplies Y.  Returns false where the scheme rejects before its
// multiplications (s1 >= q).
template <class Ops>
ESF_FN bool verify_uv(const Ops &ops, const uint8_t *sig, int qlen, const uint8_t *dg, int hsize, typename Ops::F &u, typename Ops::F &v)
{
	typedef typename Ops::F F;
	const F s1 = ops.load_le(sig + s0_len(qlen), qlen);
	u = ops.zero();
	v = ops.zero();
	if (!ops.lt_q(s1)) {
		return false;
	}
	u = ops.add(s1, hbar(ops, dg, hsize));
	v = s0_v(ops, sig, s0_len(qlen), qlen);
	return true;
}

// byte b of belt-hash's input for one item: OID || first 2l bytes of LE(W.x, clen) || LE(W.y, clen) (zeros beyond 2 clen) || digest.
// W: the affine point, X || Y big-endian, clen bytes each.
ESF_FN uint8_t belt_input_byte(uint32_t b, const uint8_t *oid, uint32_t oid_len, const uint8_t *W, uint32_t clen, int qlen, const uint8_t *dg)
{
	const uint32_t l2 = 2u * (uint32_t)s0_len(qlen);
	if (b < oid_len) {
		return oid[b];
	}
	b -= oid_len;
	if (b < l2) {
		return b < clen ? W[clen - 1u - b] : (b < 2u * clen ? W[2u * clen - 1u - (b - clen)] : (uint8_t)0);
	}
	return dg[b - l2];
}

// the verdict's byte comparison: t (from the BelT digest bt) against s0 over all l bytes
ESF_FN bool t_matches(const uint8_t *bt, const uint8_t *s0, int qlen)
{
	const int l = s0_len(qlen), tl = t_len(qlen);
	uint32_t diff = 0;
	for (int b = 0; b < l; b++) {
		diff |= (uint32_t)(s0[b] ^ (b < tl ? bt[b] : (uint8_t)0));
	}
	return diff == 0;
}

// The private key as loaded from qlen bytes (any value below R): x < q, 0 included -- the key import's rule (bign_common.c:361)
// and the signer's (:526-530), as the recording shows it (tests/golden/bign.json, family x_edge).
template <class Ops> ESF_FN bool sign_key_ok(const Ops &ops, const typename Ops::F &x)
{
	return ops.lt_q(x);
}

// s1 = k - hbar - (s0 + 2^(8l)) x from x (below q), k (below q) and bt (the BelT digest: its first t_len bytes are s0's, the
// rest of s0 is zero).  Straight-line in x and k.
template <class Ops>
ESF_FN typename Ops::F sign_s1(const Ops &ops, const typename Ops::F &x, const typename Ops::F &k, const uint8_t *bt, int qlen,
			       const uint8_t *dg, int hsize)
{
	typedef typename Ops::F F;
	const F vx = ops.mul(ops.mul(s0_v(ops, bt, t_len(qlen), qlen), ops.r2()), x);
	return ops.sub(ops.sub(k, vx), hbar(ops, dg, hsize));
}

}  // namespace ecbign
