// tests/sig_hashed_host_shim.cpp -- TEST INFRASTRUCTURE: the mod-q and byte-level steps of ECSDSA / ECOSDSA / ECKCDSA
// (libecc_amd/csrc/ecamd_sighash.h) compiled for the host (g++, no HIP), so that tests/test_sig_hashed_host.py can drive the same
// template code against Python integers on the real group orders.  The Ops policy (word-by-word Montgomery multiplication on the
// order's own word count) is the one of tests/sig_family_host_shim.cpp, included here as it stands.
#include "sig_family_host_shim.cpp"
#include "../libecc_amd/csrc/ecamd_sighash.h"

namespace {
template <int NW>
int h_verify_uv_t(const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint8_t *sig, int hsize, int qlen, const uint8_t *h,
		  uint32_t *out)
{
	FeT<NW> u, v;
	const bool ok = echsig::verify_uv(make_ops<NW>(q, rr, qinv), alg, sig, hsize, qlen, h, u, v);
	put<NW>(out, u);
	put<NW>(out + MAXW, v);
	return ok ? 0 : 1;
}
template <int NW>
int h_sign_s_t(const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *x, const uint32_t *k, const uint8_t *dg, int hsize,
	       int qlen, const uint8_t *h, uint32_t *out)
{
	const HostOps<NW> ops = make_ops<NW>(q, rr, qinv);
	FeT<NW> s = ops.zero();
	if (!echsig::sign_key_ok(ops, alg, words<NW>(x))) {
		put<NW>(out, s);
		return 2;
	}
	const bool ok = echsig::sign_s(ops, alg, words<NW>(x), words<NW>(k), dg, hsize, qlen, h, s);
	put<NW>(out, s);
	return ok ? 0 : 1;
}
}  // namespace

extern "C" {
// out: u (of G), v (of Y), 2 x 17 words; returns the flag byte
int h_verify_uv(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint8_t *sig, int hsize, int qlen, const uint8_t *h,
		uint32_t *out)
{
	return BY_NW(h_verify_uv_t)(q, rr, qinv, alg, sig, hsize, qlen, h, out);
}
// out: s (17 words); returns 0, 1 where the reference fails or restarts, 2 where the key is refused
int h_sign_s(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *x, const uint32_t *k, const uint8_t *dg, int hsize,
	     int qlen, const uint8_t *h, uint32_t *out)
{
	return BY_NW(h_sign_s_t)(q, rr, qinv, alg, x, k, dg, hsize, qlen, h, out);
}
int h_alg_known(int alg) { return echsig::alg_known(alg) ? 1 : 0; }
int h_hash_size(int hash_type) { return echsig::hash_size(hash_type); }
int h_r_len(int alg, int hsize, int qlen) { return echsig::r_len(alg, hsize, qlen); }
int h_blank_len(int alg, int clen) { return echsig::blank_len(alg, clen); }
int h_slot_ok(int alg, uint32_t len, uint32_t stride, int clen) { return echsig::slot_ok(alg, len, stride, clen) ? 1 : 0; }
int h_digest_matches(const uint8_t *dg, int hsize, const uint8_t *r, int rl) { return echsig::digest_matches(dg, hsize, r, rl) ? 1 : 0; }
}
