// tests/bign_host_shim.cpp -- TEST INFRASTRUCTURE: belt-hash (libecc_amd/csrc/ecamd_belt.h) and the per-item steps of BIGN / DBIGN
// (libecc_amd/csrc/ecamd_bign.h) compiled for the host (g++, no HIP), so that tests/test_bign_host.py can drive the same template
// code against the Python restatement and the recorded reference answers.  The Ops policy is the one of
// tests/sig_family_host_shim.cpp, included here as it stands; the substitution table is a plain array.
#include "sig_family_host_shim.cpp"
#include "../libecc_amd/csrc/ecamd_belt.h"
#include "../libecc_amd/csrc/ecamd_bign.h"

namespace {
const uint8_t BELT_H[256] = {ECAMD_BELT_H};

template <int NW>
int b_verify_uv_t(const uint32_t *q, const uint32_t *rr, uint32_t qinv, const uint8_t *sig, int qlen, const uint8_t *dg, int hsize, uint32_t *out)
{
	FeT<NW> u, v;
	const bool ok = ecbign::verify_uv(make_ops<NW>(q, rr, qinv), sig, qlen, dg, hsize, u, v);
	put<NW>(out, u);
	put<NW>(out + MAXW, v);
	return ok ? 0 : 1;
}
template <int NW>
int b_sign_s1_t(const uint32_t *q, const uint32_t *rr, uint32_t qinv, const uint32_t *x, const uint32_t *k, const uint8_t *bt, int qlen,
		const uint8_t *dg, int hsize, uint32_t *out)
{
	const HostOps<NW> ops = make_ops<NW>(q, rr, qinv);
	put<NW>(out, ecbign::sign_s1(ops, words<NW>(x), words<NW>(k), bt, qlen, dg, hsize));
	return ecbign::sign_key_ok(ops, words<NW>(x)) ? 0 : 1;
}
}  // namespace

extern "C" {
// n slots of `stride` bytes (little-endian u32 length, then the message; the length clamped to the slot as in k_belt_slots) -> n x 32
void b_belt_slots(const uint8_t *slots, uint32_t stride, uint32_t n, uint8_t *out)
{
	for (uint32_t i = 0; i < n; i++) {
		uint32_t buf[1024], len, dg[8];
		memcpy(buf, slots + (size_t)i * stride, stride);
		len = buf[0] > stride - 4 ? stride - 4 : buf[0];
		ecbelt::hash_words(BELT_H, buf + 1, len, dg);
		memcpy(out + (size_t)i * 32, dg, 32);
	}
}
// out: u (of G), v (of Y), 2 x 17 words; returns the flag byte
int b_verify_uv(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, const uint8_t *sig, int qlen, const uint8_t *dg, int hsize, uint32_t *out)
{
	return BY_NW(b_verify_uv_t)(q, rr, qinv, sig, qlen, dg, hsize, out);
}
// out: s1 (17 words); returns 1 where the key is refused
int b_sign_s1(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, const uint32_t *x, const uint32_t *k, const uint8_t *bt, int qlen,
	      const uint8_t *dg, int hsize, uint32_t *out)
{
	return BY_NW(b_sign_s1_t)(q, rr, qinv, x, k, bt, qlen, dg, hsize, out);
}
// belt-hash's slot for one item, as k_bign_fill writes it: returns its stride
uint32_t b_fill(const uint8_t *oid, uint32_t oid_len, const uint8_t *W, uint32_t clen, int qlen, const uint8_t *dg, uint32_t hsize, uint8_t *slot)
{
	const uint32_t ilen = ecbign::belt_input_len(oid_len, qlen, hsize), stride = ecbign::belt_stride(oid_len, qlen, hsize);
	memset(slot, 0, stride);
	for (uint32_t b = 0; b < 4; b++) {
		slot[b] = (uint8_t)(ilen >> (8 * b));
	}
	for (uint32_t b = 0; b < ilen; b++) {
		slot[4 + b] = ecbign::belt_input_byte(b, oid, oid_len, W, clen, qlen, dg);
	}
	return stride;
}
int b_t_matches(const uint8_t *bt, const uint8_t *s0, int qlen) { return ecbign::t_matches(bt, s0, qlen) ? 1 : 0; }
int b_alg_known(int alg) { return ecbign::alg_known(alg) ? 1 : 0; }
int b_hash_size(int hash_type) { return ecbign::hash_size(hash_type); }
int b_s0_len(int qlen) { return ecbign::s0_len(qlen); }
int b_sig_len(int qlen) { return ecbign::sig_len(qlen); }
int b_t_len(int qlen) { return ecbign::t_len(qlen); }
int b_slot_ok(uint32_t len, uint32_t stride) { return ecbign::slot_ok(len, stride) ? 1 : 0; }
}
