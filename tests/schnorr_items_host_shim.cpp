// tests/schnorr_items_host_shim.cpp -- TEST INFRASTRUCTURE: the per-item steps of BIP0340 / ECFSDSA
// (libecc_amd/csrc/ecamd_schnorr.h) compiled for the host (g++, no HIP), so that tests/test_schnorr_items_host.py can drive the same
// template code against Python integers on the real group orders.  The Ops policy (word-by-word Montgomery multiplication on the
// order's own word count) is the one of tests/sig_family_host_shim.cpp, included here as it stands.
#include "sig_family_host_shim.cpp"
#include "../libecc_amd/csrc/ecamd_schnorr.h"

namespace {
// out: e, q - e, BIP0340's s, ECFSDSA's s (4 x 17 words); returns bit 0: verify_s_ok(x taken as s), bit 1: sign_key_ok(x), bit 2: nonce_ok(k),
// bit 3: ECFSDSA's s != 0
template <int NW>
int s_item_t(const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *x, const uint32_t *k, const uint8_t *dg, int hsize,
	     int y_odd, int r_odd, uint32_t *out)
{
	const HostOps<NW> ops = make_ops<NW>(q, rr, qinv);
	const FeT<NW> e = ecschnorr::digest_e(ops, dg, hsize);
	put<NW>(out, e);
	put<NW>(out + MAXW, ecschnorr::neg_e(ops, e));
	int ret = (ecschnorr::verify_s_ok(ops, alg, words<NW>(x)) ? 1 : 0) | (ecschnorr::sign_key_ok(ops, alg, words<NW>(x)) ? 2 : 0) |
		  (ecschnorr::nonce_ok(ops, words<NW>(k)) ? 4 : 0);
	FeT<NW> s = ops.zero();
	if ((ret & 6) == 6) {
		put<NW>(out + 2 * MAXW, ecschnorr::bip0340_s(ops, words<NW>(x), words<NW>(k), e, y_odd != 0, r_odd != 0));
		ret |= ecschnorr::ecfsdsa_s(ops, words<NW>(x), words<NW>(k), e, s) ? 8 : 0;
		put<NW>(out + 3 * MAXW, s);
	}
	return ret;
}
}  // namespace

extern "C" {
int s_item(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *x, const uint32_t *k, const uint8_t *dg, int hsize,
	   int y_odd, int r_odd, uint32_t *out)
{
	return BY_NW(s_item_t)(q, rr, qinv, alg, x, k, dg, hsize, y_odd, r_odd, out);
}
int s_alg_known(int alg) { return ecschnorr::alg_known(alg) ? 1 : 0; }
int s_r_len(int alg, int clen) { return ecschnorr::r_len(alg, clen); }
int s_r_off(int alg, int hsize) { return ecschnorr::r_off(alg, hsize); }
int s_x_off(int alg, int hsize, int clen) { return ecschnorr::x_off(alg, hsize, clen); }
int s_fixed_len(int alg, int hsize, int clen) { return ecschnorr::fixed_len(alg, hsize, clen); }
int s_slot_ok(int alg, uint32_t len, uint32_t stride, int hsize, int clen) { return ecschnorr::slot_ok(alg, len, stride, hsize, clen) ? 1 : 0; }
int s_coord_ok(const uint8_t *c, const uint8_t *p_be, int clen) { return ecschnorr::coord_ok(c, p_be, clen) ? 1 : 0; }
void s_lift_y(uint8_t *out, const uint8_t *y, const uint8_t *p_be, int clen) { ecschnorr::lift_y(out, y, p_be, clen); }
int s_accept(int alg, const uint8_t *W, const uint8_t *r, int clen) { return ecschnorr::accept(alg, W, r, clen) ? 1 : 0; }
}
