// tests/sig_family_host_shim.cpp -- TEST INFRASTRUCTURE: the mod-q steps of ECGDSA / ECRDSA / SM2 (libecc_amd/csrc/ecamd_sigfam.h)
// compiled for the host (g++, no HIP), so that tests/test_sig_family_host.py can drive the same template code against Python
// integers on the real group orders.  The Ops policy here is a word-by-word Montgomery multiplication on the order's own word
// count nw (8, 12 or 17 of the 17 words every array has; R = 2^(32 nw) as in the kernels); the constants q, R^2 mod q and
// -1/q mod 2^32 come from the caller.
#include <cstring>
#include "../libecc_amd/csrc/ecamd_sigfam.h"

namespace {
constexpr int MAXW = 17;
template <int NW> struct FeT {
	uint32_t v[NW];
};
template <int NW> struct HostOps {
	typedef FeT<NW> Fe;
	typedef Fe F;
	enum { WORDS = NW };
	Fe q, rr;
	uint32_t qinv;   // -1 / q mod 2^32
	static bool geq(const uint32_t *a, uint32_t top, const uint32_t *b)
	{
		if (top) {
			return true;
		}
		for (int i = NW - 1; i >= 0; i--) {
			if (a[i] != b[i]) {
				return a[i] > b[i];
			}
		}
		return true;
	}
	static void sub_in(uint32_t *a, const uint32_t *b)
	{
		uint64_t borrow = 0;
		for (int i = 0; i < NW; i++) {
			const uint64_t x = (uint64_t)a[i] - b[i] - borrow;
			a[i] = (uint32_t)x;
			borrow = (x >> 63) & 1;
		}
	}
	Fe mul(const Fe &a, const Fe &b) const
	{
		uint32_t t[NW + 2];
		memset(t, 0, sizeof(t));
		for (int i = 0; i < NW; i++) {
			uint64_t c = 0;
			for (int j = 0; j < NW; j++) {
				const uint64_t x = (uint64_t)a.v[i] * b.v[j] + t[j] + c;
				t[j] = (uint32_t)x;
				c = x >> 32;
			}
			uint64_t x = (uint64_t)t[NW] + c;
			t[NW] = (uint32_t)x;
			t[NW + 1] = (uint32_t)(x >> 32);
			const uint32_t m = t[0] * qinv;
			c = ((uint64_t)m * q.v[0] + t[0]) >> 32;
			for (int j = 1; j < NW; j++) {
				x = (uint64_t)m * q.v[j] + t[j] + c;
				t[j - 1] = (uint32_t)x;
				c = x >> 32;
			}
			x = (uint64_t)t[NW] + c;
			t[NW - 1] = (uint32_t)x;
			t[NW] = t[NW + 1] + (uint32_t)(x >> 32);
		}
		if (geq(t, t[NW], q.v)) {
			sub_in(t, q.v);
		}
		Fe r;
		memcpy(r.v, t, sizeof(r.v));
		return r;
	}
	Fe add(const Fe &a, const Fe &b) const
	{
		uint32_t t[NW];
		uint64_t c = 0;
		for (int i = 0; i < NW; i++) {
			const uint64_t x = (uint64_t)a.v[i] + b.v[i] + c;
			t[i] = (uint32_t)x;
			c = x >> 32;
		}
		if (geq(t, (uint32_t)c, q.v)) {
			sub_in(t, q.v);
		}
		Fe r;
		memcpy(r.v, t, sizeof(r.v));
		return r;
	}
	Fe neg(const Fe &a) const
	{
		if (is_zero(a)) {
			return a;
		}
		Fe r = q;
		sub_in(r.v, a.v);
		return r;
	}
	Fe sub(const Fe &a, const Fe &b) const { return add(a, neg(b)); }
	Fe zero() const
	{
		Fe r;
		memset(r.v, 0, sizeof(r.v));
		return r;
	}
	Fe r2() const { return rr; }
	bool is_zero(const Fe &a) const
	{
		uint32_t acc = 0;
		for (int i = 0; i < NW; i++) {
			acc |= a.v[i];
		}
		return acc == 0;
	}
	bool lt_q(const Fe &a) const { return !geq(a.v, 0, q.v); }
	Fe load_be(const uint8_t *p, int len) const
	{
		Fe r = zero();
		for (int pos = 0; pos < len && pos < 4 * NW; pos++) {
			r.v[pos >> 2] |= (uint32_t)p[len - 1 - pos] << (8 * (pos & 3));
		}
		return r;
	}
	Fe load_le(const uint8_t *p, int len) const
	{
		Fe r = zero();
		for (int pos = 0; pos < len && pos < 4 * NW; pos++) {
			r.v[pos >> 2] |= (uint32_t)p[pos] << (8 * (pos & 3));
		}
		return r;
	}
	Fe shr(Fe a, int n) const
	{
		if (n > 0) {
			for (int j = 0; j < NW; j++) {
				const uint32_t hi = (j + 1 < NW) ? a.v[j + 1] : 0u;
				a.v[j] = (a.v[j] >> n) | (hi << (32 - n));
			}
		}
		return a;
	}
};

template <int NW> HostOps<NW> make_ops(const uint32_t *q, const uint32_t *rr, uint32_t qinv)
{
	HostOps<NW> o;
	memcpy(o.q.v, q, sizeof(o.q.v));
	memcpy(o.rr.v, rr, sizeof(o.rr.v));
	o.qinv = qinv;
	return o;
}
template <int NW> FeT<NW> words(const uint32_t *w)
{
	FeT<NW> r;
	memcpy(r.v, w, sizeof(r.v));
	return r;
}
template <int NW> void put(uint32_t *out, const FeT<NW> &a)
{
	memset(out, 0, MAXW * sizeof(uint32_t));
	memcpy(out, a.v, sizeof(a.v));
}

using namespace ecsigfam;

template <int NW>
void digest_e_t(const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint8_t *dg, int hlen, int qlen, int qbits, uint32_t *out)
{
	put<NW>(out, digest_e(make_ops<NW>(q, rr, qinv), alg, dg, hlen, qlen, qbits));
}

template <int NW>
int front_end_t(const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *r, const uint32_t *s, const uint32_t *e,
		const uint32_t *dinv_m, uint32_t *out, uint32_t *divisor)
{
	const HostOps<NW> ops = make_ops<NW>(q, rr, qinv);
	const FeT<NW> R = words<NW>(r), S = words<NW>(s), E = words<NW>(e);
	memset(out, 0, 3 * MAXW * sizeof(uint32_t));
	put<NW>(divisor, verify_divisor(ops, alg, R, E));
	if (!verify_ranges(ops, R, S)) {
		return 1;
	}
	FeT<NW> u, v, tg;
	if (!verify_uv(ops, alg, R, S, E, words<NW>(dinv_m), u, v, tg)) {
		return 1;
	}
	put<NW>(out, u);
	put<NW>(out + MAXW, v);
	put<NW>(out + 2 * MAXW, tg);
	return 0;
}

template <int NW>
int sign_rs_t(const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *x, const uint32_t *k, const uint32_t *e,
	      const uint32_t *wx, const uint32_t *xinv_m, uint32_t *out)
{
	const HostOps<NW> ops = make_ops<NW>(q, rr, qinv);
	FeT<NW> r, s;
	const bool ok = sign_rs(ops, alg, words<NW>(x), words<NW>(k), words<NW>(e), words<NW>(wx), words<NW>(xinv_m), r, s);
	put<NW>(out, r);
	put<NW>(out + MAXW, s);
	return ok ? 0 : 1;
}
}  // namespace

#define BY_NW(call) (nw == 8 ? call<8> : nw == 12 ? call<12> : call<17>)

extern "C" {
// every array: 17 little-endian words, of which the order's nw (8, 12 or 17) are used
void t_digest_e(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint8_t *dg, int hlen, int qlen, int qbits,
		uint32_t *out)
{
	BY_NW(digest_e_t)(q, rr, qinv, alg, dg, hlen, qlen, qbits, out);
}

// the front end for one item: r, s as loaded, e from digest_e, dinv_m the Montgomery form of 1 / verify_divisor (the caller inverts).
// out: u, v, target (3 x 17 words; zeros where flagged); returns the flag byte; *divisor receives verify_divisor for the caller
int t_front_end(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *r, const uint32_t *s, const uint32_t *e,
		const uint32_t *dinv_m, uint32_t *out, uint32_t *divisor)
{
	return BY_NW(front_end_t)(q, rr, qinv, alg, r, s, e, dinv_m, out, divisor);
}

int t_verify_inverts(int alg) { return verify_inverts(alg) ? 1 : 0; }
int t_sign_inverts(int alg) { return sign_inverts(alg) ? 1 : 0; }
int t_alg_known(int alg) { return alg_known(alg) ? 1 : 0; }

int t_sign_key_ok(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *x)
{
	if (nw == 8) {
		return sign_key_ok(make_ops<8>(q, rr, qinv), alg, words<8>(x)) ? 1 : 0;
	}
	if (nw == 12) {
		return sign_key_ok(make_ops<12>(q, rr, qinv), alg, words<12>(x)) ? 1 : 0;
	}
	return sign_key_ok(make_ops<17>(q, rr, qinv), alg, words<17>(x)) ? 1 : 0;
}

// the signing back end for one item (x, k in range): out r, s (2 x 17 words); returns 1 where the reference restarts
int t_sign_rs(int nw, const uint32_t *q, const uint32_t *rr, uint32_t qinv, int alg, const uint32_t *x, const uint32_t *k, const uint32_t *e,
	      const uint32_t *wx, const uint32_t *xinv_m, uint32_t *out)
{
	return BY_NW(sign_rs_t)(q, rr, qinv, alg, x, k, e, wx, xinv_m, out);
}
}
