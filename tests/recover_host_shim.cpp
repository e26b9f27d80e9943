// tests/recover_host_shim.cpp -- TEST INFRASTRUCTURE: the field-level steps of ECDSA public-key recovery
// (libecc_amd/csrc/ecamd_recover.h) compiled for the host (g++, no HIP), so that tests/test_recover_host.py can drive the same
// template code against Python integers.  The Ops policy here is arithmetic modulo a prime below 2^62 on unsigned __int128; the
// kernels instantiate the same templates over the saturated Montgomery words of ecamd_field.h.
#include <cstring>
#include "../libecc_amd/csrc/ecamd_recover.h"

using namespace ecrecover;

typedef unsigned __int128 u128;

struct HostOps {
	uint64_t m;
	uint64_t mul(uint64_t a, uint64_t b) const { return (uint64_t)((u128)a * b % m); }
	uint64_t sqr(uint64_t a) const { return mul(a, a); }
	uint64_t add(uint64_t a, uint64_t b) const { return (uint64_t)(((u128)a + b) % m); }
	uint64_t sub(uint64_t a, uint64_t b) const { return (uint64_t)(((u128)a + m - b) % m); }
	uint64_t neg(uint64_t a) const { return sub(0, a); }
};

extern "C" {
// out: x1, y1, x2, y2
void t_sums(uint64_t m, uint64_t xa, uint64_t ya, uint64_t xb, uint64_t yb, uint64_t dinv, uint64_t *out)
{
	const HostOps ops{m};
	recover_sums(ops, xa, ya, xb, yb, dinv, out[0], out[1], out[2], out[3]);
}

// out: u, v
void t_uv(uint64_t m, uint64_t e, uint64_t s, uint64_t rinv, uint64_t *out)
{
	const HostOps ops{m};
	recover_uv(ops, e, s, rinv, out[0], out[1]);
}

int t_needs_redo(uint32_t stA, uint32_t stB, int same_x)
{
	return recover_needs_redo(stA, stB, same_x != 0) ? 1 : 0;
}

// the digest as k_recover_prep reads it (recover_e: digest_window, a big-endian load of elen bytes, shift_right), before the
// reduction mod q: 17 little-endian words
void t_digest_window(const uint8_t *dg, int hlen, int qlen, int qbits, uint32_t *out)
{
	int rshift = 0;
	const int elen = digest_window(hlen, qlen, qbits, &rshift);
	uint32_t v[17];
	memset(v, 0, sizeof(v));
	for (int pos = 0; pos < elen && pos < 68; pos++) {
		v[pos >> 2] |= (uint32_t)dg[elen - 1 - pos] << (8 * (pos & 3));
	}
	shift_right<17>(v, rshift);
	memcpy(out, v, sizeof(v));
}

int t_be_geq(const uint8_t *a, int alen, const uint8_t *b, int blen)
{
	return be_geq(a, alen, b, blen) ? 1 : 0;
}
}
