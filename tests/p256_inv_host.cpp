// tests/p256_inv_host.cpp -- TEST INFRASTRUCTURE: the secp256r1 field inversion of libecc_amd/csrc/ecamd_p256.h compiled for the
// host (plain C++17, no HIP), as tests/u29_host_shim.cpp does for the rest of the header.
//   * as a shared library, tests/test_p256_inv_host.py drives it against Python integers;
//   * with -DP256_INV_MAIN it is a stand-alone program that checks inv(x) x = 1 by the header's own multiplication, for the edge
//     cases and 10^5 random values -- the form in which it is built with -fsanitize=address,undefined (the divsteps live on signed
//     shifts and signed 64-bit accumulators).
#include <cstdio>
#include <cstring>
#define U29_INLINE_MUL 1
#include "../libecc_amd/csrc/ecamd_p256.h"

using namespace p256;

// one inversion with its internals: out = inv(a) (9 limbs); fg = the final f and g (2 x 9 signed limbs) of the same divstep run;
// returns the number of divsteps executed
static int inv_traced(const uint32_t *a, uint32_t *out, int32_t *fg)
{
	Fmul x;
	memcpy(x.l, a, 36);
	const Fmul r = inv(x);
	memcpy(out, r.l, 36);
	const Fcanon xc = canonical(x);
	int32_t d[9];
	return safegcd_run(fg, fg + 9, d, xc.l, K::R2);
}

extern "C" {
// n inversions: a, out n x 9 limbs; fg n x 18; steps n
void t_inv_batch(int n, const uint32_t *a, uint32_t *out, int32_t *fg, int32_t *steps)
{
	for (int i = 0; i < n; i++) {
		steps[i] = inv_traced(a + 9 * i, out + 9 * i, fg + 18 * i);
	}
}
void t_inv_fermat(const uint32_t *a, uint32_t *out)
{
	Fmul x;
	memcpy(x.l, a, 36);
	const Fmul r = inv_fermat(x);
	memcpy(out, r.l, 36);
}
void t_inv_consts(uint32_t *out)  // e0 = R^2 mod p (9), SAFEGCD_N, SAFEGCD_BATCHES, P256_INV_FERMAT
{
	memcpy(out, K::R2, 36);
	out[9] = SAFEGCD_N;
	out[10] = SAFEGCD_BATCHES;
	out[11] = P256_INV_FERMAT;
}
}

#ifdef P256_INV_MAIN
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}

static int failures = 0;

// a: nine limbs within Fmul's bounds (limbs <= MASK, value < 2p)
static void check(const uint32_t *a, const char *what)
{
	uint32_t out[9];
	int32_t fg[18];
	const int steps = inv_traced(a, out, fg);
	Fmul x, y;
	memcpy(x.l, a, 36);
	memcpy(y.l, out, 36);
	const Fcanon xc = canonical(x);
	bool zero = true;
	for (int i = 0; i < 9; i++) {
		zero = zero && xc.l[i] == 0;
	}
	const Fcanon prod = canonical(mul(x, y));  // a R * a^-1 R / R = R
	bool ok = steps == SAFEGCD_N * SAFEGCD_BATCHES;
	bool g0 = true, f1 = fg[0] == 1, fm1 = fg[8] == -1;
	for (int i = 0; i < 9; i++) {
		ok = ok && prod.l[i] == (zero ? 0u : K::ONE[i]);
		ok = ok && (!zero || out[i] == 0);
		ok = ok && out[i] <= (i < 8 ? MASK : (1u << 24));
		g0 = g0 && fg[9 + i] == 0;
		f1 = f1 && (i == 0 || fg[i] == 0);
		fm1 = fm1 && (i == 8 || fg[i] == (int32_t)MASK);
	}
	ok = ok && g0 && (zero || f1 || fm1);
	uint32_t fer[9];
	t_inv_fermat(a, fer);
	Fmul fr;
	memcpy(fr.l, fer, 36);
	const Fcanon fc = canonical(fr);
	for (int i = 0; i < 9; i++) {
		ok = ok && fc.l[i] == out[i];  // the divstep result is canonical, and equals the chain's residue
	}
	if (!ok) {
		failures++;
		fprintf(stderr, "FAIL %s: %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", what, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7],
			a[8]);
	}
}

// limbs of v + k p for the canonical digits v (k = 0 or 1), exact digits
static void plus_p(uint32_t *a, int k)
{
	uint32_t c = 0;
	for (int i = 0; i < 9; i++) {
		const uint32_t s = a[i] + (k ? u29::P256::P[i] : 0u) + c;
		a[i] = i < 8 ? (s & MASK) : s;
		c = i < 8 ? (s >> 29) : 0;
	}
}

int main()
{
	uint32_t a[9];
	// 0, 1, 2, p - 1, p - 2, as plain digits and shifted by p (value in [p, 2p): the loosest value Fmul admits)
	for (int k = 0; k < 2; k++) {
		for (int v = 0; v < 3; v++) {
			memset(a, 0, sizeof a);
			a[0] = (uint32_t)v;
			plus_p(a, k);
			check(a, "small");
		}
		for (int v = 1; v < 3; v++) {
			memcpy(a, u29::P256::P, 36);
			a[0] -= (uint32_t)v;
			plus_p(a, k);
			check(a, "p - small");
		}
		check(K::ONE, "R");
		check(K::R2, "R^2");
	}
	// every limb at its bound: limbs 0..7 = MASK, top limb as large as the value bound 2p allows
	for (int i = 0; i < 8; i++) {
		a[i] = MASK;
	}
	a[8] = (2u << 24) - 2;
	check(a, "all limbs at the bound");
	// single bits 2^k, k < 256, and 2^256 - 1
	for (int k = 0; k < 256; k++) {
		memset(a, 0, sizeof a);
		a[k / 29] = 1u << (k % 29);
		check(a, "2^k");
	}
	for (int i = 0; i < 8; i++) {
		a[i] = MASK;
	}
	a[8] = (1u << 24) - 1;
	check(a, "2^256 - 1");
	// random: 9 x 29 bits with the top limb below 2p's (0x1fffffe), so the value is < 2p
	for (int n = 0; n < 100000; n++) {
		for (int i = 0; i < 8; i++) {
			a[i] = (uint32_t)rng() & MASK;
		}
		a[8] = (uint32_t)(rng() % ((2u << 24) - 2));
		check(a, "random");
	}
	printf("p256 inversion: %d failures, %d divsteps per inversion\n", failures, SAFEGCD_N * SAFEGCD_BATCHES);
	return failures ? 1 : 0;
}
#endif
