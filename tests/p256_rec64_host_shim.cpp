// tests/p256_rec64_host_shim.cpp -- TEST INFRASTRUCTURE: the 64-digit signed odd recoding of the secp256r1 fast path
// (recode_odd64, libecc_amd/csrc/ecamd_p256.h) compiled for the host (g++, no HIP), so that tests/test_p256_rec64_host.py
// can drive the same code against Python integers.  t_ladder64 follows k_p256_loop_odd<8, MASKED> (ecamd_p256_kernel.hip)
// step for step; t_table_odd makes its table as k_p256_table_odd / k_p256_affine_coz do.
#include <cstring>
#define U29_INLINE_MUL 1
#include "../libecc_amd/csrc/ecamd_p256.h"

using namespace p256;

#ifdef ECAMD_COUNT_MADS
extern "C" {
uint64_t ecamd_mad_count = 0;
}
#endif

constexpr int WB = 4;
constexpr int NE = 1 << (WB - 1);

template <class T> static void ld(T &x, const uint32_t *a)
{
	memcpy(x.l, a, 36);
}
template <class T> static void st(uint32_t *a, const T &x)
{
	memcpy(a, x.l, 36);
}

extern "C" {
uint64_t t_mads(void)
{
#ifdef ECAMD_COUNT_MADS
	return ecamd_mad_count;
#else
	return 0;
#endif
}
void t_mads_reset(void)
{
#ifdef ECAMD_COUNT_MADS
	ecamd_mad_count = 0;
#endif
}

// kw: 8 words of k; d: the 64 digits, top first; returns the sign (1: [k]P = -[sum]P)
int t_digits64(const uint32_t *kw, int32_t *d)
{
	uint32_t e[8];
	const bool sign = recode_odd64(e, kw);
	for (int j = 0; j < 64; j++) {
		u32 idx;
		const bool neg = odd_digit<8, WB>(e, idx);
		d[j] = neg ? -(int32_t)(2 * idx + 1) : (int32_t)(2 * idx + 1);
	}
	return sign ? 1 : 0;
}

// the odd-window table of an affine point (Montgomery-domain canonical limbs x, y): NE entries x (x, y), 18 words each
void t_table_odd(const uint32_t *x, const uint32_t *y, uint32_t *tab)
{
	Fcanon xa, ya;
	ld(xa, x);
	ld(ya, y);
	CoZ D, T[NE];
	FR r[NE];
	FZ z;
	dblu(xa, ya, D, T[0], z);
	for (int j = 1; j < NE; j++) {
		zaddu(D, T[j - 1], T[j], r[j]);
		z = weaken<FZ>(mul(z, r[j]));
	}
	Fmul zi = inv(weaken<Fmul>(mul(z, constant<Fcanon>(K::ONE))));
	for (int j = NE - 1; j >= 1; j--) {
		const Fmul zi2 = weaken<Fmul>(sqr(zi));
		const Fmul zi3 = weaken<Fmul>(mul(zi2, zi));
		st(tab + 18 * j, canonical(mul(T[j].X, zi2)));
		st(tab + 18 * j + 9, canonical(mul(T[j].Y, zi3)));
		if (j > 1) {
			zi = weaken<Fmul>(mul(zi, r[j]));
		}
	}
	st(tab, xa);
	st(tab + 9, ya);
}

// the window loop with the sign applied: start entry (y negated when the sign is set), then 63 windows of 4 doublings and one
// mixed addition whose digit sign is flipped by the scalar's; returns 0, or 1 when an exceptional pair was met (the kernel's
// ECAMD_STATUS_REDO).  out: Jacobian X, Y, Z (27 words, Montgomery limbs)
int t_ladder64(const uint32_t *tab, const uint32_t *kw, uint32_t *out)
{
	uint32_t e[8];
	const bool sign = recode_odd64(e, kw);
	u32 idx;
	Fcanon tx, ty;
	(void)odd_digit<8, WB>(e, idx);
	ld(tx, tab + 18 * idx);
	ld(ty, tab + 18 * idx + 9);
	Jac acc;
	acc.X = weaken<FX>(tx);
	acc.Y = weaken<FY>(carry(sign ? neg_aff(ty) : weaken<FYaff>(ty)));
	acc.Z = weaken<FZ>(constant<Fcanon>(K::ONE));
	bool bad = false, hz;
	for (int j = 1; j < 64; j++) {
		for (int d = 0; d < WB; d++) {
			acc = dbl(acc);
		}
		const bool neg = odd_digit<8, WB>(e, idx) != sign;
		ld(tx, tab + 18 * idx);
		ld(ty, tab + 18 * idx + 9);
		const FYaff y2 = neg ? neg_aff(ty) : weaken<FYaff>(ty);
		acc = madd(acc, tx, y2, hz);
		bad = bad | hz;
	}
	st(out, acc.X);
	st(out + 9, acc.Y);
	st(out + 18, acc.Z);
	return bad ? 1 : 0;
}
}
