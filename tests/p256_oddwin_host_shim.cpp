// tests/p256_oddwin_host_shim.cpp -- TEST INFRASTRUCTURE: the co-Z group law, the odd-digit recoding and the odd-window
// pipeline of the secp256r1 fast path (libecc_amd/csrc/ecamd_p256.h) compiled for the host (g++, no HIP), so that
// tests/test_p256_oddwin_host.py can drive the same template code against Python integers.  The pipeline functions below
// follow k_p256_table_odd / k_p256_affine_coz / k_p256_loop_odd (ecamd_p256_kernel.hip) step for step.
#include <cstring>
#define U29_INLINE_MUL 1
#include "../libecc_amd/csrc/ecamd_p256.h"

using namespace p256;

#ifdef ECAMD_COUNT_MADS
extern "C" {
uint64_t ecamd_mad_count = 0;
}
#endif

#ifndef SHIM_WB
#define SHIM_WB 4
#endif
constexpr int WB = SHIM_WB;
constexpr int NE = 1 << (WB - 1);  // table entries P, 3P, ..., (2 NE - 1)P

template <class T> static void ld(T &x, const uint32_t *a)
{
	memcpy(x.l, a, 36);
}
template <class T> static void st(uint32_t *a, const T &x)
{
	memcpy(a, x.l, 36);
}

extern "C" {
int t_wb(void)
{
	return WB;
}

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

// x, y: multiplication results (the Montgomery form of an imported point, value < 17/16 p); out: D.X, D.Y, P1.X, P1.Y, z
void t_dblu(const uint32_t *x, const uint32_t *y, uint32_t *out)
{
	MulOut<17>::type a, b;
	ld(a, x);
	ld(b, y);
	CoZ D, P1;
	FZ z;
	dblu(a, b, D, P1, z);
	st(out, D.X);
	st(out + 9, D.Y);
	st(out + 18, P1.X);
	st(out + 27, P1.Y);
	st(out + 36, z);
}

// p1x: FXc, p1y: FYc, p2x: FXc, p2y: FYc; out: R.X, R.Y, P1'.X, P1'.Y, r (5 x 9 limbs)
void t_zaddu(const uint32_t *p1x, const uint32_t *p1y, const uint32_t *p2x, const uint32_t *p2y, uint32_t *out)
{
	CoZ P1, P2, R;
	FR r;
	ld(P1.X, p1x);
	ld(P1.Y, p1y);
	ld(P2.X, p2x);
	ld(P2.Y, p2y);
	zaddu(P1, P2, R, r);
	st(out, R.X);
	st(out + 9, R.Y);
	st(out + 18, P1.X);
	st(out + 27, P1.Y);
	st(out + 36, r);
}

// E of the recoding; kw: KW words of k (KW = 8 or 17); e: KW + 1 words out; returns t
int t_recode_odd(const uint32_t *kw, int nkw, int slen, uint32_t *e)
{
	if (nkw == 8) {
		return recode_odd<8, WB>(e, kw, slen);
	}
	return recode_odd<17, WB>(e, kw, slen);
}
// the digits, top first: d[0..t)
int t_digits(const uint32_t *kw, int nkw, int slen, int32_t *d)
{
	uint32_t e[18];
	const int t = t_recode_odd(kw, nkw, slen, e);
	for (int j = 0; j < t; j++) {
		u32 idx;
		const bool neg = (nkw == 8) ? odd_digit<9, WB>(e, idx) : odd_digit<18, WB>(e, idx);
		d[j] = neg ? -(int32_t)(2 * idx + 1) : (int32_t)(2 * idx + 1);
	}
	return t;
}

// the odd-window table of an affine point (Montgomery-domain canonical limbs x, y):
// chain (k_p256_table_odd) + one inversion + back-substitution (k_p256_affine_coz);
// tab: NE entries x (x, y) canonical Montgomery limbs, 18 words each
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

// per-item arithmetic of the odd-window pipeline as the kernels run it (the MAD counter sees exactly these calls):
// chain + affine entries (the shared inversion excluded) and the window loop; returns 0, or 1 when an exceptional pair
// was met (the kernel's ECAMD_STATUS_REDO).  out: Jacobian X, Y, Z (27 words, Montgomery limbs)
int t_ladder_odd(const uint32_t *tab, const uint32_t *kw, int nkw, int slen, uint32_t *out)
{
	uint32_t e[18];
	const int t = t_recode_odd(kw, nkw, slen, e);
	u32 idx;
	Fcanon tx, ty;
	if (nkw == 8) {
		(void)odd_digit<9, WB>(e, idx);
	} else {
		(void)odd_digit<18, WB>(e, idx);
	}
	ld(tx, tab + 18 * idx);
	ld(ty, tab + 18 * idx + 9);
	Jac acc;
	acc.X = weaken<FX>(tx);
	acc.Y = weaken<FY>(ty);
	acc.Z = weaken<FZ>(constant<Fcanon>(K::ONE));
	bool bad = false, hz;
	for (int j = 1; j < t; j++) {
		for (int d = 0; d < WB; d++) {
			acc = dbl(acc);
		}
		const bool neg = (nkw == 8) ? odd_digit<9, WB>(e, idx) : odd_digit<18, WB>(e, idx);
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

// MADs of one item's chain (import and on-curve check excluded) and back-substitution: what k_p256_table_odd and
// k_p256_affine_coz execute per item beyond the shared inversion
uint64_t t_table_mads(const uint32_t *x, const uint32_t *y)
{
	Fcanon xa, ya;
	ld(xa, x);
	ld(ya, y);
	t_mads_reset();
	CoZ D, T[NE];
	FR r[NE];
	FZ z;
	dblu(xa, ya, D, T[0], z);
	for (int j = 1; j < NE; j++) {
		zaddu(D, T[j - 1], T[j], r[j]);
		z = weaken<FZ>(mul(z, r[j]));
	}
	Fmul zi = weaken<Fmul>(constant<Fcanon>(K::ONE));
	for (int j = NE - 1; j >= 1; j--) {
		const Fmul zi2 = weaken<Fmul>(sqr(zi));
		const Fmul zi3 = weaken<Fmul>(mul(zi2, zi));
		(void)canonical(mul(T[j].X, zi2));
		(void)canonical(mul(T[j].Y, zi3));
		if (j > 1) {
			zi = weaken<Fmul>(mul(zi, r[j]));
		}
	}
	return t_mads();
}
}
