// libecc_amd/csrc/ecamd_p256.h -- secp256r1 group law on radix-2^29 lazy-reduced elements.
//
// Jacobian coordinates (x = X/Z^2, y = Y/Z^3), a = -3:
//   doubling  4M + 4S   (dbl-2001-b with Z3 = 2YZ and 8 gamma^2 = 2 (2 gamma)^2; 5M + 3S under one reduction fewer
//                        with P256_FUSED_Y3_DBL, see below)
//   addition 12M + 4S   (add-1998-cmo-2)
// against 16 / 17 multiplications for the reference's complete projective formulas
// (curves/prj_pt.c:892-950, 971-1071 in /root/reference/src).  Jacobian addition is NOT
// complete; the scalar multiplication kernel (ecamd_p256_kernel.hip) keeps an explicit
// "accumulator is infinity" flag, tests the one remaining exceptional case (H = 0: P + P or
// P + (-P)) exactly through Z3, and hands such items to the complete-formula kernel, so the
// observable result is the reference's for EVERY input.
//
// Every intermediate is a bound-tracked u29::F<LB, TB, VB>; the carry()/fold() calls below are
// exactly the ones the static_asserts of ecamd_u29.h demand.
#pragma once
#include "ecamd_u29.h"

namespace p256 {
using namespace u29;

// constants in the Montgomery domain R = 2^261 (tools/u29_consts.py)
struct K {
	static constexpr u32 R2[9] = {0x00000c00, 0x00000000, 0x1fff0000, 0x1fdfffff, 0x1fbfffff,
				      0x1fffffff, 0x1fffffff, 0x1ffffffe, 0x00000013};
	static constexpr u32 ONE[9] = {0x00000020, 0x00000000, 0x00000000, 0x1fffc000, 0x1fffffff,
				       0x1fffffff, 0x1f7fffff, 0x03ffffff, 0x00000000};
	static constexpr u32 BM[9] = {0x1897bbfb, 0x1cdf6229, 0x018486c4, 0x01732821, 0x1dad59e0,
				      0x0abf7212, 0x1a06d110, 0x17721d20, 0x008600c3};
};

template <class T> U29_FN T constant(const u32 (&c)[9])
{
	T r;
#pragma unroll
	for (int i = 0; i < 9; i++) {
		r.l[i] = c[i];
	}
	return r;
}

// loop-carried accumulator classes of the scalar multiplication
typedef F<MASK + 16, (2ull << 24), 17> FX;         // fold() output / Montgomery form of an input
typedef F<MASK + 16, (6ull << 24) + 16, 96> FY;     // carry() of a subtraction result, value < 6p
typedef F<2ull * MASK, (4ull << 24), 56> FZ;      // 2 * (multiplication result), value < 3.5p
// table entries keep Y folded (value < 17/16 p), so that the negation 2p - Y of a negative
// window digit stays small; FYsel is the common class of Y and its carried negation
typedef F<MASK + 16, (4ull << 24), 49> FYsel;
struct TabEnt {
	FX X;
	FX Y;
	FZ Z;
};

struct Jac {
	FX X;
	FY Y;
	FZ Z;
};

// ---- inversion ----
// P256_INV_FERMAT=1 brings back x^(p-2) (A/B builds: tools/build_variant.py); the default is the divstep inversion below.
#ifndef P256_INV_FERMAT
#define P256_INV_FERMAT 0
#endif

// Constant-time "safegcd" inversion (Bernstein-Yang divsteps, in the form of libsecp256k1's modinv32 with 29-bit limbs): no field
// multiplication at all.  f = p, g = x, and (d, e) follow (f, g) mod p through the same 2x2 transition matrices, so that
// d x = f e0 and e x = g e0 (mod p) hold throughout; once g = 0, f = +-1 and d = +-e0 / x.
//   * State: nine signed 29-bit limbs each (limbs 0..7 in [0, 2^29), the top limb carries the sign); |f|, |g| <= p and d, e stay
//     in (-2p, p).
//   * A batch is SAFEGCD_N = 29 divsteps on the low words of f and g alone; it yields a matrix t = (u v; q r) with
//     t (f, g) = 2^29 (f', g') and |u| + |v|, |q| + |r| <= 2^29, which is then applied to the full (f, g) (exact division) and to
//     (d, e) mod p: a multiple m p is added that clears the low 29 bits.  p = -1 mod 2^87 makes m the low 29 bits of the sum
//     itself, and m p = m (p + 1) - m costs four products, not nine (the multipliers of the Montgomery reduction again).
//   * Count: the variant used starts at delta = 1/2 (zeta = -(delta + 1/2) = -1).  For it, 590 divsteps bring g to 0 for every
//     odd modulus below 2^256 and every 0 <= g < f: proven by the convex-hull computation of P. Wuille
//     (github.com/sipa/safegcd-bounds; libsecp256k1 doc/safegcd_implementation.md, whose modinv32 runs 20 x 30 = 600 on that
//     ground).  Here SAFEGCD_BATCHES x SAFEGCD_N = 21 x 29 = 609 >= 590, ALWAYS all of them: no early exit, every choice is a
//     mask (the values inverted derive from secret scalars in the masked mode).
//   * x = 0 keeps g = 0 and d = 0 through every batch: inv(0) = 0, as x^(p-2) gives.
// tests/test_p256_inv_host.py drives this code on the host against pow(x, p - 2, p) and checks g = 0, f = +-1 at the end.
typedef int32_t i32;
typedef int64_t i64;
constexpr int SAFEGCD_N = 29;
constexpr int SAFEGCD_BATCHES = 21;
static_assert(SAFEGCD_N == W && SAFEGCD_N * SAFEGCD_BATCHES >= 590, "divstep count below the proven bound");
struct DivMat {
	i32 u, v, q, r;
};

// SAFEGCD_N divsteps on the low words; zeta = -(delta + 1/2).  Unsigned arithmetic throughout (wrap-around is meant).
U29_FN i32 divsteps29(i32 zeta, u32 f, u32 g, DivMat &t)
{
	u32 u = 1, v = 0, q = 0, r = 1;
#pragma unroll
	for (int i = 0; i < SAFEGCD_N; i++) {
		u32 m1 = (u32)(zeta >> 31);          // zeta < 0
		const u32 m2 = 0u - (g & 1u);       // g odd
		const u32 x = (f ^ m1) - m1, y = (u ^ m1) - m1, z = (v ^ m1) - m1;  // +-(f, u, v)
		g += x & m2;
		q += y & m2;
		r += z & m2;
		m1 &= m2;                            // swap: zeta < 0 and g odd
		zeta = (i32)((u32)zeta ^ m1) - 1;    // -zeta - 2 or zeta - 1
		f += g & m1;
		u += q & m1;
		v += r & m1;
		g >>= 1;
		u <<= 1;
		v <<= 1;
	}
	t.u = (i32)u;
	t.v = (i32)v;
	t.q = (i32)q;
	t.r = (i32)r;
	return zeta;
}

// (f, g) <- t (f, g) / 2^29, exact
U29_FN void safegcd_update_fg(i32 *f, i32 *g, const DivMat &t)
{
	i64 cf = (i64)t.u * f[0] + (i64)t.v * g[0];
	i64 cg = (i64)t.q * f[0] + (i64)t.r * g[0];
	cf >>= W;
	cg >>= W;
#pragma unroll
	for (int i = 1; i < 9; i++) {
		cf += (i64)t.u * f[i] + (i64)t.v * g[i];
		cg += (i64)t.q * f[i] + (i64)t.r * g[i];
		f[i - 1] = (i32)((u32)cf & MASK);
		g[i - 1] = (i32)((u32)cg & MASK);
		cf >>= W;
		cg >>= W;
	}
	f[8] = (i32)cf;
	g[8] = (i32)cg;
}

// (d, e) <- t (d, e) / 2^29 mod p, kept in (-2p, p)
U29_FN void safegcd_update_de(i32 *d, i32 *e, const DivMat &t)
{
	constexpr i32 pq[9] = {0, 0, 0, (i32)P256::Q3, 0, 0, (i32)P256::Q6, (i32)P256::Q7, (i32)P256::Q8};  // p + 1
	const i32 sd = d[8] >> 31, se = e[8] >> 31;
	// multiples of p that bring a negative d / e back above -p ...
	i32 md = (t.u & sd) + (t.v & se);
	i32 me = (t.q & sd) + (t.r & se);
	i64 cd = (i64)t.u * d[0] + (i64)t.v * e[0];
	i64 ce = (i64)t.q * d[0] + (i64)t.r * e[0];
	// ... lowered to m = the sum's low 29 bits (mod 2^29): sum + m p = sum - m + m (p + 1) is then a multiple of 2^29
	md -= (i32)(((u32)md - (u32)cd) & MASK);
	me -= (i32)(((u32)me - (u32)ce) & MASK);
	cd -= md;
	ce -= me;
	cd >>= W;
	ce >>= W;
#pragma unroll
	for (int i = 1; i < 9; i++) {
		cd += (i64)t.u * d[i] + (i64)t.v * e[i];
		ce += (i64)t.q * d[i] + (i64)t.r * e[i];
		if (pq[i] != 0) {
			cd += (i64)pq[i] * md;
			ce += (i64)pq[i] * me;
		}
		d[i - 1] = (i32)((u32)cd & MASK);
		e[i - 1] = (i32)((u32)ce & MASK);
		cd >>= W;
		ce >>= W;
	}
	d[8] = (i32)cd;
	e[8] = (i32)ce;
}

// All SAFEGCD_BATCHES batches from f = p, g = x (0 <= x < p), d = 0, e = e0 (0 <= e0 < p); returns the number of divsteps done.
U29_FN int safegcd_run(i32 *f, i32 *g, i32 *d, const u32 *x, const u32 *e0)
{
	i32 e[9];
#pragma unroll
	for (int i = 0; i < 9; i++) {
		f[i] = (i32)P256::P[i];
		g[i] = (i32)x[i];
		d[i] = 0;
		e[i] = (i32)e0[i];
	}
	i32 zeta = -1;
	int steps = 0;
#pragma unroll 1
	for (int b = 0; b < SAFEGCD_BATCHES; b++) {
		DivMat t;
		zeta = divsteps29(zeta, (u32)f[0] | ((u32)f[1] << W), (u32)g[0] | ((u32)g[1] << W), t);
		safegcd_update_de(d, e, t);
		safegcd_update_fg(f, g, t);
		steps += SAFEGCD_N;
	}
	return steps;
}

// d in (-2p, p), to be negated when f is negative  ->  the residue in [0, p)
U29_FN Fcanon safegcd_normalize(i32 *d, i32 fsign)
{
	i32 add = d[8] >> 31;
#pragma unroll
	for (int i = 0; i < 9; i++) {
		d[i] += (i32)P256::P[i] & add;  // now in (-p, p)
	}
	const i32 neg = fsign >> 31;
#pragma unroll
	for (int i = 0; i < 9; i++) {
		d[i] = (d[i] ^ neg) - neg;
	}
#pragma unroll
	for (int i = 0; i < 8; i++) {
		d[i + 1] += d[i] >> W;
		d[i] &= (i32)MASK;
	}
	add = d[8] >> 31;
#pragma unroll
	for (int i = 0; i < 9; i++) {
		d[i] += (i32)P256::P[i] & add;
	}
#pragma unroll
	for (int i = 0; i < 8; i++) {
		d[i + 1] += d[i] >> W;
		d[i] &= (i32)MASK;
	}
	Fcanon r;
#pragma unroll
	for (int i = 0; i < 9; i++) {
		r.l[i] = (u32)d[i];
	}
	return r;
}

// x = a R  ->  a^-1 R:  the divsteps invert the integer a R, and e0 = R^2 mod p puts the result back into the Montgomery domain
// for nothing (d = +-e0 / x = a^-1 R), where a Montgomery multiplication by R^3 mod p would otherwise follow.
U29_FN Fmul inv_safegcd(const Fmul &x)
{
	const Fcanon xc = canonical(x);
	i32 f[9], g[9], d[9];
	safegcd_run(f, g, d, xc.l, K::R2);
	return weaken<Fmul>(safegcd_normalize(d, f[8]));
}

// x^(p-2): e2, e4, e8, e16, e32 ladder then the 2^32, 2^128, 2^32, 2^16, 2^8, 2^4, 2^2, 2^2 tail
// (255 squarings + 13 multiplications; exponent checked in tools/u29_consts.py)
U29_FN Fmul sqr_n(Fmul x, int n)
{
#pragma unroll 1
	for (int i = 0; i < n; i++) {
		x = weaken<Fmul>(sqr(x));
	}
	return x;
}
#define P256_MULW(a, b) weaken<Fmul>(mul(a, b))
U29_FN Fmul inv_fermat(const Fmul &x)
{
	const Fmul e2 = P256_MULW(sqr_n(x, 1), x);
	const Fmul e4 = P256_MULW(sqr_n(e2, 2), e2);
	const Fmul e8 = P256_MULW(sqr_n(e4, 4), e4);
	const Fmul e16 = P256_MULW(sqr_n(e8, 8), e8);
	const Fmul e32 = P256_MULW(sqr_n(e16, 16), e16);
	Fmul r = P256_MULW(sqr_n(e32, 32), x);
	r = P256_MULW(sqr_n(r, 128), e32);
	r = P256_MULW(sqr_n(r, 32), e32);
	r = P256_MULW(sqr_n(r, 16), e16);
	r = P256_MULW(sqr_n(r, 8), e8);
	r = P256_MULW(sqr_n(r, 4), e4);
	r = P256_MULW(sqr_n(r, 2), e2);
	r = P256_MULW(sqr_n(r, 2), x);
	return r;
}

U29_FN Fmul inv(const Fmul &x)
{
#if P256_INV_FERMAT
	return inv_fermat(x);
#else
	return inv_safegcd(x);
#endif
}

// ---- Y3 as one two-product Montgomery reduction (u29::mul2) ----
// Y3 is a difference of two products that nothing else reads, in dbl, madd and add_jac alike.  With one operand of the second
// product negated against a multiple of p, both products go into the same column accumulators and are reduced ONCE: the second
// reduction (36 MADs, 17 + 17 column-carry instructions) and the trailing sub() + carry() fall away.  One switch per site
// (A/B builds: tools/build_variant.py); profiles/r24_p256_fused_y3.md has the measurements.  dbl's is on.  madd's (add_jac goes
// with it) is off: built alone it met the acceptance rule of that note in one of two sessions only, so the formula stays the
// parent's, 8M + 3S with two reductions for Y3.
#ifndef P256_FUSED_Y3_DBL
#define P256_FUSED_Y3_DBL 1
#endif
#ifndef P256_FUSED_Y3_MADD
#define P256_FUSED_Y3_MADD 0
#endif
// 2^LOGC p - b: the operand that stands for -b in a fused product
template <int LOGC, int S, class B> U29_FN auto neg(const B &b)
{
	F<0, 0, 0> zero;
#pragma unroll
	for (int i = 0; i < 9; i++) {
		zero.l[i] = 0;
	}
	return sub<LOGC, S>(zero, b);
}

// ---- doubling: (X, Y, Z) -> 2 (X, Y, Z) ----
U29_FN Jac dbl(const Jac &P)
{
	const auto delta = sqr(P.Z);                         // Z^2
	const auto gamma = sqr(P.Y);                         // Y^2
	const auto beta4 = mul(P.X, mul_small<4>(gamma));    // 4 X Y^2
	const auto t1 = sub<1, 0>(P.X, delta);               // X - Z^2 (+2p)
	const auto t2 = add(P.X, delta);                     // X + Z^2
	const auto alpha0 = mul(t1, t2);
	const auto alpha = carry(mul_small<3>(alpha0));      // 3 (X - Z^2)(X + Z^2)
	const auto a2 = sqr(alpha);
	const auto beta8 = mul_small<2>(beta4);
	const auto x3 = fold(sub<2, 1>(a2, beta8));          // alpha^2 - 8 beta
	const auto t4 = sub<1, 1>(beta4, x3);                // 4 beta - X3
#if P256_FUSED_Y3_DBL
	// alpha t4 - 8 gamma^2 = alpha t4 + (2 gamma) (16p - 4 gamma).  The squaring form 2 (2 gamma)^2 is out of reach: a sum
	// a b + c^2 cannot carry the minus sign (negating the alpha t4 side instead gives -Y3), so the 8 gamma^2 side costs 81
	// products where the squaring took 45 and the MAD count of a doubling stays what it was; what goes is the second
	// reduction's column carries and the trailing sub() + carry().  One carry() is needed whichever way 8 gamma^2 is split:
	// t4's limbs reach 2^31, so alpha t4 takes 9 2^60 of a column and leaves (k gamma) (C p - (8 / k) gamma) 5 2^60, which no
	// k in {1, 2, 4, 8} meets with uncarried bias limbs (2^61.3 at best, k = 2).  k = 2 with the negated side carried is 9 2^59.
	const auto n4 = carry(neg<4, 2>(mul_small<4>(gamma)));  // 16p - 4 gamma
	const auto y3 = mul2(alpha, t4, mul_small<2>(gamma), n4);
#else
	const auto g4 = sqr(mul_small<2>(gamma));            // 4 gamma^2
	const auto g8 = mul_small<2>(g4);                    // 8 gamma^2
	const auto y3a = mul(alpha, t4);
	const auto y3 = carry(sub<2, 1>(y3a, g8));
#endif
	const auto z3 = mul_small<2>(mul(P.Y, P.Z));         // 2 Y Z
	Jac R;
	R.X = weaken<FX>(x3);
	R.Y = weaken<FY>(y3);
	R.Z = weaken<FZ>(z3);
	return R;
}

// ---- addition: (X1, Y1, Z1) + (X2, Y2, Z2), Z2 arbitrary; returns Z3 as the raw
//      multiplication result too (exact digits) for the H == 0 test ----
template <class FX2, class FY2, class FZ2>
U29_FN Jac add_jac(const Jac &P, const FX2 &X2, const FY2 &Y2, const FZ2 &Z2, bool &h_is_zero)
{
	const auto z1z1 = sqr(P.Z);
	const auto z2z2 = sqr(Z2);
	const auto u1 = mul(P.X, z2z2);
	const auto u2 = mul(X2, z1z1);
	const auto s1 = mul(mul(P.Y, Z2), z2z2);
	const auto s2 = mul(mul(Y2, P.Z), z1z1);
	const auto h = carry(sub<1, 0>(u2, u1));
	const auto r = carry(sub<1, 0>(s2, s1));
	const auto hh = sqr(h);
	const auto hhh = mul(h, hh);
	const auto v = mul(u1, hh);
	const auto r2 = sqr(r);
	const auto x3 = fold(sub<2, 2>(r2, add(hhh, mul_small<2>(v))));
	const auto t5 = sub<1, 1>(v, x3);
#if P256_FUSED_Y3_MADD
	const auto y3 = mul2(r, t5, s1, neg<1, 0>(hhh));     // as in madd; no carry needed here either
#else
	const auto m1 = mul(r, t5);
	const auto m2 = mul(s1, hhh);
	const auto y3 = carry(sub<1, 0>(m1, m2));
#endif
	const auto z3 = mul(mul(P.Z, Z2), h);
	h_is_zero = is_zero_mulout(z3);
	Jac R;
	R.X = weaken<FX>(x3);
	R.Y = weaken<FY>(y3);
	R.Z = weaken<FZ>(z3);
	return R;
}

// ---- mixed addition: (X1, Y1, Z1) + affine (x2, y2), 8M + 3S (madd): the window table is made
//      affine by k_p256_affine (one shared inversion per 8 items), which saves 4M + 1S per window ----
typedef F<(1ull << 29) + MASK, (3ull << 24), 48> FYaff;  // y2 or 2p - y2 of an affine (canonical) table entry
template <class FY2> U29_FN Jac madd(const Jac &P, const Fcanon &X2, const FY2 &Y2, bool &h_is_zero)
{
	const auto z1z1 = sqr(P.Z);
	const auto u2 = mul(X2, z1z1);
	const auto s2 = mul(mul(Y2, P.Z), z1z1);
	const auto h = carry(sub<1, 1>(u2, P.X));
	const auto r = carry(sub<3, 1>(s2, P.Y));
	const auto hh = sqr(h);
	const auto hhh = mul(h, hh);
	const auto v = mul(P.X, hh);
	const auto r2 = sqr(r);
	const auto x3 = fold(sub<2, 2>(r2, add(hhh, mul_small<2>(v))));
	const auto t5 = sub<1, 1>(v, x3);
#if P256_FUSED_Y3_MADD
	// r t5 - Y1 hhh = r t5 + Y1 (2p - hhh).  The negation goes on hhh and not on Y1: hhh is a multiplication result below
	// 19/16 p with exact digits, so 2p dominates it limb by limb and the negated limbs stay below 2^30 -- Y1 hhh' takes 9 2^59 of
	// a column beside r t5's 9 2^60 and no carry() is needed; Y1 (value < 6p, limbs above 2^29) would take 8p and a carry().
	const auto y3 = mul2(r, t5, P.Y, neg<1, 0>(hhh));
#else
	const auto y3 = carry(sub<1, 0>(mul(r, t5), mul(P.Y, hhh)));
#endif
	const auto z3 = mul(P.Z, h);
	h_is_zero = is_zero_mulout(z3);
	Jac R;
	R.X = weaken<FX>(x3);
	R.Y = weaken<FY>(y3);
	R.Z = weaken<FZ>(z3);
	return R;
}
U29_FN FYaff neg_aff(const Fcanon &y)
{
	F<0, 0, 0> zero;
#pragma unroll
	for (int i = 0; i < 9; i++) {
		zero.l[i] = 0;
	}
	return weaken<FYaff>(sub<1, 0>(zero, y));
}

// 2p - Y, limbs re-normalised: the negated table entry of a negative window digit
U29_FN FYsel neg_y(const FX &y)
{
	F<0, 0, 0> zero;
#pragma unroll
	for (int i = 0; i < 9; i++) {
		zero.l[i] = 0;
	}
	return weaken<FYsel>(carry(sub<1, 1>(zero, y)));
}

// ---- co-Z arithmetic (Meloni; the odd-multiple table of Longa-Miri): two points that share one Z ----
// The window table [1, 3, ..., 2^w - 1]P is built as 2P then (2j + 1)P = 2P + (2j - 1)P by co-Z additions that keep 2P on
// the Z of the new entry.  Each step multiplies Z by r = X(2P) - X((2j - 1)P), so Z_j = Z_0 r_1 ... r_j and the affine pass
// walks the entries down from ONE inverse: 1/Z_{j-1} = r_j / Z_j.
typedef F<MASK + 16, (2ull << 24), 32> FXc;        // co-Z X: fold() output or multiplication result (value < 2p)
typedef F<MASK + 16, (4ull << 24), 63> FYc;        // co-Z Y: value < 63/16 p (its top limb stays below 4p's)
typedef F<MASK + 15, (8ull << 24), 128> FR;         // carry() of X1 - X2 + 4p: the Z ratio of one co-Z addition
struct CoZ {
	FXc X;
	FYc Y;
};

// dblu: affine P = (x, y) -> 2P and P, both on Z = 2y (3M + 3S; doubling with Z = 1 as in dbl, and P' = (4 x y^2, 8 y^4)
// falls out of it).  y != 0: the group order is an odd prime, so P has no order 2.
template <class AX, class AY> U29_FN void dblu(const AX &x, const AY &y, CoZ &D, CoZ &P1, FZ &z)
{
	const Fcanon one = constant<Fcanon>(K::ONE);
	const auto gamma = sqr(y);                           // y^2
	const auto beta4 = mul(x, mul_small<4>(gamma));      // 4 x y^2
	const auto t1 = sub<1, 0>(x, one);                   // x - 1 (+2p)
	const auto t2 = add(x, one);                         // x + 1
	const auto alpha = carry(mul_small<3>(mul(t1, t2))); // 3 (x^2 - 1)
	const auto a2 = sqr(alpha);
	const auto x3 = fold(sub<2, 1>(a2, mul_small<2>(beta4)));
	const auto g8 = mul_small<2>(sqr(mul_small<2>(gamma)));  // 8 y^4
	const auto y3 = fold(sub<2, 2>(mul(alpha, sub<1, 1>(beta4, x3)), g8));
	D.X = weaken<FXc>(x3);
	D.Y = weaken<FYc>(y3);
	P1.X = weaken<FXc>(beta4);
	P1.Y = weaken<FYc>(carry(g8));
	z = weaken<FZ>(mul_small<2>(y));
}

// zaddu: co-Z P1 + P2 -> R = P1 + P2 and P1 rescaled, both on Z r with r = X1 - X2 (5M + 2S).  Callers guarantee
// P1 != +-P2 (X1 != X2): in the table chain P1 = 2P and P2 = (2j - 1)P, and 2P = +-(2j - 1)P would need a point order
// dividing 2j + 1 or 2j - 3 <= 31, while the group order is a prime far above that.
U29_FN void zaddu(CoZ &P1, const CoZ &P2, CoZ &R, FR &r)
{
	const auto h = carry(sub<2, 1>(P1.X, P2.X));         // X1 - X2 (+4p)
	const auto c = sqr(h);
	const auto w1 = mul(P1.X, c);                        // X1 (X1 - X2)^2
	const auto w2 = mul(P2.X, c);                        // X2 (X1 - X2)^2
	const auto dy = carry(sub<2, 1>(P1.Y, P2.Y));        // Y1 - Y2 (+4p)
	const auto d = sqr(dy);
	const auto a1 = mul(P1.Y, sub<1, 0>(w1, w2));        // Y1 (W1 - W2)
	const auto x3 = fold(sub<2, 1>(d, add(w1, w2)));     // (Y1 - Y2)^2 - W1 - W2
	const auto y3 = carry(sub<1, 0>(mul(dy, sub<1, 1>(w1, x3)), a1));
	R.X = weaken<FXc>(x3);
	R.Y = weaken<FYc>(y3);
	P1.X = weaken<FXc>(w1);
	P1.Y = weaken<FYc>(a1);
	r = weaken<FR>(h);
}

// ---- regular odd-digit recoding (Joye-Tunstall) over WB-bit windows ----
// k' = k, or k + q when k is even (same point, odd scalar; branch-free: the masked mode runs the same code), then
// k' = sum_{j < t} d_j 2^(WB j) with every d_j odd in [-(2^WB - 1), 2^WB - 1]:  d_j = 2 e_j - (2^WB - 1) where e_j are the
// WB-bit windows of E = (k' >> 1) + 2^(WB t - 1), t = ceil((max(8 slen, 256) + 1) / WB) (k' < 2^(max(8 slen, 256) + 1)).
// The top window has e >= 2^(WB-1): its digit is positive.  kw: k in KW little-endian words; e: E in KW + 1 words, LEFT-
// aligned (the top window in the top WB bits of e[KW]) -- E << s = ((k' - 1) << (s - 1)) + 2^(32 (KW + 1) - 1).  Returns t.
// KW == 8 serves scalars of at most 32 bytes only, so t (and every shift) is a compile-time constant there.
struct QOrder {
	static constexpr u32 W[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu};
};
template <int KW, int WB> U29_FN int recode_odd(u32 *e, const u32 *kw, int slen)
{
	constexpr int NW = KW + 1;
	const u32 even = (kw[0] & 1u) - 1u;  // all ones when k is even
	u64 c = 0;
#pragma unroll
	for (int w = 0; w < KW; w++) {
		c += (u64)kw[w] + (w < 8 ? (QOrder::W[w] & even) : 0u);
		e[w] = (u32)c;
		c >>= 32;
	}
	e[KW] = (u32)c;
	e[0] &= ~1u;  // k' - 1
	const int nbits = (KW == 8) ? 257 : ((8 * slen > 256 ? 8 * slen : 256) + 1);
	const int t = (nbits + WB - 1) / WB;
	const int sh = 32 * NW - WB * t - 1;
	for (int s = 0; s < (sh >> 5); s++) {
#pragma unroll
		for (int w = NW - 1; w > 0; w--) {
			e[w] = e[w - 1];
		}
		e[0] = 0;
	}
	const int bs = sh & 31;
#pragma unroll
	for (int w = NW - 1; w > 0; w--) {
		e[w] = (u32)((((u64)e[w] << 32) | e[w - 1]) >> (32 - bs));
	}
	e[0] = (u32)(((u64)e[0] << 32) >> (32 - bs));
	e[NW - 1] |= 0x80000000u;
	return t;
}
// next window of a left-aligned E (top WB bits of e[NW - 1]), E shifted on; idx: table entry of |d| = 2 idx + 1; returns d < 0
template <int NW, int WB> U29_FN bool odd_digit(u32 *e, u32 &idx)
{
	constexpr u32 HALF = 1u << (WB - 1);
	const u32 win = e[NW - 1] >> (32 - WB);
#pragma unroll
	for (int w = NW - 1; w > 0; w--) {
		e[w] = (e[w] << WB) | (e[w - 1] >> (32 - WB));
	}
	e[0] <<= WB;
	const bool neg = win < HALF;
	idx = (win & (HALF - 1)) ^ (neg ? HALF - 1 : 0u);
	return neg;
}

// ---- the same recoding in 64 digits of 4 bits, for scalars below 2^256 (at most 32 bytes) ----
// k + q costs a 257th bit, hence a 65th digit.  Instead the odd k' stays below 2^256 and carries a sign:
//   k odd: k' = k, +;   k even, k < q: k' = q - k, -;   k even, k > q: k' = k - q, +      (k = q is odd)
// so that [k]P = +-[k']P.  Branch-free (the masked mode runs the same code): d = k - q with borrow b, d negated when b is set.
// E = (k' - 1) / 2 + 2^255 fills the eight words of e exactly, so it is left-aligned as it stands: odd_digit<8, 4> reads its 64
// windows, top first, and the top one is >= 8 (a positive digit).  Returns the sign (true: negative); the caller flips the
// `neg` of every digit with it, which negates the whole sum.
U29_FN bool recode_odd64(u32 *e, const u32 *kw)
{
	const u32 even = (kw[0] & 1u) - 1u;  // all ones when k is even
	u32 d[8];
	u32 borrow = 0;
#pragma unroll
	for (int w = 0; w < 8; w++) {
		const u64 x = (u64)kw[w] - QOrder::W[w] - borrow;
		d[w] = (u32)x;
		borrow = (u32)(x >> 63);
	}
	const u32 below = 0u - borrow;  // all ones when k < q
	u64 c = borrow;
#pragma unroll
	for (int w = 0; w < 8; w++) {
		c += (u64)(d[w] ^ below);  // -d = ~d + 1
		d[w] = ((u32)c & even) | (kw[w] & ~even);
		c >>= 32;
	}
#pragma unroll
	for (int w = 0; w < 7; w++) {
		e[w] = (d[w] >> 1) | (d[w + 1] << 31);
	}
	e[7] = (d[7] >> 1) | 0x80000000u;
	return (even & below) != 0u;
}

U29_FN TabEnt to_tab(const Jac &P)
{
	TabEnt T;
	T.X = P.X;
	T.Y = weaken<FX>(fold(P.Y));
	T.Z = P.Z;
	return T;
}

}  // namespace p256
