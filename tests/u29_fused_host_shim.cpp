// tests/u29_fused_host_shim.cpp -- TEST INFRASTRUCTURE: the two-product Montgomery primitives of libecc_amd/csrc/ecamd_u29.h (mul2,
// mulsqr) and the formulas that use them (ecamd_p256.h: dbl, madd, add_jac), compiled for the host beside everything that
// tests/u29_host_shim.cpp exports (t_dbl, t_add, t_madd, ...).
//   * as a shared library, built with both switches (P256_FUSED_Y3_DBL, P256_FUSED_Y3_MADD) at 1 and with both at 0,
//     tests/test_u29_fused_host.py drives it against Python integers and one build against the other;
//   * with -DU29_FUSED_MAIN it is a stand-alone program: mul2 / mulsqr against the header's own mul / sqr / add on operands at the
//     bounds of their classes and on random ones, then a chain of windows (4 dbl + 1 madd) whose affine end point it prints --
//     the form in which it is built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include "u29_host_shim.cpp"

// the operand classes of the two fused sites, derived by the expressions of dbl() and madd() themselves
typedef decltype(fold(std::declval<FY>())) TX3;
typedef decltype(sqr(std::declval<FZ>())) TDelta;
typedef decltype(sqr(std::declval<FY>())) TGamma;
typedef decltype(mul(std::declval<FX>(), mul_small<4>(std::declval<TGamma>()))) TBeta4;
typedef decltype(carry(mul_small<3>(mul(sub<1, 0>(std::declval<FX>(), std::declval<TDelta>()), add(std::declval<FX>(), std::declval<TDelta>()))))) TAlpha;
typedef decltype(sub<1, 1>(std::declval<TBeta4>(), std::declval<TX3>())) TT4;
typedef decltype(mul_small<2>(std::declval<TGamma>())) TG2;
typedef decltype(carry(neg<4, 2>(mul_small<4>(std::declval<TGamma>())))) TN4;
typedef decltype(carry(std::declval<TG2>())) TG2c;  // mulsqr's squared operand: 2 gamma, carried

typedef decltype(mul(std::declval<Fcanon>(), std::declval<TDelta>())) TU2;
typedef decltype(mul(mul(std::declval<FYaff>(), std::declval<FZ>()), std::declval<TDelta>())) TS2;
typedef decltype(carry(sub<1, 1>(std::declval<TU2>(), std::declval<FX>()))) TH;
typedef decltype(carry(sub<3, 1>(std::declval<TS2>(), std::declval<FY>()))) TR;
typedef decltype(sqr(std::declval<TH>())) THH;
typedef decltype(mul(std::declval<TH>(), std::declval<THH>())) THHH;
typedef decltype(sub<1, 1>(std::declval<decltype(mul(std::declval<FX>(), std::declval<THH>()))>(), std::declval<TX3>())) TT5;
typedef decltype(neg<1, 0>(std::declval<THHH>())) TNH;

typedef decltype(mul2(std::declval<TAlpha>(), std::declval<TT4>(), std::declval<TG2>(), std::declval<TN4>())) TY3dbl;
typedef decltype(mul2(std::declval<TR>(), std::declval<TT5>(), std::declval<FY>(), std::declval<TNH>())) TY3madd;
typedef decltype(mulsqr(std::declval<TAlpha>(), std::declval<TT4>(), std::declval<TG2c>())) TY3sqr;

template <class T> static void bounds(uint64_t *o)
{
	o[0] = T::LB;
	o[1] = T::TB;
	o[2] = T::VB;
}
template <class T> static T load(const uint32_t *a)
{
	T x;
	memcpy(x.l, a, 36);
	return x;
}

extern "C" {
// (LB, TB, VB) of: dbl's a, b, c, d and result; madd's a, b, c, d and result; mulsqr's c and result
void t_fused_bounds(uint64_t *o)
{
	bounds<TAlpha>(o);
	bounds<TT4>(o + 3);
	bounds<TG2>(o + 6);
	bounds<TN4>(o + 9);
	bounds<TY3dbl>(o + 12);
	bounds<TR>(o + 15);
	bounds<TT5>(o + 18);
	bounds<FY>(o + 21);
	bounds<TNH>(o + 24);
	bounds<TY3madd>(o + 27);
	bounds<TG2c>(o + 30);
	bounds<TY3sqr>(o + 33);
}
void t_mul2_dbl(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out)
{
	const auto r = mul2(load<TAlpha>(a), load<TT4>(b), load<TG2>(c), load<TN4>(d));
	memcpy(out, r.l, 36);
}
void t_mul2_madd(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out)
{
	const auto r = mul2(load<TR>(a), load<TT5>(b), load<FY>(c), load<TNH>(d));
	memcpy(out, r.l, 36);
}
void t_mulsqr(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out)
{
	const auto r = mulsqr(load<TAlpha>(a), load<TT4>(b), load<TG2c>(c));
	memcpy(out, r.l, 36);
}
int t_fused_switches() { return P256_FUSED_Y3_DBL | (P256_FUSED_Y3_MADD << 1); }
}

#ifdef U29_FUSED_MAIN
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}
static int failures = 0;

// the canonical residue of x R (x < 8p, any limbs): both sides of a comparison go through it
template <class T> static Fcanon canon(const T &x) { return canonical(mul(fold(x), constant<Fcanon>(K::R2))); }
static void expect_same(const Fcanon &x, const Fcanon &y, const char *what)
{
	if (memcmp(x.l, y.l, 36) != 0) {
		failures++;
		fprintf(stderr, "FAIL %s\n", what);
	}
}
// mode 0: every limb at its bound; 1: random below the bounds; the value bound is then met by lowering the top limb
template <class T> static T operand(int mode)
{
	T x;
	for (int i = 0; i < 9; i++) {
		const uint64_t hi = i < 8 ? T::LB : T::TB;
		x.l[i] = (uint32_t)(mode == 0 ? hi : rng() % (hi + 1));
	}
	// value < VB p / 16 holds when the top limb is below VB 2^20 - 2^3 or so (p > 2^256 - 2^225, eight loose limbs add < 2^236)
	const uint64_t vtop = T::VB * (1ull << 20) - T::VB * 8 - 32;
	if (x.l[8] > vtop) {
		x.l[8] = (uint32_t)vtop;
	}
	return x;
}
template <class A, class B, class C, class D> static void check_mul2(int mode, const char *what)
{
	const A a = operand<A>(mode);
	const B b = operand<B>(mode);
	const C c = operand<C>(mode);
	const D d = operand<D>(mode);
	const auto got = mul2(a, b, c, d);
	for (int i = 0; i < 8; i++) {
		if (got.l[i] > MASK) {
			failures++;
			fprintf(stderr, "FAIL %s: loose digit\n", what);
		}
	}
	if (got.l[8] > decltype(got)::TB) {
		failures++;
		fprintf(stderr, "FAIL %s: top limb above its bound\n", what);
	}
	expect_same(canon(got), canon(add(mul(a, b), mul(c, d))), what);
}
template <class A, class B, class C> static void check_mulsqr(int mode, const char *what)
{
	const A a = operand<A>(mode);
	const B b = operand<B>(mode);
	const C c = operand<C>(mode);
	const auto got = mulsqr(a, b, c);
	if (got.l[8] > decltype(got)::TB) {
		failures++;
		fprintf(stderr, "FAIL %s: top limb above its bound\n", what);
	}
	expect_same(canon(got), canon(add(mul(a, b), sqr(c))), what);
}

int main(int argc, char **argv)
{
	const int windows = argc > 1 ? atoi(argv[1]) : 1000;
	for (int n = 0; n < 20001; n++) {
		const int mode = n == 0 ? 0 : 1;
		check_mul2<TAlpha, TT4, TG2, TN4>(mode, "mul2, dbl's classes");
		check_mul2<TR, TT5, FY, TNH>(mode, "mul2, madd's classes");
		check_mulsqr<TAlpha, TT4, TG2c>(mode, "mulsqr");
	}
	// windows of 4 dbl + 1 madd of +-G from G: acc <- 16 acc + G (even windows), 16 acc - G (odd ones)
	static const uint32_t gx[8] = {0xd898c296u, 0xf4a13945u, 0x2deb33a0u, 0x77037d81u, 0x63a440f2u, 0xf8bce6e5u, 0xe12c4247u, 0x6b17d1f2u};
	static const uint32_t gy[8] = {0x37bf51f5u, 0xcbb64068u, 0x6b315eceu, 0x2bce3357u, 0x7c0f9e16u, 0x8ee7eb4au, 0xfe1a7f9bu, 0x4fe342e2u};
	const Fcanon r2 = constant<Fcanon>(K::R2), one = constant<Fcanon>(K::ONE);
	const Fcanon GX = canonical(mul(from_words(gx), r2)), GY = canonical(mul(from_words(gy), r2));
	Jac acc;
	acc.X = weaken<FX>(GX);
	acc.Y = weaken<FY>(GY);
	acc.Z = weaken<FZ>(one);
	for (int w = 0; w < windows; w++) {
		for (int d = 0; d < 4; d++) {
			acc = dbl(acc);
		}
		bool hz;
		acc = (w & 1) ? madd(acc, GX, neg_aff(GY), hz) : madd(acc, GX, weaken<FYaff>(GY), hz);
		if (hz) {
			failures++;
			fprintf(stderr, "FAIL window %d: exceptional pair\n", w);
		}
	}
	const Fmul z = weaken<Fmul>(mul(acc.Z, one));
	const Fmul zi = inv(z);
	const Fmul zi2 = weaken<Fmul>(sqr(zi));
	const Fcanon x = canonical(mul(mul(acc.X, zi2), Fcanon{{1, 0, 0, 0, 0, 0, 0, 0, 0}}));
	const Fcanon y = canonical(mul(mul(mul(fold(acc.Y), zi2), zi), Fcanon{{1, 0, 0, 0, 0, 0, 0, 0, 0}}));
	uint32_t xw[8], yw[8];
	to_words(xw, x);
	to_words(yw, y);
	printf("switches %d windows %d failures %d\nx ", t_fused_switches(), windows, failures);
	for (int i = 7; i >= 0; i--) {
		printf("%08x", xw[i]);
	}
	printf("\ny ");
	for (int i = 7; i >= 0; i--) {
		printf("%08x", yw[i]);
	}
	printf("\n");
	return failures ? 1 : 0;
}
#endif
