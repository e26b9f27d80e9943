// tests/u29g_device_shim.hip -- TEST INFRASTRUCTURE: device build of the generic radix-2^29 headers
// (ecamd_u29g.h, ecamd_jacg.h, ecamd_rcbg.h), the twin of tests/u29g_host_shim.cpp.  One kernel per
// operation and field size, one item per lane: operands come from global arrays, the header function
// runs, the result limbs go back.  Built by tests/u29_device.py with the flags of the product
// (-DU29_ASM_MAD: the v_mad_u64_u32 / v_mad_i64_i32 statements the host build never compiles) and driven
// by tests/test_gpu_u29g_units.py.  The curve image sits in __constant__ memory as in
// ecamd_g29_kernel.hip, so that it is wave-uniform (the "s" operands of the MADs assume that).
// No product logic here.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../libecc_amd/csrc/ecamd_jacg.h"
#if defined(G29_P25519) || defined(G29_P448)
#include "../libecc_amd/csrc/ecamd_rcbg.h"   /* the two units whose EdDSA tail uses it */
#define SHIM_RCB 1
#endif

using namespace jacg;

template <int PB> struct KG;   // the unit's curve image in __constant__ memory

template <class T> static __device__ __forceinline__ void ld(T &x, const uint32_t *src)
{
#pragma unroll
	for (int j = 0; j < T::C::NL; j++) {
		x.l[j] = src[j];
	}
}
template <class T> static __device__ __forceinline__ void st(uint32_t *dst, const T &x)
{
#pragma unroll
	for (int j = 0; j < T::C::NL; j++) {
		dst[j] = x.l[j];
	}
}
template <class P> static __device__ __forceinline__ void ld3(P &pt, const uint32_t *src)
{
	constexpr int NL = decltype(pt.X)::C::NL;
	ld(pt.X, src);
	ld(pt.Y, src + NL);
	ld(pt.Z, src + 2 * NL);
}
template <class P> static __device__ __forceinline__ void st3(uint32_t *dst, const P &pt)
{
	constexpr int NL = decltype(pt.X)::C::NL;
	st(dst, pt.X);
	st(dst + NL, pt.Y);
	st(dst + 2 * NL, pt.Z);
}

#define SHIM_ITEM() \
	const int i = blockIdx.x * 64 + threadIdx.x; \
	if (i >= n) { \
		return; \
	} \
	constexpr int NL = Cfg<PB>::NL; \
	const CurveG<NL> &K = KG<PB>::get(); \
	(void)K

template <int PB> __global__ __launch_bounds__(64) void k_mul(const uint32_t *a, const uint32_t *b, uint32_t *out, int sq, int n)
{
	SHIM_ITEM();
	typename Cls<PB>::FA x, y;
	ld(x, a + (size_t)i * NL);
	ld(y, b + (size_t)i * NL);
	if (sq) {
		st(out + (size_t)i * NL, sqr(x, K));
	} else {
		st(out + (size_t)i * NL, mul(x, y, K));
	}
}
#if defined(G29_P25519) || defined(G29_P448)
template <int PB> __global__ __launch_bounds__(64) void k_mulword(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	// the loosest operand class the ladders hand over: a carried difference
	E<PB, (1ull << 32) - 1, g29::P448 ? ((1ull << 29) - 1) : ((1ull << 32) - 1), 16> x;
	ld(x, a + (size_t)i * NL);
	st(out + (size_t)i * NL, mul_word<g29::P448 ? 39081u : 121665u>(x));
}
#endif
template <int PB> __global__ __launch_bounds__(64) void k_dbl(const uint32_t *p, uint32_t *out, int n)
{
	SHIM_ITEM();
	Jac<PB> P;
	ld3(P, p + (size_t)i * 3 * NL);
	st3(out + (size_t)i * 3 * NL, dbl(P, K));
}
template <int PB> __global__ __launch_bounds__(64) void k_add(const uint32_t *p, const uint32_t *q, uint32_t *out, uint32_t *flag, int n)
{
	SHIM_ITEM();
	Jac<PB> P;
	typename Cls<PB>::FA X2, Y2, Z2;
	ld3(P, p + (size_t)i * 3 * NL);
	ld(X2, q + (size_t)i * 3 * NL);
	ld(Y2, q + (size_t)i * 3 * NL + NL);
	ld(Z2, q + (size_t)i * 3 * NL + 2 * NL);
	bool hz;
	st3(out + (size_t)i * 3 * NL, add_jac(P, X2, Y2, Z2, hz, K));
	flag[i] = hz ? 1 : 0;
}
#if !defined(G29_K256)
// mixed addition / doubling on the tight accumulator class JacT (the window loop of the affine-table kernels)
template <int PB> __global__ __launch_bounds__(64) void k_madd(const uint32_t *p, const uint32_t *q, uint32_t *out, int n)
{
	SHIM_ITEM();
	JacT<PB> P;
	typename Cls<PB>::FA X2, Y2;
	ld3(P, p + (size_t)i * 3 * NL);
	ld(X2, q + (size_t)i * 2 * NL);
	ld(Y2, q + (size_t)i * 2 * NL + NL);
	st3(out + (size_t)i * 3 * NL, madd_jac(P, X2, Y2, K));
}
template <int PB> __global__ __launch_bounds__(64) void k_dblt(const uint32_t *p, uint32_t *out, int n)
{
	SHIM_ITEM();
	JacT<PB> P;
	ld3(P, p + (size_t)i * 3 * NL);
	st3(out + (size_t)i * 3 * NL, dbl(P, K));
}
#endif
template <int PB> __global__ __launch_bounds__(64) void k_neg(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	typename Cls<PB>::FM x;
	ld(x, a + (size_t)i * NL);
	st(out + (size_t)i * NL, neg<PB>(x, K));
}
template <int PB> __global__ __launch_bounds__(64) void k_inv(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	typename Cls<PB>::FM x;
	ld(x, a + (size_t)i * NL);
	st(out + (size_t)i * NL, inv<PB>(x, K));
}
template <int PB> __global__ __launch_bounds__(64) void k_canon(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	typename Cls<PB>::FM x;
	ld(x, a + (size_t)i * NL);
	uint32_t d[NL];
	canonical_digits(d, x, K);
#pragma unroll
	for (int j = 0; j < NL; j++) {
		out[(size_t)i * NL + j] = d[j];
	}
}
#ifdef SHIM_RCB
// complete (RCB) addition / doubling of ecamd_rcbg.h: p, q, out = X || Y || Z (FA class); dbl: q ignored.  flag: Y == 0 | (Z == 0) << 1
template <int PB> __global__ __launch_bounds__(64) void k_rcb(const uint32_t *p, const uint32_t *q, uint32_t *out, uint32_t *flag, int dbl, int n)
{
	SHIM_ITEM();
	rcbg::PtG<PB> P, Q;
	ld3(P, p + (size_t)i * 3 * NL);
	ld3(Q, q + (size_t)i * 3 * NL);
	const rcbg::PtG<PB> R = dbl ? rcbg::dbl_rcb<PB>(P, K) : rcbg::add_rcb<PB>(P, Q, K);
	st3(out + (size_t)i * 3 * NL, R);
	flag[i] = (rcbg::coord_is_zero<PB>(R.Y, K) ? 1 : 0) | (rcbg::coord_is_zero<PB>(R.Z, K) ? 2 : 0);
}
#endif
// lift_x_even: xw = the abscissa as NW saturated little-endian words; out = xo || yo (multiplication-result class); flag = ok
template <int PB> __global__ __launch_bounds__(64) void k_liftx(const uint32_t *xw, uint32_t *out, uint32_t *flag, int n)
{
	SHIM_ITEM();
	constexpr int NW = (PB + 31) / 32;
	uint32_t w[NW];
#pragma unroll
	for (int j = 0; j < NW; j++) {
		w[j] = xw[(size_t)i * NW + j];
	}
	const auto xd = from_words<PB, NW>(w);
	typename Cls<PB>::FM xo, yo;
	const bool ok = lift_x_even<PB>(xd, K, xo, yo);
	st(out + (size_t)i * 2 * NL, xo);
	st(out + (size_t)i * 2 * NL + NL, yo);
	flag[i] = ok ? 1 : 0;
}

// ---- host side: allocation, copies, one launch, one synchronize; the first hipError_t comes back as an int ----
struct Bufs {
	void *p[6];
	int np = 0;
	hipError_t e = hipSuccess;
	uint32_t *in(const uint32_t *h, size_t words)
	{
		uint32_t *d = out(words);
		if (e == hipSuccess) {
			e = hipMemcpy(d, h, 4 * words, hipMemcpyHostToDevice);
		}
		return d;
	}
	uint32_t *out(size_t words)
	{
		void *d = nullptr;
		if (e == hipSuccess) {
			e = hipMalloc(&d, 4 * words);
			if (e == hipSuccess) {
				p[np++] = d;
				e = hipMemset(d, 0, 4 * words);
			}
		}
		return (uint32_t *)d;
	}
	void sync()
	{
		if (e == hipSuccess) {
			e = hipGetLastError();
		}
		if (e == hipSuccess) {
			e = hipDeviceSynchronize();
		}
	}
	void back(uint32_t *h, const uint32_t *d, size_t words)
	{
		if (e == hipSuccess) {
			e = hipMemcpy(h, d, 4 * words, hipMemcpyDeviceToHost);
		}
	}
	~Bufs()
	{
		for (int j = 0; j < np; j++) {
			(void)hipFree(p[j]);
		}
	}
};
#define SHIM_GRID(n) dim3(((n) + 63) / 64), dim3(64), 0, 0

template <int PB> struct Dev {
	typedef Cfg<PB> C;
	static constexpr int NL = C::NL;
	static constexpr int NW = (PB + 31) / 32;
	typedef CurveG<NL> CK;
	static void curve(Bufs &B, const uint32_t *k)
	{
		if (B.e == hipSuccess) {
			B.e = KG<PB>::put(k);
		}
	}
	static int mul_(const uint32_t *k, const uint32_t *a, const uint32_t *b, uint32_t *out, int sq, int n)
	{
		Bufs B;
		curve(B, k);
		const uint32_t *da = B.in(a, (size_t)n * NL), *db = B.in(b, (size_t)n * NL);
		uint32_t *d = B.out((size_t)n * NL);
		if (B.e == hipSuccess) {
			hipLaunchKernelGGL(k_mul<PB>, SHIM_GRID(n), da, db, d, sq, n);
		}
		B.sync();
		B.back(out, d, (size_t)n * NL);
		return (int)B.e;
	}
	static int mulword_(const uint32_t *a, uint32_t *out, int n)
	{
#if defined(G29_P25519) || defined(G29_P448)
		Bufs B;
		const uint32_t *da = B.in(a, (size_t)n * NL);
		uint32_t *d = B.out((size_t)n * NL);
		if (B.e == hipSuccess) {
			hipLaunchKernelGGL(k_mulword<PB>, SHIM_GRID(n), da, d, n);
		}
		B.sync();
		B.back(out, d, (size_t)n * NL);
		return (int)B.e;
#else
		(void)a;
		(void)out;
		(void)n;
		return -1;
#endif
	}
	// one operand of `win` words per item, one result of `wout` words per item
	template <class KERN> static int unary(KERN kern, const uint32_t *k, const uint32_t *a, uint32_t *out, int win, int wout, int n)
	{
		Bufs B;
		curve(B, k);
		const uint32_t *da = B.in(a, (size_t)n * win);
		uint32_t *d = B.out((size_t)n * wout);
		if (B.e == hipSuccess) {
			hipLaunchKernelGGL(kern, SHIM_GRID(n), da, d, n);
		}
		B.sync();
		B.back(out, d, (size_t)n * wout);
		return (int)B.e;
	}
	static int dbl_(const uint32_t *k, const uint32_t *p, uint32_t *out, int n) { return unary(k_dbl<PB>, k, p, out, 3 * NL, 3 * NL, n); }
	static int neg_(const uint32_t *k, const uint32_t *a, uint32_t *out, int n) { return unary(k_neg<PB>, k, a, out, NL, NL, n); }
	static int inv_(const uint32_t *k, const uint32_t *a, uint32_t *out, int n) { return unary(k_inv<PB>, k, a, out, NL, NL, n); }
	static int canon_(const uint32_t *k, const uint32_t *a, uint32_t *out, int n) { return unary(k_canon<PB>, k, a, out, NL, NL, n); }
	static int add_(const uint32_t *k, const uint32_t *p, const uint32_t *q, uint32_t *out, uint32_t *flag, int n)
	{
		Bufs B;
		curve(B, k);
		const uint32_t *dp = B.in(p, (size_t)n * 3 * NL), *dq = B.in(q, (size_t)n * 3 * NL);
		uint32_t *d = B.out((size_t)n * 3 * NL), *df = B.out(n);
		if (B.e == hipSuccess) {
			hipLaunchKernelGGL(k_add<PB>, SHIM_GRID(n), dp, dq, d, df, n);
		}
		B.sync();
		B.back(out, d, (size_t)n * 3 * NL);
		B.back(flag, df, n);
		return (int)B.e;
	}
#if !defined(G29_K256)
	static int madd_(const uint32_t *k, const uint32_t *p, const uint32_t *q, uint32_t *out, int n)
	{
		Bufs B;
		curve(B, k);
		const uint32_t *dp = B.in(p, (size_t)n * 3 * NL), *dq = B.in(q, (size_t)n * 2 * NL);
		uint32_t *d = B.out((size_t)n * 3 * NL);
		if (B.e == hipSuccess) {
			hipLaunchKernelGGL(k_madd<PB>, SHIM_GRID(n), dp, dq, d, n);
		}
		B.sync();
		B.back(out, d, (size_t)n * 3 * NL);
		return (int)B.e;
	}
	static int dblt_(const uint32_t *k, const uint32_t *p, uint32_t *out, int n) { return unary(k_dblt<PB>, k, p, out, 3 * NL, 3 * NL, n); }
	static void infot_(uint32_t *out)
	{
		out[0] = (uint32_t)ClsT<PB>::VT;
		out[1] = (uint32_t)ClsT<PB>::FT::LB;
		out[2] = (uint32_t)ClsT<PB>::FT::TB;
	}
#else
	// secp256k1's flavour keeps the Jacobian-table kernel: no JacT there
	static int madd_(const uint32_t *, const uint32_t *, const uint32_t *, uint32_t *, int) { return -1; }
	static int dblt_(const uint32_t *, const uint32_t *, uint32_t *, int) { return -1; }
	static void infot_(uint32_t *out) { out[0] = 0; }
#endif
	static int rcb_(const uint32_t *k, const uint32_t *p, const uint32_t *q, uint32_t *out, uint32_t *flag, int dbl, int n)
	{
#ifdef SHIM_RCB
		Bufs B;
		curve(B, k);
		const uint32_t *dp = B.in(p, (size_t)n * 3 * NL), *dq = B.in(q, (size_t)n * 3 * NL);
		uint32_t *d = B.out((size_t)n * 3 * NL), *df = B.out(n);
		if (B.e == hipSuccess) {
			hipLaunchKernelGGL(k_rcb<PB>, SHIM_GRID(n), dp, dq, d, df, dbl, n);
		}
		B.sync();
		B.back(out, d, (size_t)n * 3 * NL);
		B.back(flag, df, n);
		return (int)B.e;
#else
		(void)k, (void)p, (void)q, (void)out, (void)flag, (void)dbl, (void)n;
		return -1;
#endif
	}
	static int liftx_(const uint32_t *k, const uint32_t *xw, uint32_t *out, uint32_t *flag, int n)
	{
		Bufs B;
		curve(B, k);
		const uint32_t *dx = B.in(xw, (size_t)n * NW);
		uint32_t *d = B.out((size_t)n * 2 * NL), *df = B.out(n);
		if (B.e == hipSuccess) {
			hipLaunchKernelGGL(k_liftx<PB>, SHIM_GRID(n), dx, d, df, n);
		}
		B.sync();
		B.back(out, d, (size_t)n * 2 * NL);
		B.back(flag, df, n);
		return (int)B.e;
	}
	static void info_(uint32_t *out)
	{
		out[0] = NL;
		out[1] = (uint32_t)C::HEAD;
		out[2] = (uint32_t)(int32_t)C::TOPSH;
		out[3] = (uint32_t)Cls<PB>::LC;
		out[4] = (uint32_t)(Cls<PB>::VA & 0xffffffffu);
		out[5] = (uint32_t)sizeof(CK);
		out[6] = (uint32_t)Cls<PB>::FA::LB;
		out[7] = (uint32_t)Cls<PB>::FA::TB;
	}
};

#define SHIM(PB) \
	__constant__ CurveG<Cfg<PB>::NL> g_shim_k_##PB; \
	template <> struct KG<PB> { \
		static __device__ __forceinline__ const CurveG<Cfg<PB>::NL> &get() { return g_shim_k_##PB; } \
		static hipError_t put(const uint32_t *k) \
		{ \
			return hipMemcpyToSymbol(HIP_SYMBOL(g_shim_k_##PB), k, sizeof(CurveG<Cfg<PB>::NL>), 0, hipMemcpyHostToDevice); \
		} \
	}; \
	extern "C" { \
	int gd_mul_##PB(const uint32_t *k, const uint32_t *a, const uint32_t *b, uint32_t *o, int sq, int n) { return Dev<PB>::mul_(k, a, b, o, sq, n); } \
	int gd_dbl_##PB(const uint32_t *k, const uint32_t *p, uint32_t *o, int n) { return Dev<PB>::dbl_(k, p, o, n); } \
	int gd_mulword_##PB(const uint32_t *a, uint32_t *o, int n) { return Dev<PB>::mulword_(a, o, n); } \
	int gd_add_##PB(const uint32_t *k, const uint32_t *p, const uint32_t *q, uint32_t *o, uint32_t *f, int n) { return Dev<PB>::add_(k, p, q, o, f, n); } \
	int gd_madd_##PB(const uint32_t *k, const uint32_t *p, const uint32_t *q, uint32_t *o, int n) { return Dev<PB>::madd_(k, p, q, o, n); } \
	int gd_dblt_##PB(const uint32_t *k, const uint32_t *p, uint32_t *o, int n) { return Dev<PB>::dblt_(k, p, o, n); } \
	void gd_infot_##PB(uint32_t *o) { Dev<PB>::infot_(o); } \
	int gd_neg_##PB(const uint32_t *k, const uint32_t *a, uint32_t *o, int n) { return Dev<PB>::neg_(k, a, o, n); } \
	int gd_inv_##PB(const uint32_t *k, const uint32_t *a, uint32_t *o, int n) { return Dev<PB>::inv_(k, a, o, n); } \
	int gd_canon_##PB(const uint32_t *k, const uint32_t *a, uint32_t *o, int n) { return Dev<PB>::canon_(k, a, o, n); } \
	void gd_info_##PB(uint32_t *o) { Dev<PB>::info_(o); } \
	int gd_liftx_##PB(const uint32_t *k, const uint32_t *xw, uint32_t *o, uint32_t *f, int n) { return Dev<PB>::liftx_(k, xw, o, f, n); } \
	int gd_rcb_##PB(const uint32_t *k, const uint32_t *p, const uint32_t *q, uint32_t *o, uint32_t *f, int dbl, int n) \
	{ \
		return Dev<PB>::rcb_(k, p, q, o, f, dbl, n); \
	} \
	}

// what this object was built as: bit 0 = U29_ASM_MAD (the asm MAD branches of the headers), bits 8.. = the flavour
// (0 dense, 1 G29_M521P, 2 G29_P25519, 3 G29_P384S, 4 G29_K256, 5 G29_P448, 6 G29_P224S, 7 G29_P192S)
extern "C" int gd_flags(void)
{
	int f = 0;
#if defined(U29_ASM_MAD)
	f |= 1;
#endif
#if defined(G29_M521P)
	f |= 1 << 8;
#elif defined(G29_P25519)
	f |= 2 << 8;
#elif defined(G29_P384S)
	f |= 3 << 8;
#elif defined(G29_K256)
	f |= 4 << 8;
#elif defined(G29_P448)
	f |= 5 << 8;
#elif defined(G29_P224S)
	f |= 6 << 8;
#elif defined(G29_P192S)
	f |= 7 << 8;
#endif
	return f;
}

// a flavour flag compiles only its own size (the other sizes do not compile under it)
#if defined(SHIM_ONLY_255)
SHIM(255)
#elif defined(SHIM_ONLY_384)
SHIM(384)
#elif defined(SHIM_ONLY_256)
SHIM(256)
#elif defined(SHIM_ONLY_448)
SHIM(448)
#elif defined(SHIM_ONLY_224)
SHIM(224)
#elif defined(SHIM_ONLY_192)
SHIM(192)
#elif defined(SHIM_ONLY_521)
SHIM(521)
#else
SHIM(192)
SHIM(224)
SHIM(255)
SHIM(256)
SHIM(320)
SHIM(384)
SHIM(448)
SHIM(511)
SHIM(512)
SHIM(521)
#endif
