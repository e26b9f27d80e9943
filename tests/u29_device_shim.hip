// tests/u29_device_shim.hip -- TEST INFRASTRUCTURE: device build of secp256r1's radix-2^29 headers
// (ecamd_u29.h, ecamd_p256.h), the twin of tests/u29_host_shim.cpp.  One kernel per operation, one item
// per lane; built by tests/u29_device.py with the flags of the product (-DU29_ASM_MAD) and driven by
// tests/test_gpu_u29_unit.py.  No product logic here.
#include <hip/hip_runtime.h>
#include <cstdint>
#define U29_INLINE_MUL 1
#include "../libecc_amd/csrc/ecamd_p256.h"

using namespace p256;

template <class T> static __device__ __forceinline__ void ld(T &x, const uint32_t *src)
{
#pragma unroll
	for (int j = 0; j < 9; j++) {
		x.l[j] = src[j];
	}
}
template <class T> static __device__ __forceinline__ void st(uint32_t *dst, const T &x)
{
#pragma unroll
	for (int j = 0; j < 9; j++) {
		dst[j] = x.l[j];
	}
}
static __device__ __forceinline__ void ldj(Jac &P, const uint32_t *src)
{
	ld(P.X, src);
	ld(P.Y, src + 9);
	ld(P.Z, src + 18);
}
static __device__ __forceinline__ void stj(uint32_t *dst, const Jac &P)
{
	st(dst, P.X);
	st(dst + 9, P.Y);
	st(dst + 18, P.Z);
}

#define SHIM_ITEM() \
	const int i = blockIdx.x * 64 + threadIdx.x; \
	if (i >= n) { \
		return; \
	}

// a, b: 9 limbs each (must respect Fmul bounds); out: 9 limbs
__global__ __launch_bounds__(64) void k_mul(const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
	SHIM_ITEM();
	Fmul x, y;
	ld(x, a + (size_t)i * 9);
	ld(y, b + (size_t)i * 9);
	st(out + (size_t)i * 9, mul(x, y));
}
__global__ __launch_bounds__(64) void k_sqr(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	Fmul x;
	ld(x, a + (size_t)i * 9);
	st(out + (size_t)i * 9, sqr(x));
}
// loose operands: limbs up to 2^30.3, value up to ~6p (class used for worst-case tests)
__global__ __launch_bounds__(64) void k_mul_loose(const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
	SHIM_ITEM();
	F<(1ull << 30), (6ull << 24), 96> x, y;
	ld(x, a + (size_t)i * 9);
	ld(y, b + (size_t)i * 9);
	st(out + (size_t)i * 9, mul(x, y));
}
__global__ __launch_bounds__(64) void k_fold(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	F<0xfffffffeull, (6ull << 24), 100> x;
	ld(x, a + (size_t)i * 9);
	st(out + (size_t)i * 9, fold(x));
}
__global__ __launch_bounds__(64) void k_inv(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	Fmul x;
	ld(x, a + (size_t)i * 9);
	st(out + (size_t)i * 9, inv(x));
}
// out: 8 saturated words per item
__global__ __launch_bounds__(64) void k_canonical_words(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	Fmul x;
	ld(x, a + (size_t)i * 9);
	const Fcanon c = canonical(x);
	uint32_t w[8];
	to_words(w, c);
#pragma unroll
	for (int j = 0; j < 8; j++) {
		out[(size_t)i * 8 + j] = w[j];
	}
}
// in: 8 saturated words per item
__global__ __launch_bounds__(64) void k_from_words(const uint32_t *words, uint32_t *out, int n)
{
	SHIM_ITEM();
	uint32_t w[8];
#pragma unroll
	for (int j = 0; j < 8; j++) {
		w[j] = words[(size_t)i * 8 + j];
	}
	st(out + (size_t)i * 9, from_words(w));
}
// out: one word per item
__global__ __launch_bounds__(64) void k_is_zero(const uint32_t *a, uint32_t *out, int n)
{
	SHIM_ITEM();
	F<MASK, (4ull << 24), 64> x;
	ld(x, a + (size_t)i * 9);
	out[i] = is_zero_mulout(x) ? 1 : 0;
}
// Jacobian ops on loop-carried classes: in/out 27 limbs (X, Y, Z)
__global__ __launch_bounds__(64) void k_dbl(const uint32_t *p, uint32_t *out, int n)
{
	SHIM_ITEM();
	Jac P;
	ldj(P, p + (size_t)i * 27);
	stj(out + (size_t)i * 27, dbl(P));
}
__global__ __launch_bounds__(64) void k_add(const uint32_t *p, const uint32_t *q, uint32_t *out, uint32_t *flag, int n)
{
	SHIM_ITEM();
	Jac P;
	ldj(P, p + (size_t)i * 27);
	FX X2;
	FZ Z2;
	FYsel Y2;
	ld(X2, q + (size_t)i * 27);
	ld(Y2, q + (size_t)i * 27 + 9);
	ld(Z2, q + (size_t)i * 27 + 18);
	bool hz;
	stj(out + (size_t)i * 27, add_jac(P, X2, Y2, Z2, hz));
	flag[i] = hz ? 1 : 0;
}
// q: 18 limbs (affine x, y); negate is the same for the whole launch
__global__ __launch_bounds__(64) void k_madd(const uint32_t *p, const uint32_t *q, uint32_t *out, uint32_t *flag, int negate, int n)
{
	SHIM_ITEM();
	Jac P;
	ldj(P, p + (size_t)i * 27);
	Fcanon X2, Y2;
	ld(X2, q + (size_t)i * 18);
	ld(Y2, q + (size_t)i * 18 + 9);
	bool hz;
	const Jac R = negate ? madd(P, X2, neg_aff(Y2), hz) : madd(P, X2, weaken<FYaff>(Y2), hz);
	stj(out + (size_t)i * 27, R);
	flag[i] = hz ? 1 : 0;
}
// P, D, R2, ONE, BM (9 each), Q3 Q6 Q7 Q8 as the device code sees them
__global__ __launch_bounds__(64) void k_consts(uint32_t *out)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) {
		return;
	}
#pragma unroll
	for (int j = 0; j < 9; j++) {
		out[j] = u29::P256::P[j];
		out[9 + j] = u29::P256::D[j];
		out[18 + j] = K::R2[j];
		out[27 + j] = K::ONE[j];
		out[36 + j] = K::BM[j];
	}
	out[45] = u29::P256::Q3;
	out[46] = u29::P256::Q6;
	out[47] = u29::P256::Q7;
	out[48] = u29::P256::Q8;
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

// one operand of `win` words per item, one result of `wout` words per item
template <class KERN> static int unary(KERN kern, const uint32_t *a, uint32_t *out, int win, int wout, int n)
{
	Bufs B;
	const uint32_t *da = B.in(a, (size_t)n * win);
	uint32_t *d = B.out((size_t)n * wout);
	if (B.e == hipSuccess) {
		hipLaunchKernelGGL(kern, SHIM_GRID(n), da, d, n);
	}
	B.sync();
	B.back(out, d, (size_t)n * wout);
	return (int)B.e;
}
template <class KERN> static int binary(KERN kern, const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
	Bufs B;
	const uint32_t *da = B.in(a, (size_t)n * 9), *db = B.in(b, (size_t)n * 9);
	uint32_t *d = B.out((size_t)n * 9);
	if (B.e == hipSuccess) {
		hipLaunchKernelGGL(kern, SHIM_GRID(n), da, db, d, n);
	}
	B.sync();
	B.back(out, d, (size_t)n * 9);
	return (int)B.e;
}

extern "C" {
int gd_p256_mul(const uint32_t *a, const uint32_t *b, uint32_t *out, int n) { return binary(k_mul, a, b, out, n); }
int gd_p256_mul_loose(const uint32_t *a, const uint32_t *b, uint32_t *out, int n) { return binary(k_mul_loose, a, b, out, n); }
int gd_p256_sqr(const uint32_t *a, uint32_t *out, int n) { return unary(k_sqr, a, out, 9, 9, n); }
int gd_p256_fold(const uint32_t *a, uint32_t *out, int n) { return unary(k_fold, a, out, 9, 9, n); }
int gd_p256_inv(const uint32_t *a, uint32_t *out, int n) { return unary(k_inv, a, out, 9, 9, n); }
int gd_p256_canonical_words(const uint32_t *a, uint32_t *out, int n) { return unary(k_canonical_words, a, out, 9, 8, n); }
int gd_p256_from_words(const uint32_t *w, uint32_t *out, int n) { return unary(k_from_words, w, out, 8, 9, n); }
int gd_p256_is_zero(const uint32_t *a, uint32_t *out, int n) { return unary(k_is_zero, a, out, 9, 1, n); }
int gd_p256_dbl(const uint32_t *p, uint32_t *out, int n) { return unary(k_dbl, p, out, 27, 27, n); }
int gd_p256_add(const uint32_t *p, const uint32_t *q, uint32_t *out, uint32_t *flag, int n)
{
	Bufs B;
	const uint32_t *dp = B.in(p, (size_t)n * 27), *dq = B.in(q, (size_t)n * 27);
	uint32_t *d = B.out((size_t)n * 27), *df = B.out(n);
	if (B.e == hipSuccess) {
		hipLaunchKernelGGL(k_add, SHIM_GRID(n), dp, dq, d, df, n);
	}
	B.sync();
	B.back(out, d, (size_t)n * 27);
	B.back(flag, df, n);
	return (int)B.e;
}
int gd_p256_madd(const uint32_t *p, const uint32_t *q, uint32_t *out, uint32_t *flag, int negate, int n)
{
	Bufs B;
	const uint32_t *dp = B.in(p, (size_t)n * 27), *dq = B.in(q, (size_t)n * 18);
	uint32_t *d = B.out((size_t)n * 27), *df = B.out(n);
	if (B.e == hipSuccess) {
		hipLaunchKernelGGL(k_madd, SHIM_GRID(n), dp, dq, d, df, negate, n);
	}
	B.sync();
	B.back(out, d, (size_t)n * 27);
	B.back(flag, df, n);
	return (int)B.e;
}
int gd_p256_consts(uint32_t *out)
{
	Bufs B;
	uint32_t *d = B.out(49);
	if (B.e == hipSuccess) {
		hipLaunchKernelGGL(k_consts, dim3(1), dim3(64), 0, 0, d);
	}
	B.sync();
	B.back(out, d, 49);
	return (int)B.e;
}
// what this object was built as: bit 0 = U29_ASM_MAD (the asm MAD branches of the headers), bits 8.. = 8 (secp256r1's own unit)
int gd_flags(void)
{
	int f = 8 << 8;
#if defined(U29_ASM_MAD)
	f |= 1;
#endif
	return f;
}
}
