// libecc_amd/csrc/ecamd_bign_kernels.h -- the kernels of batched BIGN / DBIGN around their multiplications and k_belt_slots
// (included at the end of ecamd_kernels.hip, behind ecamd_sigfam_kernels.h: SigfamOps, modulus q in a constant slot).
//
//   k_bign_prep   verification front end: s1 < q, hbar from the whole digest (Horner over element-sized chunks), the multipliers
//                 u = s1 + hbar of G and v = s0 + 2^(8l) of Y as big-endian bytes, the flag byte.  No inversion.
//   (W' = [u]G + [v]Y as affine bytes: the two multiplications, then k_recover_fin / k_recover_redo, whose first sum is W')
//   k_bign_fill   belt-hash's slot OID || first 2l bytes of LE(W.x) || LE(W.y) || digest, built in a staging buffer
//   (k_belt_slots)
//   k_bign_cmp    verification: W' finite, the first min(l, 32) bytes of the BelT digest equal to s0, the rest of s0 zero
//   k_bign_sign   signing: s1 from k, x, hbar and s0; the status byte; the signature bytes (zeros where the reference fails)
// A digest the device computed itself comes from a message slot; a slot whose length does not fit the stride rejects its item
// (k_bign_prep flags it, k_bign_sign fails it).
#pragma once
#include "ecamd_bign.h"

template <int NW> static __device__ __forceinline__ void fe_store_le_bytes(u8 *dst, int len, const Fe<NW> &a)
{
#pragma unroll
	for (int j = 0; j < NW; j++) {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if (4 * j + k < len) {
				dst[4 * j + k] = (u8)(a.v[j] >> (8 * k));
			}
		}
	}
}

static __device__ __forceinline__ bool bign_slot_usable(const EcamdBignArgs &A, u32 i)
{
	return A.mslots == nullptr || ecbign::slot_ok(*(const u32 *)(A.mslots + (size_t)i * A.mstride), A.mstride);
}

// One item per lane: the front end has no inversion to share.
template <int NW> __global__ __launch_bounds__(64) void k_bign_prep(EcamdBignArgs A)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int qlen = (int)A.qlen;
	const SigfamOps<NW> ops{A.qslot};
	Fe<NW> u, v;
	bool ok = ecbign::verify_uv(ops, A.sigs + (size_t)i * ecbign::sig_len(qlen), qlen, A.dg + (size_t)i * A.hsize, (int)A.hsize, u, v);
	ok &= bign_slot_usable(A, i);
	fe_store_be<NW>(A.u + (size_t)i * qlen, qlen, ok ? u : fe_zero<NW>());
	fe_store_be<NW>(A.v + (size_t)i * qlen, qlen, ok ? v : fe_zero<NW>());
	A.flags[i] = ok ? 0 : 1;
}

// One byte per thread: byte b of item i's BelT slot, the length word included.  An item without a commitment (flagged, or W not
// a finite point) gets zeros in the place of the coordinates: its digest decides nothing.
__global__ __launch_bounds__(256) void k_bign_fill(EcamdBignArgs A)
{
	const u32 ilen = ecbign::belt_input_len(A.oid_len, (int)A.qlen, A.hsize), per = 4u + ilen;
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= (size_t)A.n * per) {
		return;
	}
	const u32 i = (u32)(t / per), b = (u32)(t % per);
	const bool prior = A.sign ? false : A.flags[i] != 0;
	const bool have = !prior & (A.stW[i] == 0);
	u8 val;
	if (b < 4) {
		val = (u8)(ilen >> (8 * b));
	} else {
		const u32 c = b - 4u;
		const bool coord = c >= A.oid_len && c < A.oid_len + 2u * (u32)ecbign::s0_len((int)A.qlen);
		if (c < A.oid_len) {
			// the OID lies in the kernel's argument block: picked by constant indices, so that the block is not copied to scratch
			u8 o = 0;
#pragma unroll
			for (u32 j = 0; j < (u32)ecbign::MAX_OID; j++) {
				o = (j == c) ? A.oid[j] : o;
			}
			val = o;
		} else {
			val = ecbign::belt_input_byte(c, nullptr, A.oid_len, A.W + (size_t)i * 2 * A.clen, A.clen, (int)A.qlen, A.dg + (size_t)i * A.hsize);
			val = (coord & !have) ? (u8)0 : val;
		}
	}
	A.slots[(size_t)i * A.bstride + b] = val;
}

__global__ __launch_bounds__(256) void k_bign_cmp(EcamdBignArgs A)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int qlen = (int)A.qlen;
	const bool live = (A.flags[i] == 0) & (A.stW[i] == 0);
	const bool same = ecbign::t_matches(A.bt + (size_t)i * ecbign::DIGEST_BT, A.sigs + (size_t)i * ecbign::sig_len(qlen), qlen);
	A.out[i] = (live & same) ? 0 : 1;
}

// One item per lane.  status 1: x >= q, k not in [1, q - 1], [k]G not a finite point, or an unusable message slot.  The value is
// computed for every lane and selected at the end: no branch on x or k.
template <int NW> __global__ __launch_bounds__(64) void k_bign_sign(EcamdBignArgs A)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int qs = A.qslot;
	const int qlen = (int)A.qlen, l = ecbign::s0_len(qlen), tl = ecbign::t_len(qlen);
	const SigfamOps<NW> ops{qs};
	const Fe<NW> x = fe_load_be<NW>(A.privs + (size_t)i * qlen, qlen);
	const Fe<NW> kk = fe_load_be<NW>(A.nonces + (size_t)i * qlen, qlen);
	const bool ok = ecbign::sign_key_ok(ops, x) & !fe_is_zero<NW>(kk) & fe_lt_p<NW>(kk, qs) & (A.stW[i] == 0) & bign_slot_usable(A, i);
	const u8 *bt = A.bt + (size_t)i * ecbign::DIGEST_BT;
	const Fe<NW> s1 = ecbign::sign_s1(ops, x, kk, bt, qlen, A.dg + (size_t)i * A.hsize, (int)A.hsize);
	u8 *sig = A.out + (size_t)i * ecbign::sig_len(qlen);
	for (int b = 0; b < l; b++) {
		sig[b] = (ok & (b < tl)) ? bt[b < tl ? b : 0] : (u8)0;
	}
	fe_store_le_bytes<NW>(sig + l, qlen, ok ? s1 : fe_zero<NW>());
	A.status[i] = ok ? 0 : 1;
}

// every byte the kernels touch lies inside the arrays the host sized from the same numbers
static bool bign_args_sane(const EcamdBignArgs &a)
{
	return a.hsize >= 1 && a.hsize <= (uint32_t)ecbign::MAX_DIGEST && a.oid_len <= (uint32_t)ecbign::MAX_OID && a.clen >= 1 && a.clen <= 72 &&
	       a.qlen >= 4 && a.qlen <= 68 && (a.mslots == nullptr || (a.mstride >= 4 && (a.mstride & 3u) == 0));
}

hipError_t ecamd_launch_bign_prep(int nw, const EcamdBignArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!bign_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_bign_prep<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t ecamd_launch_bign_fill(const EcamdBignArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	const uint32_t per = 4u + ecbign::belt_input_len(a.oid_len, (int)a.qlen, a.hsize);
	if (!bign_args_sane(a) || (a.bstride & 3u) || a.bstride < per) {
		return hipErrorInvalidValue;
	}
	const size_t bytes = (size_t)a.n * per;
	hipLaunchKernelGGL(k_bign_fill, dim3((unsigned)((bytes + 255) / 256)), dim3(256), 0, s, a);
	return hipGetLastError();
}

hipError_t ecamd_launch_bign_cmp(const EcamdBignArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!bign_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_bign_cmp, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
	return hipGetLastError();
}

hipError_t ecamd_launch_bign_sign(int nw, const EcamdBignArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!bign_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_bign_sign<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
