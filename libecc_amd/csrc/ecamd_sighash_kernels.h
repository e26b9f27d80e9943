// libecc_amd/csrc/ecamd_sighash_kernels.h -- the kernels of batched ECSDSA, ECOSDSA and ECKCDSA around their multiplications and
// k_sha2_slots (included at the end of ecamd_kernels.hip, behind ecamd_recover_kernels.h and ecamd_sigfam_kernels.h: SigfamOps,
// modulus q in a constant slot).
//
//   k_hsig_prep   verification front end: s in [1, q - 1], e from r (Horner over element-sized chunks for ECSDSA / ECOSDSA, the
//                 truncation, XOR and reduction for ECKCDSA), the multipliers of G and Y, the flag byte.  No inversion.
//   (W' = [u]G + [v]Y as affine bytes: the two multiplications, then k_recover_fin / k_recover_redo of the recovery path, whose
//    first sum is W')
//   k_hsig_fill   the commitment's coordinates into the blank of the staged message slot (ECSDSA: x || y, ECOSDSA: x), or the
//                 slot of FE2OS(x) itself (ECKCDSA); a slot whose length does not hold the blank or does not fit the stride flags
//                 its item
//   (k_sha2_slots)
//   k_hsig_cmp    verification: the digest against r, byte for byte, with the flags and the status of W'
//   k_hsig_sign   signing: e from the digest, s, the failure rules, the signature bytes
#pragma once
#include "ecamd_sighash.h"

// One item per lane: the front end has no inversion to share.
template <int NW> __global__ __launch_bounds__(64) void k_hsig_prep(EcamdHsigArgs A)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int qlen = (int)A.qlen, hsize = (int)A.hsize;
	const SigfamOps<NW> ops{A.qslot};
	const int rl = echsig::r_len(A.alg, hsize, qlen);
	const u8 *h = A.alg == echsig::ALG_ECKCDSA ? A.inputs + (size_t)i * hsize : nullptr;
	Fe<NW> u, v;
	const bool ok = echsig::verify_uv(ops, A.alg, A.sigs + (size_t)i * (rl + qlen), hsize, qlen, h, u, v);
	fe_store_be<NW>(A.u + (size_t)i * qlen, qlen, ok ? u : fe_zero<NW>());
	fe_store_be<NW>(A.v + (size_t)i * qlen, qlen, ok ? v : fe_zero<NW>());
	A.flags[i] = ok ? 0 : 1;
}

// One byte per thread.  ECSDSA / ECOSDSA: byte b of item i's blank (A.slots holds a copy of the caller's slots); ECKCDSA: byte b
// of item i's whole slot, the length word included.  An item without a commitment (flagged, or W not a finite point) gets
// zeros: its digest decides nothing.  Thread 0 of an item settles its flag: signing has no front end that wrote one.
// (The byte-threads of an item read A.flags[i] while its thread 0 may write it.  The write never changes what a reader computes:
// it happens in a signing call, where `prior` is forced false and the flag is not read, or for an unusable slot, where `have` is
// already false through `usable` whatever `prior` says.)
__global__ __launch_bounds__(256) void k_hsig_fill(EcamdHsigArgs A)
{
	const bool kcdsa = A.alg == echsig::ALG_ECKCDSA;
	const u32 clen = A.clen;
	const u32 per = kcdsa ? 4u + clen : (u32)echsig::blank_len(A.alg, (int)clen);
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= (size_t)A.n * per) {
		return;
	}
	const u32 i = (u32)(t / per), b = (u32)(t % per);
	u8 *slot = A.slots + (size_t)i * A.sstride;
	bool usable = true;
	if (!kcdsa) {
		usable = echsig::slot_ok(A.alg, *(const u32 *)slot, A.sstride, (int)clen);
	}
	const bool prior = A.sign ? false : A.flags[i] != 0;
	const bool have = usable & !prior & (A.stW[i] == 0);
	const u8 *W = A.W + (size_t)i * 2 * clen;
	if (kcdsa) {
		slot[b] = b < 4 ? (u8)(b == 0 ? clen : 0u) : (have ? W[b - 4] : (u8)0);   // clen <= 66: one length byte
	} else {
		slot[4 + b] = have ? W[b] : (u8)0;
	}
	if (b == 0 && (A.sign || !usable)) {
		A.flags[i] = usable ? 0 : 1;
	}
}

__global__ __launch_bounds__(256) void k_hsig_cmp(EcamdHsigArgs A)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int qlen = (int)A.qlen, hsize = (int)A.hsize;
	const int rl = echsig::r_len(A.alg, hsize, qlen);
	const bool live = (A.flags[i] == 0) & (A.stW[i] == 0);
	const bool same = echsig::digest_matches(A.dg + (size_t)i * hsize, hsize, A.sigs + (size_t)i * (rl + qlen), rl);
	A.out[i] = (live & same) ? 0 : 1;
}

// One item per lane.  status 1: what sign_key_ok refuses, k not in [1, q - 1], [k]G not a finite point, an unusable slot, or
// one of the reference's failure / restart conditions (echsig::sign_s).
template <int NW> __global__ __launch_bounds__(64) void k_hsig_sign(EcamdHsigArgs A)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int qs = A.qslot;
	const int qlen = (int)A.qlen, hsize = (int)A.hsize;
	const SigfamOps<NW> ops{qs};
	const int rl = echsig::r_len(A.alg, hsize, qlen);
	const Fe<NW> x = fe_load_be<NW>(A.privs + (size_t)i * qlen, qlen);
	const Fe<NW> kk = fe_load_be<NW>(A.nonces + (size_t)i * qlen, qlen);
	bool ok = echsig::sign_key_ok(ops, A.alg, x) & !fe_is_zero<NW>(kk) & fe_lt_p<NW>(kk, qs) & (A.stW[i] == 0) & (A.flags[i] == 0);
	const u8 *dg = A.dg + (size_t)i * hsize;
	const u8 *h = A.alg == echsig::ALG_ECKCDSA ? A.inputs + (size_t)i * hsize : nullptr;
	Fe<NW> sv = fe_zero<NW>();
	if (ok) {
		ok = echsig::sign_s(ops, A.alg, x, kk, dg, hsize, qlen, h, sv);
	}
	u8 *sig = A.out + (size_t)i * (rl + qlen);
	for (int b = 0; b < rl; b++) {
		sig[b] = ok ? dg[hsize - rl + b] : (u8)0;
	}
	fe_store_be<NW>(sig + rl, qlen, ok ? sv : fe_zero<NW>());
	A.status[i] = ok ? 0 : 1;
}

static bool hsig_args_sane(const EcamdHsigArgs &a)
{
	return echsig::alg_known(a.alg) && a.hsize >= 20 && a.hsize <= 64 && a.clen >= 1 && a.clen <= 72;   // 20: RIPEMD-160
}

hipError_t ecamd_launch_hsig_prep(int nw, const EcamdHsigArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!hsig_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_hsig_prep<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t ecamd_launch_hsig_fill(const EcamdHsigArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	const bool kcdsa = a.alg == echsig::ALG_ECKCDSA;
	const uint32_t per = kcdsa ? 4u + a.clen : (uint32_t)echsig::blank_len(a.alg, (int)a.clen);
	// every byte written lies inside the staged slot (ECKCDSA's `per` counts the length word, the blank's does not)
	if (!hsig_args_sane(a) || (a.sstride & 3u) || a.sstride < (kcdsa ? per : 4u + per)) {
		return hipErrorInvalidValue;
	}
	const size_t bytes = (size_t)a.n * per;
	hipLaunchKernelGGL(k_hsig_fill, dim3((unsigned)((bytes + 255) / 256)), dim3(256), 0, s, a);
	return hipGetLastError();
}

hipError_t ecamd_launch_hsig_cmp(const EcamdHsigArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!hsig_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_hsig_cmp, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
	return hipGetLastError();
}

hipError_t ecamd_launch_hsig_sign(int nw, const EcamdHsigArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!hsig_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_hsig_sign<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
