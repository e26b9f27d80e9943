// libecc_amd/csrc/ecamd_schnorr_kernels.h -- the kernels of BIP0340 and ECFSDSA item by item around their multiplications,
// k_sha2_slots, k_schnorr_ne and k_recover_fin / k_recover_redo (included at the end of ecamd_kernels.hip, behind
// ecamd_sighash_kernels.h: SigfamOps, modulus q in a constant slot).
//
//   k_schnorr_item_prep   verification front end, one item per lane: the key's status and range, the ranges of the commitment
//                         and of s, the slot's length; the flag byte, the key as the equation uses it (BIP0340: the even-y
//                         representative), the scalar s, ECFSDSA's W for the on-curve test, and the staged slot patched with the
//                         signature's own commitment bytes and the key's x
//   (k_ptf op 2 on W; k_sha2_slots; k_schnorr_ne; A = [s]G, B = [q - e]Y; W' = A + B by k_recover_fin / k_recover_redo)
//   k_schnorr_item_cmp    the verdict: BIP0340 finite, y even, x = r; ECFSDSA finite, x || y = r -- under the flags, the on-curve
//                         test of W and the status of W'
//   k_schnorr_item_fill   signing: the commitment (and BIP0340's Y.x) into the blanks of the staged slot; settles the flag byte
//   k_schnorr_item_sign   signing back end: the parity of R, the flips, e from the digest, s.  No inversion.
#pragma once
#include "ecamd_schnorr.h"

template <int NW> __global__ __launch_bounds__(64) void k_schnorr_item_prep(EcamdSchnorrItemArgs A)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int alg = A.alg, qlen = (int)A.qlen, clen = (int)A.clen, hsize = (int)A.hsize;
	const bool bip = alg == ecschnorr::ALG_BIP0340;
	const SigfamOps<NW> ops{A.qslot};
	const int rl = ecschnorr::r_len(alg, clen);
	const u8 *key = A.keys + (size_t)i * 2 * clen, *sig = A.sigs + (size_t)i * (rl + qlen);
	u8 *slot = A.slots + (size_t)i * A.sstride;
	const u32 kst = A.kst ? A.kst[i] : 0u;
	// the key: BIP0340 takes the unique representative (the point at infinity has none); ECFSDSA uses the key as it is
	const bool kinf = !bip & (kst == 2u);
	bool ok = (kst == 0u) | kinf;
	ok = ok & (kinf | (ecschnorr::coord_ok(key, A.p_be, clen) & ecschnorr::coord_ok(key + clen, A.p_be, clen)));
	// the commitment: r < p; W.x, W.y < p (on the curve: k_ptf)
	ok = ok & ecschnorr::coord_ok(sig, A.p_be, clen) & (bip | ecschnorr::coord_ok(sig + clen, A.p_be, clen));
	const Fe<NW> sv = fe_load_be<NW>(sig + rl, qlen);
	ok = ok & ecschnorr::verify_s_ok(ops, alg, sv);
	const bool usable = ecschnorr::slot_ok(alg, *(const u32 *)slot, A.sstride, hsize, clen);
	ok = ok & usable;
	A.flags[i] = ok ? (kinf ? 2 : 0) : 1;
	fe_store_be<NW>(A.s_out + (size_t)i * qlen, qlen, ok ? sv : fe_zero<NW>());
	// a key at infinity has no bytes: the generator stands in (a valid point of the subgroup, whatever the signature holds); its
	// product is not used: k_schnorr_item_cmp reads [s]G for such an item
	u8 *ko = A.key_out + (size_t)i * 2 * clen;
	const u8 *ksrc = kinf ? A.gen : key;
	for (int b = 0; b < clen; b++) {
		ko[b] = ksrc[b];
	}
	if (bip) {
		ecschnorr::lift_y(ko + clen, key + clen, A.p_be, clen);
	} else {
		for (int b = 0; b < clen; b++) {
			ko[clen + b] = ksrc[clen + b];
		}
		u8 *wo = A.w_out + (size_t)i * 2 * clen;
		for (int b = 0; b < 2 * clen; b++) {
			wo[b] = sig[b];
		}
	}
	if (usable) {
		// the verdict depends on key, signature and message only: the commitment field is the signature's
		u8 *d = slot + 4 + ecschnorr::r_off(alg, hsize);
		for (int b = 0; b < rl; b++) {
			d[b] = sig[b];
		}
		if (bip) {
			for (int b = 0; b < clen; b++) {
				d[clen + b] = key[b];
			}
		}
	}
}

__global__ __launch_bounds__(256) void k_schnorr_item_cmp(EcamdSchnorrItemArgs A)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int alg = A.alg, clen = (int)A.clen;
	const int rl = ecschnorr::r_len(alg, clen);
	const u32 fl = A.flags[i];
	const bool kinf = fl == 2u;   // ECFSDSA, the key at infinity: W' = [s]G
	const bool wok = A.wst ? A.wst[i] == 0 : true;
	const u8 *W = (kinf ? A.A : A.W) + (size_t)i * 2 * clen;
	const u32 st = kinf ? A.stA[i] : A.stW[i];
	const bool live = (fl != 1u) & wok & (st == 0u);
	const bool same = ecschnorr::accept(alg, W, A.sigs + (size_t)i * (rl + (int)A.qlen), clen);
	A.out[i] = (live & same) ? 0 : 1;
}

// One byte per thread: byte b of the 2 clen bytes that signing writes into item i's staged slot -- BIP0340: R.x || Y.x behind the
// two tag hashes, ECFSDSA: W.x || W.y at the front.  An item without a commitment or (BIP0340) without a key gets zeros: its digest
// decides nothing.  Thread 0 of an item writes its flag (nothing reads it before k_schnorr_item_sign).
__global__ __launch_bounds__(256) void k_schnorr_item_fill(EcamdSchnorrItemArgs A)
{
	const u32 clen = A.clen, per = 2 * clen;
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= (size_t)A.n * per) {
		return;
	}
	const u32 i = (u32)(t / per), b = (u32)(t % per);
	const bool bip = A.alg == ecschnorr::ALG_BIP0340;
	u8 *slot = A.slots + (size_t)i * A.sstride;
	const bool usable = ecschnorr::slot_ok(A.alg, *(const u32 *)slot, A.sstride, (int)A.hsize, (int)clen);
	const bool have = (A.stW[i] == 0) & (!bip || A.kst[i] == 0);
	const u8 *W = A.W + (size_t)i * per;
	if (usable) {
		const u8 v = (bip && b >= clen) ? A.keys[(size_t)i * per + (b - clen)] : W[b];
		slot[4 + ecschnorr::r_off(A.alg, (int)A.hsize) + b] = have ? v : (u8)0;
	}
	if (b == 0) {
		A.flags[i] = usable ? 0 : 1;
	}
}

// One item per lane.  status 1: what sign_key_ok refuses, k not in [1, q - 1], [k]G not a finite point, BIP0340's key not a
// finite point of the curve, an unusable slot, ECFSDSA's s = 0.
template <int NW> __global__ __launch_bounds__(64) void k_schnorr_item_sign(EcamdSchnorrItemArgs A)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	const int alg = A.alg, qlen = (int)A.qlen, clen = (int)A.clen, hsize = (int)A.hsize;
	const bool bip = alg == ecschnorr::ALG_BIP0340;
	const SigfamOps<NW> ops{A.qslot};
	const int rl = ecschnorr::r_len(alg, clen);
	const Fe<NW> x = fe_load_be<NW>(A.privs + (size_t)i * qlen, qlen);
	const Fe<NW> kk = fe_load_be<NW>(A.nonces + (size_t)i * qlen, qlen);
	bool ok = ecschnorr::sign_key_ok(ops, alg, x) & ecschnorr::nonce_ok(ops, kk) & (A.stW[i] == 0) & (A.flags[i] == 0);
	if (bip) {
		ok = ok & (A.kst[i] == 0);
	}
	const u8 *R = A.W + (size_t)i * 2 * clen;
	Fe<NW> sv = fe_zero<NW>();
	if (ok) {
		const Fe<NW> e = ecschnorr::digest_e(ops, A.dg + (size_t)i * hsize, hsize);
		if (bip) {
			const u8 *Y = A.keys + (size_t)i * 2 * clen;
			sv = ecschnorr::bip0340_s(ops, x, kk, e, ecschnorr::be_is_odd(Y + clen, clen), ecschnorr::be_is_odd(R + clen, clen));
		} else {
			ok = ecschnorr::ecfsdsa_s(ops, x, kk, e, sv);
		}
	}
	u8 *sig = A.out + (size_t)i * (rl + qlen);
	for (int b = 0; b < rl; b++) {
		sig[b] = ok ? R[b] : (u8)0;
	}
	fe_store_be<NW>(sig + rl, qlen, ok ? sv : fe_zero<NW>());
	A.status[i] = ok ? 0 : 1;
}

// every byte the kernels write into a staged slot lies inside it: the fixed fields fit the stride
static bool schnorr_item_args_sane(const EcamdSchnorrItemArgs &a)
{
	return ecschnorr::alg_known(a.alg) && a.hsize >= 20 && a.hsize <= 64 && a.clen >= 1 && a.clen <= 72 && (a.sstride & 3u) == 0 &&   // 20: RIPEMD-160
	       a.sstride >= 4u + (uint32_t)ecschnorr::fixed_len(a.alg, (int)a.hsize, (int)a.clen);
}

hipError_t ecamd_launch_schnorr_item_prep(int nw, const EcamdSchnorrItemArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!schnorr_item_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_schnorr_item_prep<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t ecamd_launch_schnorr_item_cmp(const EcamdSchnorrItemArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!schnorr_item_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_schnorr_item_cmp, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
	return hipGetLastError();
}

hipError_t ecamd_launch_schnorr_item_fill(const EcamdSchnorrItemArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!schnorr_item_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	const size_t bytes = (size_t)a.n * 2 * a.clen;
	hipLaunchKernelGGL(k_schnorr_item_fill, dim3((unsigned)((bytes + 255) / 256)), dim3(256), 0, s, a);
	return hipGetLastError();
}

hipError_t ecamd_launch_schnorr_item_sign(int nw, const EcamdSchnorrItemArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (!schnorr_item_args_sane(a)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (nw) {
#define X(N) case N: hipLaunchKernelGGL(k_schnorr_item_sign<N>, grid, block, 0, s, a); break;
		ECAMD_FOR_NW(X)
#undef X
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
