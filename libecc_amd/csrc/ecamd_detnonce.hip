// libecc_amd/csrc/ecamd_detnonce.hip -- the two nonce generators that signing schemes of the reference run on their own besides RFC 6979,
// for a batch, one item per lane:
//   k_dbign_nonce<SCAN>     deterministic BIGN, STB 34.101.45 section 6.3.3 (__bign_determinitic_nonce, sig/bign_common.c:200-342)
//   k_bip0340_nonce<ALG>    BIP0340's tagged hashes (_bip0340_sign, sig/bip0340.c:213-294)
// The steps are ecamd_dbign_nonce.h's and ecamd_bip0340_nonce.h's; this file is the launch geometry, the word buffers in LDS, the
// substitution table and the stores.
//
// k_dbign_nonce keeps r (eight blocks), theta and belt-hash's state in registers; the lane's column of the word buffer holds belt-hash's
// input once.  EVERY substitution index of this kernel depends on the private key (ecamd_belt.h).  SCAN = false gathers from the
// 256-octet LDS table as k_belt_slots does (the library's default mode, which allows secret-dependent addresses); SCAN = true
// (secret-scalar mode) reads the table's 64 dwords at wave-uniform addresses for every look-up and selects by compares, one scan
// per four octets.  Both give the same bytes.  Lanes whose candidate was rejected go on while the others wait.
//
// k_bip0340_nonce looks nothing up by a secret.  The message is read from the item's slot where it lies, behind the fixed fields.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_dbign_nonce.h"
#include "ecamd_bip0340_nonce.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__constant__ __attribute__((aligned(16))) u8 c_dn_belt_h[256] = {ECAMD_BELT_H};   // read as dwords by the staging and by the scan
__constant__ u32 c_dn_k256[64] = {ECAMD_SHA256_K};
__constant__ u64 c_dn_k512[80] = {ECAMD_SHA512_K};

template <bool SCAN> __global__ __launch_bounds__(64) void k_dbign_nonce(EcamdDbignNonceArgs A)
{
	__shared__ u32 sT[ecdbign::IN_WORDS * 64];
#if defined(__HIPCC__)
	__shared__ __attribute__((aligned(16))) u8 sH[256];
	((u32 *)sH)[threadIdx.x] = ((const u32 *)c_dn_belt_h)[threadIdx.x];   // 64 threads x 4 octets
	__syncthreads();
	const u8 *tab = sH;
#else
	// a host build (tests/det_nonce_kernel_host_shim.cpp) has no barrier: the table is read where it lies, as in k_belt_slots
	const u8 *tab = c_dn_belt_h;
#endif
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	u32 q[ecdbign::NL], k[ecdbign::NL], rejects;
#pragma unroll
	for (int l = 0; l < ecdbign::NL; l++) {
		q[l] = A.q[l];
	}
	const u8 *priv = A.privs + (size_t)i * A.qlen, *dig = A.digests + (size_t)i * A.hlen;
	int st;
	if constexpr (SCAN) {
		const ecbelt::ScanTab H = {(const u32 *)tab};
		st = ecdbign::nonce(H, priv, dig, A.hlen, A.oid, A.oid_len, A.t, A.t_len, q, A.qbits, sT + threadIdx.x, 64, k, &rejects);
	} else {
		st = ecdbign::nonce(tab, priv, dig, A.hlen, A.oid, A.oid_len, A.t, A.t_len, q, A.qbits, sT + threadIdx.x, 64, k, &rejects);
	}
	ecrfc::limbs_to_be(k, A.nonces + (size_t)i * A.qlen, A.qlen);
	A.status[i] = (u8)st;
}

hipError_t ecamd_launch_dbign_nonce(const EcamdDbignNonceArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (a.qlen == 0 || a.qlen > (uint32_t)ecdbign::MAX_QLEN || a.qlen != (a.qbits + 7) / 8 || a.hlen == 0 || a.hlen > (uint32_t)ecdbign::MAX_DIGEST ||
	    a.oid_len > (uint32_t)ecdbign::MAX_OID || a.t_len > (uint32_t)ecdbign::MAX_T) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	if (a.scan) {
		hipLaunchKernelGGL(k_dbign_nonce<true>, grid, block, 0, s, a);
	} else {
		hipLaunchKernelGGL(k_dbign_nonce<false>, grid, block, 0, s, a);
	}
	return hipGetLastError();
}

template <int ALG> __global__ __launch_bounds__(64) void k_bip0340_nonce(EcamdBip0340NonceArgs A)
{
	typedef typename ecrfc::Alg<ALG>::W W;
	constexpr int VW = ecrfc::Hmac<ALG>::VW, HS = ecrfc::Alg<ALG>::HSIZE;
	__shared__ u32 sT[ecbip::PRE_WORDS * 64];
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	u32 k[ecbip::NL];
#pragma unroll
	for (int l = 0; l < ecbip::NL; l++) {
		k[l] = 0;
	}
	int st = 1;
	const u8 *slot = A.slots + (size_t)i * A.stride;
	const u32 len = *(const u32 *)slot;
	// a slot that does not hold the fixed fields or does not fit the stride, a key that did not import: no nonce
	if (ecbip::slot_ok(len, A.stride, HS, A.clen) && A.kst[i] == 0) {
		u32 q[ecbip::NL];
#pragma unroll
		for (int l = 0; l < ecbip::NL; l++) {
			q[l] = A.q[l];
		}
		W ta[VW], tn[VW];
#pragma unroll
		for (int t = 0; t < VW; t++) {
			ta[t] = (W)A.tag_aux[t];
			tn[t] = (W)A.tag_nonce[t];
		}
		const u32 fixed = ecbip::fixed_len(HS, A.clen);
		const u8 *priv = A.privs + (size_t)i * A.qlen, *Y = A.keys + (size_t)i * 2 * A.clen, *aux = A.aux + (size_t)i * A.qlen;
		if constexpr (ALG == 224 || ALG == 256) {
			st = ecbip::nonce<ALG>(priv, Y, A.clen, aux, ta, tn, slot + 4 + fixed, len - fixed, q, A.qbits, sT + threadIdx.x, 64,
					       (const u32 *)c_dn_k256, k);
		} else {
			st = ecbip::nonce<ALG>(priv, Y, A.clen, aux, ta, tn, slot + 4 + fixed, len - fixed, q, A.qbits, sT + threadIdx.x, 64,
					       (const u64 *)c_dn_k512, k);
		}
	}
	ecrfc::limbs_to_be(k, A.nonces + (size_t)i * A.qlen, A.qlen);
	A.status[i] = (u8)st;
}

hipError_t ecamd_launch_bip0340_nonce(int hash_type, const EcamdBip0340NonceArgs &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (a.qlen == 0 || a.qlen > (uint32_t)ecbip::MAX_QLEN || a.qlen != (a.qbits + 7) / 8 || a.clen == 0 || a.clen > (uint32_t)ecbip::MAX_CLEN ||
	    a.stride < 4 || (a.stride & 3u)) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (hash_type) {
	case 1: hipLaunchKernelGGL(k_bip0340_nonce<224>, grid, block, 0, s, a); break;
	case 2: hipLaunchKernelGGL(k_bip0340_nonce<256>, grid, block, 0, s, a); break;
	case 3: hipLaunchKernelGGL(k_bip0340_nonce<384>, grid, block, 0, s, a); break;
	case 4: hipLaunchKernelGGL(k_bip0340_nonce<512>, grid, block, 0, s, a); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
