// libecc_amd/csrc/ecamd_rfc6979.hip -- k_rfc6979_nonce<ALG>: the nonce of deterministic ECDSA (RFC 6979 section 3.2; the reference's
// __ecdsa_rfc6979_nonce, sig/ecdsa_common.c:48-169) for a batch, one item per lane.  The steps are ecamd_rfc6979.h's; this file
// is the launch geometry, the word buffer in LDS and the stores.
//
// Per item about 18 compressions for SHA-256 with a 256-bit order (a hashed short message is one), all on registers: the ipad /
// opad states of the current K, V, the message schedule and the working variables.  The only memory in the loop is the lane's
// column of the word buffer.  Lanes of a wave whose candidate was rejected run the RFC's retry while the others wait; the wave ends
// with its last lane.  Private keys are read octet by octet (qlen = 66 and 29 are no multiple of a word).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_rfc6979.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__constant__ u32 c_rfc_k256[64] = {ECAMD_SHA256_K};
__constant__ u64 c_rfc_k512[80] = {ECAMD_SHA512_K};

template <int ALG> __global__ __launch_bounds__(64) void k_rfc6979_nonce(EcamdRfc6979Args A)
{
	__shared__ u32 sT[ecrfc::TAIL_WORDS * 64];
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= A.n) {
		return;
	}
	u8 *out = A.nonces + (size_t)i * A.qlen;
	u32 k[ecrfc::NL];
	int st = 1;
	// a message slot whose length word does not fit the stride has no digest: no nonce either
	const bool slot_bad = A.slots != nullptr && !ecrfc::slot_ok(*(const u32 *)(A.slots + (size_t)i * A.stride), A.stride);
	if (slot_bad) {
#pragma unroll
		for (int l = 0; l < ecrfc::NL; l++) {
			k[l] = 0;
		}
	} else {
		u32 q[ecrfc::NL];
#pragma unroll
		for (int l = 0; l < ecrfc::NL; l++) {
			q[l] = A.q[l];
		}
		u32 retries;
		if constexpr (ALG == 224 || ALG == 256) {
			st = ecrfc::nonce<ALG>(A.privs + (size_t)i * A.qlen, A.digests + (size_t)i * ecrfc::Alg<ALG>::HSIZE, q, A.qbits, sT + threadIdx.x, 64,
					       (const u32 *)c_rfc_k256, k, &retries);
		} else {
			st = ecrfc::nonce<ALG>(A.privs + (size_t)i * A.qlen, A.digests + (size_t)i * ecrfc::Alg<ALG>::HSIZE, q, A.qbits, sT + threadIdx.x, 64,
					       (const u64 *)c_rfc_k512, k, &retries);
		}
	}
	ecrfc::limbs_to_be(k, out, A.qlen);
	A.status[i] = (u8)st;
}

hipError_t ecamd_launch_rfc6979_nonce(int hash_type, const EcamdRfc6979Args &a, hipStream_t s)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	if (a.qlen == 0 || a.qlen > (uint32_t)ecrfc::MAX_QLEN || a.qlen != (a.qbits + 7) / 8 || (a.slots && (a.stride < 4 || (a.stride & 3u)))) {
		return hipErrorInvalidValue;
	}
	const dim3 grid((a.n + 63) / 64), block(64);
	switch (hash_type) {
	case 1: hipLaunchKernelGGL(k_rfc6979_nonce<224>, grid, block, 0, s, a); break;
	case 2: hipLaunchKernelGGL(k_rfc6979_nonce<256>, grid, block, 0, s, a); break;
	case 3: hipLaunchKernelGGL(k_rfc6979_nonce<384>, grid, block, 0, s, a); break;
	case 4: hipLaunchKernelGGL(k_rfc6979_nonce<512>, grid, block, 0, s, a); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
