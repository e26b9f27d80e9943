// libecc_amd/csrc/ecamd_hash3.hip -- the rest of libecc's table of fixed-length hashes for a batch of short messages, one message per
// lane, in the slot format of ecamd_hash.hip (a little-endian u32 length, then the bytes, one stride per call): SHA3-224 / 256 / 384 /
// 512 (ecamd_keccak.h), SHA-512/224 and SHA-512/256 (ecamd_sha512t.h), RIPEMD-160 (ecamd_rmd160.h) and BASH224 / 256 / 384 / 512
// (ecamd_bash.h), and the one launcher that serves the whole table (ec_digest_slots_batch): it sends the numbers the older files
// serve to their launchers.
//
// All four units are register-only: the sponge states are 25 and 24 64-bit words per lane, the rounds are unrolled so that rotation
// counts and word indices are constants, the round constants sit in constant memory and are indexed by the round number, and there
// is no LDS.  Registers and scratch as the compiler reports them: profiles/r19_hash_table.md.
//
// Everything hashed here is public, so nothing differs in secret-scalar mode.
//
// A slot whose length does not fit its stride gets an all-zero digest, for every hash_type of ecamd_launch_digest_slots (the SHA-2
// kernel of ecamd_hash.hip hashes what fits; k_zero_unfit clears those digests afterwards).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_keccak.h"
#include "ecamd_sha512t.h"
#include "ecamd_rmd160.h"
#include "ecamd_bash.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__constant__ u64 c_h3_keccak_rc[24] = {ECAMD_KECCAK_RC};
__constant__ u64 c_h3_bash_rc[24] = {ECAMD_BASH_RC};
__constant__ u64 c_h3_k512[80] = {ECAMD_SHA512_K};

// HSIZE: 28, 32, 48, 64
template <int HSIZE> __global__ __launch_bounds__(64) void k_sha3_slots(const u8 *slots, u32 stride, u32 n, u8 *out, u32 out_stride)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) {
		return;
	}
	eckk::slot_digest<HSIZE>(c_h3_keccak_rc, slots + (size_t)i * stride, stride, out + (size_t)i * out_stride);
}

// T: 224, 256
template <int T> __global__ __launch_bounds__(64) void k_sha512t_slots(const u8 *slots, u32 stride, u32 n, u8 *out, u32 out_stride)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) {
		return;
	}
	ecs5t::slot_digest<T>((const u64 *)c_h3_k512, slots + (size_t)i * stride, stride, out + (size_t)i * out_stride);
}

__global__ __launch_bounds__(64) void k_rmd160_slots(const u8 *slots, u32 stride, u32 n, u8 *out, u32 out_stride)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) {
		return;
	}
	ecrmd::slot_digest(slots + (size_t)i * stride, stride, out + (size_t)i * out_stride);
}

// BITS: 224, 256, 384, 512
template <int BITS> __global__ __launch_bounds__(64) void k_bash_slots(const u8 *slots, u32 stride, u32 n, u8 *out, u32 out_stride)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) {
		return;
	}
	ecbash::slot_digest<BITS>(c_h3_bash_rc, slots + (size_t)i * stride, stride, out + (size_t)i * out_stride);
}

// behind a kernel that hashes what fits: the digest of a slot that does not fit its stride becomes zeros
__global__ __launch_bounds__(256) void k_zero_unfit(const u8 *slots, u32 stride, u32 n, u8 *out, u32 out_stride, u32 dl)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || *(const u32 *)(slots + (size_t)i * stride) <= stride - 4) {
		return;
	}
	u8 *d = out + (size_t)i * out_stride;
	for (u32 b = 0; b < dl; b++) {
		d[b] = 0;
	}
}

// hash_type: libecc's hash_alg_type numbering.  Every fixed-length hash of the table but belt-hash (16, BIGN's own entry points) and
// SHAKE256 (12, which libecc's table lists with 114 octets for Ed448 alone).
int ecamd_digest_len_any(int hash_type)
{
	if (hash_type < 1 || hash_type > 20 || hash_type == 12 || hash_type == 16) {
		return 0;
	}
	const int dl = eckk::hash_size(hash_type) + ecs5t::hash_size(hash_type) + ecrmd::hash_size(hash_type) + ecbash::hash_size(hash_type);
	return dl ? dl : ecamd_hash_digest_len(hash_type);
}

hipError_t ecamd_launch_digest_slots(int hash_type, const uint8_t *slots, uint32_t stride, uint32_t n, uint8_t *out, uint32_t out_stride, hipStream_t s)
{
	const uint32_t dl = (uint32_t)ecamd_digest_len_any(hash_type);
	if (dl == 0 || stride < 4 || (stride & 3u) || out_stride < dl) {
		return hipErrorInvalidValue;
	}
	if (n == 0) {
		return hipSuccess;
	}
	const dim3 grid((n + 63) / 64), block(64);
#define H3_LAUNCH(K) hipLaunchKernelGGL(K, grid, block, 0, s, slots, stride, n, out, out_stride)
	switch (hash_type) {
	case 5: H3_LAUNCH(k_sha3_slots<28>); break;
	case 6: H3_LAUNCH(k_sha3_slots<32>); break;
	case 7: H3_LAUNCH(k_sha3_slots<48>); break;
	case 8: H3_LAUNCH(k_sha3_slots<64>); break;
	case 9: H3_LAUNCH(k_sha512t_slots<224>); break;
	case 10: H3_LAUNCH(k_sha512t_slots<256>); break;
	case 15: H3_LAUNCH(k_rmd160_slots); break;
	case 17: H3_LAUNCH(k_bash_slots<224>); break;
	case 18: H3_LAUNCH(k_bash_slots<256>); break;
	case 19: H3_LAUNCH(k_bash_slots<384>); break;
	case 20: H3_LAUNCH(k_bash_slots<512>); break;
	default: {
		// 1 .. 4, 11, 13, 14: the kernels of ecamd_hash.hip and ecamd_hash2.hip
		const hipError_t e = ecamd_launch_hash_slots(hash_type, slots, stride, n, out, out_stride, s);
		if (e != hipSuccess || hash_type > 4) {
			return e;
		}
		hipLaunchKernelGGL(k_zero_unfit, dim3((n + 255) / 256), dim3(256), 0, s, slots, stride, n, out, out_stride, dl);
		break;
	}
	}
#undef H3_LAUNCH
	return hipGetLastError();
}
