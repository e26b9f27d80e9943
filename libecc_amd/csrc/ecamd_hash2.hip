// libecc_amd/csrc/ecamd_hash2.hip -- SM3 and Streebog-256 / -512 of a batch of short messages, one message per lane, in the slot format
// of ecamd_hash.hip (a little-endian u32 length, then the bytes, one stride per call), and SM2's Z: the device hashes of the
// message-level ECGDSA / ECRDSA / SM2 entry points (ec_sig_verify_msg_batch, ec_sig_sign_msg_batch, ec_hash_slots_batch).
//
// SM3 is register-only (ecamd_sm3.h).  Streebog (ecamd_streebog.h) gathers from the combined table T[j][b] of 8 x 256 x 64 bits:
// each workgroup builds its 16 KiB copy in LDS once, from pi and A in constant memory (32 entries per lane), and then walks a
// grid-stride loop over the items so that the fill is paid once per workgroup, not once per 64 items.  LDS layout: entry (j, b) at
// word 256 j + b, read with one 64-bit gather per look-up -- 64 per LPS, 13 LPS per g_N; the addresses are message-derived and
// random, so bank conflicts are what a random 64-bit gather meets (not measured here: profiles/r17_sig_msg.md).
//
// Everything hashed here is public (the headers say why), so the look-ups are the same in secret-scalar mode.
//
// A slot whose length does not fit its stride gets an all-zero digest; the callers reject the item.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ecamd_internal.h"
#include "ecamd_sm3.h"
#include "ecamd_streebog.h"
#include "ecamd_sm2z.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

__global__ __launch_bounds__(64) void k_sm3_slots(const u8 *slots, u32 stride, u32 n, u8 *out, u32 out_stride)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) {
		return;
	}
	const u32 *slot = (const u32 *)(slots + (size_t)i * stride);
	const u32 len = slot[0];
	u32 dg[8];
	if (len > stride - 4) {
#pragma unroll
		for (int k = 0; k < 8; k++) {
			dg[k] = 0;
		}
	} else {
		ecsm3::hash_words(slot + 1, len, dg);
	}
	ecsm3::digest_bytes(dg, out + (size_t)i * out_stride);
}

__constant__ u8 c_sb_pi[256] = {ECAMD_STREEBOG_PI};
__constant__ u64 c_sb_a[64] = {ECAMD_STREEBOG_A};
__constant__ u64 c_sb_c[96] = {ECAMD_STREEBOG_C};

// BITS: 256, 512
template <int BITS> __global__ __launch_bounds__(64) void k_streebog_slots(const u8 *slots, u32 stride, u32 n, u8 *out, u32 out_stride)
{
	__shared__ u64 sT[ecsb::TABLE_WORDS];
	for (u32 e = threadIdx.x; e < (u32)ecsb::TABLE_WORDS; e += 64) {
		sT[e] = ecsb::table_entry(c_sb_pi, c_sb_a, e >> 8, e & 255u);
	}
	__syncthreads();
	const u64 *T = sT;
	for (u32 i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64) {
		const u32 *slot = (const u32 *)(slots + (size_t)i * stride);
		const u32 len = slot[0];
		u64 h[8];
		if (len > stride - 4) {
#pragma unroll
			for (int k = 0; k < 8; k++) {
				h[k] = 0;
			}
		} else {
			ecsb::hash_words<BITS>(T, c_sb_c, slot + 1, len, h);
		}
		ecsb::digest_bytes<BITS>(h, out + (size_t)i * out_stride);
	}
}

hipError_t ecamd_launch_sm3_slots(const uint8_t *slots, uint32_t stride, uint32_t n, uint8_t *out, uint32_t out_stride, hipStream_t s)
{
	if (n == 0) {
		return hipSuccess;
	}
	if (stride < 4 || (stride & 3u) || out_stride < 32) {
		return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_sm3_slots, dim3((n + 63) / 64), dim3(64), 0, s, slots, stride, n, out, out_stride);
	return hipGetLastError();
}

hipError_t ecamd_launch_streebog_slots(int hash_type, const uint8_t *slots, uint32_t stride, uint32_t n, uint8_t *out, uint32_t out_stride, hipStream_t s)
{
	if (n == 0) {
		return hipSuccess;
	}
	const uint32_t dl = (uint32_t)ecsb::hash_size(hash_type);
	if (dl == 0 || stride < 4 || (stride & 3u) || out_stride < dl) {
		return hipErrorInvalidValue;
	}
	// at most 2048 workgroups (eight per compute unit of a 256-unit device): beyond that each walks several groups of 64 items
	const uint32_t groups = (n + 63) / 64, grid = groups < 2048u ? groups : 2048u;
	if (hash_type == 13) {
		hipLaunchKernelGGL(k_streebog_slots<256>, dim3(grid), dim3(64), 0, s, slots, stride, n, out, out_stride);
	} else {
		hipLaunchKernelGGL(k_streebog_slots<512>, dim3(grid), dim3(64), 0, s, slots, stride, n, out, out_stride);
	}
	return hipGetLastError();
}

int ecamd_hash_digest_len(int hash_type)
{
	if (hash_type == 11) {
		return ecsm3::DIGEST_BYTES;
	}
	const int sb = ecsb::hash_size(hash_type);
	return sb ? sb : ecamd_sha2_digest_len(hash_type);
}

hipError_t ecamd_launch_hash_slots(int hash_type, const uint8_t *slots, uint32_t stride, uint32_t n, uint8_t *out, uint32_t out_stride, hipStream_t s)
{
	if (hash_type == 11) {
		return ecamd_launch_sm3_slots(slots, stride, n, out, out_stride, s);
	}
	if (ecsb::hash_size(hash_type)) {
		return ecamd_launch_streebog_slots(hash_type, slots, stride, n, out, out_stride, s);
	}
	if (n && out_stride < (uint32_t)ecamd_sha2_digest_len(hash_type)) {
		return hipErrorInvalidValue;
	}
	return ecamd_launch_sha2_slots(hash_type, slots, stride, n, out, out_stride, s);
}

// ---- SM2's Z (ecamd_sm2z.h): one key per lane, from the midstate of the call's prefix ----
__constant__ u32 c_z_k256[64] = {ECAMD_SHA256_K};
__constant__ u64 c_z_k512[80] = {ECAMD_SHA512_K};

__global__ __launch_bounds__(64) void k_sm2_z(ecsm2z::Prefix P, const u8 *keys, u32 klen, u8 *z, u32 hsize, u32 n)
{
	const u32 i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) {
		return;
	}
	ecsm2z::z_item(P, keys + (size_t)i * klen, klen, z + (size_t)i * hsize, (const u32 *)c_z_k256, (const u64 *)c_z_k512);
}

hipError_t ecamd_launch_sm2_z(const ecsm2z::Prefix &P, const uint8_t *keys, uint32_t klen, uint8_t *z, uint32_t hsize, uint32_t n, hipStream_t s)
{
	if (n == 0) {
		return hipSuccess;
	}
	if ((uint32_t)ecsm2z::hash_size(P.hash_type) != hsize || klen == 0 || klen > 2u * ecsm2z::MAX_CLEN || P.tail_len >= ecsm2z::block_size(P.hash_type)) {
		return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_sm2_z, dim3((n + 63) / 64), dim3(64), 0, s, P, keys, klen, z, hsize, n);
	return hipGetLastError();
}

// ---- the per-item rejections of the message-level calls ----
__global__ __launch_bounds__(256) void k_sig_msg_bad(const u8 *slots, u32 stride, u32 blank, const u8 *kst, u8 *bad, u32 n)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) {
		return;
	}
	const u32 len = *(const u32 *)(slots + (size_t)i * stride);
	bad[i] = (len > stride - 4 || len < blank || (kst && kst[i] != 0)) ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_sig_msg_reject_sign(u8 *sigs, u32 siglen, u8 *status, const u8 *bad, u32 n)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || !bad[i]) {
		return;
	}
	status[i] = 1;
	u8 *d = sigs + (size_t)i * siglen;
	for (u32 b = 0; b < siglen; b++) {
		d[b] = 0;
	}
}
hipError_t ecamd_launch_sig_msg_bad(const uint8_t *slots, uint32_t stride, uint32_t blank, const uint8_t *kst, uint8_t *bad, uint32_t n, hipStream_t s)
{
	if (n == 0) {
		return hipSuccess;
	}
	if (stride < 4 || (stride & 3u)) {
		return hipErrorInvalidValue;
	}
	hipLaunchKernelGGL(k_sig_msg_bad, dim3((n + 255) / 256), dim3(256), 0, s, slots, stride, blank, kst, bad, n);
	return hipGetLastError();
}
hipError_t ecamd_launch_sig_msg_reject_sign(uint8_t *sigs, uint32_t siglen, uint8_t *status, const uint8_t *bad, uint32_t n, hipStream_t s)
{
	if (n) {
		hipLaunchKernelGGL(k_sig_msg_reject_sign, dim3((n + 255) / 256), dim3(256), 0, s, sigs, siglen, status, bad, n);
	}
	return hipGetLastError();
}
