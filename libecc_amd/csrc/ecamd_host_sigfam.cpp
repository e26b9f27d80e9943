// libecc_amd/csrc/ecamd_host_sigfam.cpp -- host side of the C ABI declared in include/libecc_amd.h: the signature families that hash on the device, and the message-level forms
// (ecamd_host_internal.h says what the host units share and how they are laid out).
#include "ecamd_host_internal.h"
#include "ecamd_sighash.h"
#include "ecamd_schnorr.h"
#include "ecamd_bign.h"
#include "ecamd_rfc6979.h"
#include "ecamd_dbign_nonce.h"
#include "ecamd_bip0340_nonce.h"
#include "ecamd_bip0340_nonce_ht.h"
#include "ecamd_sm2z.h"
#include <mutex>

using namespace ecamd_host;

// ------------------------------------------------------------------------------------------
// The commitment hash of the five schemes that hash AFTER their multiplication (ECKCDSA / ECSDSA / ECOSDSA, ECFSDSA / BIP0340).  The
// older names (ec_sig_hashed_*, ec_schnorr_*_batch, ec_bip0340_*_batch) take hash_type 1 .. 4; their _ht forms take every hash of
// ec_digest_slots_batch.  Both run the cores below: `ht` only widens the set the argument check admits.  1 .. 4 launch k_sha2_slots
// alone whichever name was called (the same kernels, bytes and speed); the others go through ecamd_hash3.hip's launcher, which gives
// a slot that does not fit its stride an all-zero digest -- such an item is flagged by the fill kernels before its digest is read.
// ------------------------------------------------------------------------------------------
static const char *const HT_SET = "hash_type must be 1 .. 11, 13 .. 15 or 17 .. 20 (every fixed-length hash of libecc's table but belt-hash)";

static uint32_t commit_hsize(int hash_type)
{
	return (uint32_t)ecamd_digest_len_any(hash_type);   // 1 .. 4: echsig::hash_size's values; 20 for RIPEMD-160
}

static int commit_hash_ok(const char *fn, bool ht, int hash_type)
{
	if (ht ? commit_hsize(hash_type) == 0 : echsig::hash_size(hash_type) == 0) {
		return fail(std::string(fn) + ": " + (ht ? HT_SET : "hash_type must be 1 .. 4 (SHA-224, SHA-256, SHA-384, SHA-512)"));
	}
	return 0;
}

static hipError_t commit_hash_launch(int hash_type, const uint8_t *slots, uint32_t stride, uint32_t m, uint8_t *out, uint32_t hsize, hipStream_t s)
{
	if (hash_type >= 1 && hash_type <= 4) {
		return ecamd_launch_sha2_slots(hash_type, slots, stride, m, out, hsize, s);
	}
	return ecamd_launch_digest_slots(hash_type, slots, stride, m, out, hsize, s);
}

// ------------------------------------------------------------------------------------------
// batched ECSDSA / ECOSDSA / ECKCDSA (include/libecc_amd.h: ec_sig_hashed_*): the schemes that hash the commitment.  Per chunk of
// at most max_chunk items, verification is
//   k_hsig_prep       s in [1, q - 1], e from r, the multipliers u (of G) and v (of Y), the flag byte
//   A = [u]G, B = [v]Y one fixed-base and one variable-base pass; on a cofactor curve [q]Y too, as ECDSA verification does
//   k_recover_fin     W' = A + B as affine bytes, one shared inversion per eight items (its second sum A - B is not used)
//   k_recover_redo    the items with A or B at infinity or x_A = x_B, on the complete formulas
//   k_hsig_fill       W' into the blank of a copy of the caller's slots, or ECKCDSA's slot of FE2OS(W'x)
//   k_sha2_slots      the digest
//   k_hsig_cmp        the digest against r
// and signing is [k]G (secret-scalar mode as the context says), k_hsig_fill, k_sha2_slots, k_hsig_sign.
// Frames: ST_ with ST_SLOTS and ST_DIGESTS; signing SG_.  Only enqueues.
// ------------------------------------------------------------------------------------------
static uint32_t hsig_staged_stride(const ecamd_curve *cv, int alg, uint32_t stride)
{
	return alg == ECAMD_SIG_ECKCDSA ? (uint32_t)((4 + cv->clen + 3) & ~3) : stride;
}

// a stride that cannot hold the length word and the blank: no slot is usable, every item is rejected
static bool hsig_no_room(const ecamd_curve *cv, int alg, uint32_t stride)
{
	return alg != ECAMD_SIG_ECKCDSA && stride < 4u + (uint32_t)echsig::blank_len(alg, cv->clen);
}

static int hsig_stage_hash(ecamd_ctx *ctx, int hash_type, uint32_t m, EcamdHsigArgs &H, const uint8_t *d_in, uint32_t stride,
			   hipStream_t s)
{
	uint8_t **S = ctx->stage;
	if (H.alg != ECAMD_SIG_ECKCDSA) {
		// the caller's array is not modified: the coordinates go into a copy
		HIPCHK(hipMemcpyAsync(S[ST_SLOTS], d_in, (size_t)m * stride, hipMemcpyDeviceToDevice, s));
	}
	H.slots = S[ST_SLOTS];
	H.dg = S[ST_DIGESTS];
	HIPCHK(ecamd_launch_hsig_fill(H, s));
	HIPCHK(commit_hash_launch(hash_type, S[ST_SLOTS], H.sstride, m, S[ST_DIGESTS], H.hsize, s));
	return 0;
}

static int hsig_verify_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *d_pub,
				  const uint8_t *d_sig, const uint8_t *d_in, uint32_t stride, uint8_t *d_res, hipStream_t s)
{
	PublicScalars pub_scope(ctx);   // u, v and the group order are public
	const size_t cl = (size_t)cv->clen, plen = 2 * cl, ql = (size_t)cv->qlen;
	const uint32_t hsize = commit_hsize(hash_type);
	if (hsig_no_room(cv, alg, stride)) {
		HIPCHK(hipMemsetAsync(d_res, 1, n, s));
		return 0;
	}
	const size_t siglen = (size_t)echsig::r_len(alg, (int)hsize, (int)ql) + ql;
	const uint32_t sstride = hsig_staged_stride(cv, alg, stride);
	const uint32_t chunk = chunk_items(ctx, n);
	if (verify_sum_need(ctx, cv, chunk) || stage_need(ctx, {{ST_SLOTS, (size_t)chunk * sstride}, {ST_DIGESTS, (size_t)chunk * hsize}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *pub = d_pub + (size_t)off * plen, *in = d_in + (size_t)off * stride;
		EcamdHsigArgs H;
		memset(&H, 0, sizeof(H));
		H.sigs = d_sig + (size_t)off * siglen;
		H.inputs = in;
		H.u = S[ST_U];
		H.v = S[ST_V];
		H.flags = S[ST_FLAGS];
		H.W = S[ST_W];
		H.stW = S[ST_STW];
		H.out = d_res + off;
		H.n = m;
		H.qlen = (uint32_t)ql;
		H.clen = (uint32_t)cl;
		H.hsize = hsize;
		H.sstride = sstride;
		H.qslot = cv->qslot;
		H.alg = alg;
		HIPCHK(ecamd_launch_hsig_prep(cv->qnw, H, s));
		if (verify_sum_dev(ctx, cv, m, pub, s) || hsig_stage_hash(ctx, hash_type, m, H, in, stride, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_hsig_cmp(H, s));
		return 0;
	});
}

static int hsig_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *d_privs,
				const uint8_t *d_nonces, const uint8_t *d_in, uint32_t stride, uint8_t *d_sigs, uint8_t *d_status, hipStream_t s)
{
	const size_t cl = (size_t)cv->clen, plen = 2 * cl, ql = (size_t)cv->qlen;
	const uint32_t hsize = commit_hsize(hash_type);
	const size_t siglen = (size_t)echsig::r_len(alg, (int)hsize, (int)ql) + ql;
	const uint32_t sstride = hsig_staged_stride(cv, alg, stride);
	if (hsig_no_room(cv, alg, stride)) {
		HIPCHK(hipMemsetAsync(d_sigs, 0, n * siglen, s));
		HIPCHK(hipMemsetAsync(d_status, 1, n, s));
		return 0;
	}
	const uint32_t chunk = chunk_items(ctx, n);
	if (stage_need(ctx, SG_KG, chunk * plen) || stage_need(ctx, SG_STKG, chunk) ||
	    stage_need(ctx, ST_FLAGS, chunk) || stage_need(ctx, ST_SLOTS, (size_t)chunk * sstride) ||
	    stage_need(ctx, ST_DIGESTS, (size_t)chunk * hsize)) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *in = d_in + (size_t)off * stride;
		if (smul_dev_locked(ctx, cv, m, d_nonces + off * ql, (uint32_t)ql, nullptr, S[SG_KG], S[SG_STKG], s)) {   // W = [k]G
			return -1;
		}
		EcamdHsigArgs H;
		memset(&H, 0, sizeof(H));
		H.inputs = in;
		H.privs = d_privs + off * ql;
		H.nonces = d_nonces + off * ql;
		H.flags = S[ST_FLAGS];
		H.W = S[SG_KG];
		H.stW = S[SG_STKG];
		H.out = d_sigs + (size_t)off * siglen;
		H.status = d_status + off;
		H.n = m;
		H.qlen = (uint32_t)ql;
		H.clen = (uint32_t)cl;
		H.hsize = hsize;
		H.sstride = sstride;
		H.qslot = cv->qslot;
		H.alg = alg;
		H.sign = 1;
		if (hsig_stage_hash(ctx, hash_type, m, H, in, stride, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_hsig_sign(cv->qnw, H, s));
		return 0;
	});
}

static int hsig_args_ok(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *a, const void *b,
			const void *c, const void *d, const void *e, uint32_t stride)
{
	if (!echsig::alg_known(alg)) {
		return fail(std::string(fn) + ": alg must be ECAMD_SIG_ECKCDSA, ECAMD_SIG_ECSDSA or ECAMD_SIG_ECOSDSA");
	}
	if (commit_hash_ok(fn, ht, hash_type)) {
		return -1;
	}
	if (!ctx || !cv || cv->ctx != ctx || (n && (!a || !b || !c || !d || !e))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->qslot < 0) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	if (alg == ECAMD_SIG_ECKCDSA) {
		if (stride != commit_hsize(hash_type)) {
			return fail(std::string(fn) + ": ECKCDSA takes digests h = H(z || m): stride must be the hash's digest size");
		}
	} else if ((stride & 3u) || stride > 4096 || stride < 4) {
		return fail(std::string(fn) + ": stride must be a multiple of 4 in 4 .. 4096");
	}
	return 0;
}

static int ec_sig_hashed_verify_batch_dev_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n,
					       const void *d_pubkeys, const void *d_sigs, const void *d_inputs, uint32_t stride, void *d_result,
					       void *hip_stream)
{
	if (hsig_args_ok(fn, ht, ctx, cv, alg, hash_type, n, d_pubkeys, d_sigs, d_inputs, d_result, d_result, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return hsig_verify_dev_locked(ctx, cv, alg, hash_type, n, (const uint8_t *)d_pubkeys, (const uint8_t *)d_sigs, (const uint8_t *)d_inputs, stride,
					      (uint8_t *)d_result, s);
	});
}

static int ec_sig_hashed_verify_batch_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n,
					   const uint8_t *pubkeys, const uint8_t *sigs, const uint8_t *inputs, uint32_t stride, uint8_t *result)
{
	if (hsig_args_ok(fn, ht, ctx, cv, alg, hash_type, n, pubkeys, sigs, inputs, result, result, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t siglen = (size_t)echsig::r_len(alg, (int)commit_hsize(hash_type), cv->qlen) + cv->qlen;
	const std::vector<HostArr> arrs = {{pubkeys, nullptr, (size_t)2 * cv->clen}, {sigs, nullptr, siglen}, {inputs, nullptr, stride}, {nullptr, result, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return hsig_verify_dev_locked(ctx, cv, alg, hash_type, m, ip[0], ip[1], ip[2], stride, op[3], s);
	});
}

static int ec_sig_hashed_sign_batch_dev_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n,
					     const void *d_privs, const void *d_nonces, const void *d_inputs, uint32_t stride, void *d_sigs,
					     void *d_status, void *hip_stream)
{
	if (hsig_args_ok(fn, ht, ctx, cv, alg, hash_type, n, d_privs, d_nonces, d_inputs, d_sigs, d_status, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return hsig_sign_dev_locked(ctx, cv, alg, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_nonces, (const uint8_t *)d_inputs, stride,
					    (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

static int ec_sig_hashed_sign_batch_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n,
					 const uint8_t *privs, const uint8_t *nonces, const uint8_t *inputs, uint32_t stride, uint8_t *sigs,
					 uint8_t *status)
{
	if (hsig_args_ok(fn, ht, ctx, cv, alg, hash_type, n, privs, nonces, inputs, sigs, status, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const size_t siglen = (size_t)echsig::r_len(alg, (int)commit_hsize(hash_type), cv->qlen) + ql;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {nonces, nullptr, ql}, {inputs, nullptr, stride}, {nullptr, sigs, siglen}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return hsig_sign_dev_locked(ctx, cv, alg, hash_type, m, ip[0], ip[1], ip[2], stride, op[3], op[4], s);
	});
}

// ------------------------------------------------------------------------------------------
// batched BIGN / DBIGN (include/libecc_amd.h: ec_bign_*): the scheme that hashes its commitment with belt-hash.  Per chunk of at
// most max_chunk items, verification is
//   k_sha2_slots / k_belt_slots   hash_type != 0 only: the digests of the caller's message slots
//   k_bign_prep       s1 < q, hbar, the multipliers u (of G) and v (of Y), the flag byte
//   A = [u]G, B = [v]Y one fixed-base and one variable-base pass (public scalars); on a cofactor curve [q]Y too, as ECDSA verification does
//   k_recover_fin     W' = A + B as affine bytes, one shared inversion per eight items (its second sum A - B is not used)
//   k_recover_redo    the items with A or B at infinity (u = 0) or x_A = x_B, on the complete formulas
//   k_bign_fill       belt-hash's slot OID || <LE(W'x) || LE(W'y)>_2l || digest
//   k_belt_slots      t
//   k_bign_cmp        t against s0
// and signing is [k]G (secret-scalar mode as the context says), k_bign_fill, k_belt_slots, k_bign_sign.
// Frames: ST_ with ST_SLOTS (belt-hash's slots), ST_DIGESTS (the digests of the messages) and ST_BELT; signing SG_.  Only enqueues.
// ------------------------------------------------------------------------------------------
static int bign_message_digests(ecamd_ctx *ctx, int hash_type, uint32_t m, const uint8_t *d_in, uint32_t stride, EcamdBignArgs &B, hipStream_t s)
{
	if (hash_type == 0) {
		B.dg = d_in;          // the caller hashed: stride is the digest length
		B.mslots = nullptr;
		return 0;
	}
	uint8_t **S = ctx->stage;
	if (hash_type == ecbign::HASH_BELT) {
		HIPCHK(ecamd_launch_belt_slots(d_in, stride, m, S[ST_DIGESTS], B.hsize, s));
	} else {
		HIPCHK(ecamd_launch_sha2_slots(hash_type, d_in, stride, m, S[ST_DIGESTS], B.hsize, s));
	}
	B.dg = S[ST_DIGESTS];
	B.mslots = d_in;
	B.mstride = stride;
	return 0;
}

static void bign_args(EcamdBignArgs &B, const ecamd_curve *cv, int hash_type, uint32_t stride, const uint8_t *oid, uint32_t oid_len, uint32_t m)
{
	memset(&B, 0, sizeof(B));
	B.n = m;
	B.qlen = (uint32_t)cv->qlen;
	B.clen = (uint32_t)cv->clen;
	B.hsize = hash_type == 0 ? stride : (uint32_t)ecbign::hash_size(hash_type);
	B.oid_len = oid_len;
	B.bstride = ecbign::belt_stride(oid_len, cv->qlen, B.hsize);
	B.qslot = cv->qslot;
	if (oid_len) {
		memcpy(B.oid, oid, oid_len);
	}
}

static int bign_stage_belt(ecamd_ctx *ctx, EcamdBignArgs &B, hipStream_t s)
{
	uint8_t **S = ctx->stage;
	B.slots = S[ST_SLOTS];
	B.bt = S[ST_BELT];
	HIPCHK(ecamd_launch_bign_fill(B, s));
	HIPCHK(ecamd_launch_belt_slots(S[ST_SLOTS], B.bstride, B.n, S[ST_BELT], ecbign::DIGEST_BT, s));
	return 0;
}

static int bign_verify_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig,
				  const uint8_t *d_in, uint32_t stride, const uint8_t *oid, uint32_t oid_len, uint8_t *d_res, hipStream_t s)
{
	PublicScalars pub_scope(ctx);   // u, v and the group order are public
	const size_t cl = (size_t)cv->clen, plen = 2 * cl, siglen = (size_t)ecbign::sig_len(cv->qlen);
	const uint32_t chunk = chunk_items(ctx, n);
	EcamdBignArgs B;
	bign_args(B, cv, hash_type, stride, oid, oid_len, chunk);
	if (verify_sum_need(ctx, cv, chunk) ||
	    stage_need(ctx, {{ST_SLOTS, (size_t)chunk * B.bstride}, {ST_DIGESTS, hash_type ? (size_t)chunk * B.hsize : 0},
			     {ST_BELT, (size_t)chunk * ecbign::DIGEST_BT}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *pub = d_pub + (size_t)off * plen;
		B.n = m;
		B.sigs = d_sig + (size_t)off * siglen;
		B.u = S[ST_U];
		B.v = S[ST_V];
		B.flags = S[ST_FLAGS];
		B.W = S[ST_W];
		B.stW = S[ST_STW];
		B.out = d_res + off;
		if (bign_message_digests(ctx, hash_type, m, d_in + (size_t)off * stride, stride, B, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_bign_prep(cv->qnw, B, s));
		if (verify_sum_dev(ctx, cv, m, pub, s) || bign_stage_belt(ctx, B, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_bign_cmp(B, s));
		return 0;
	});
}

static int bign_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_privs, const uint8_t *d_nonces,
				const uint8_t *d_in, uint32_t stride, const uint8_t *oid, uint32_t oid_len, uint8_t *d_sigs, uint8_t *d_status,
				hipStream_t s)
{
	const size_t cl = (size_t)cv->clen, plen = 2 * cl, ql = (size_t)cv->qlen, siglen = (size_t)ecbign::sig_len(cv->qlen);
	const uint32_t chunk = chunk_items(ctx, n);
	EcamdBignArgs B;
	bign_args(B, cv, hash_type, stride, oid, oid_len, chunk);
	if (stage_need(ctx, SG_KG, chunk * plen) || stage_need(ctx, SG_STKG, chunk) ||
	    stage_need(ctx, ST_SLOTS, (size_t)chunk * B.bstride) ||
	    stage_need(ctx, ST_DIGESTS, hash_type ? (size_t)chunk * B.hsize : 0) ||
	    stage_need(ctx, ST_BELT, (size_t)chunk * ecbign::DIGEST_BT)) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		if (smul_dev_locked(ctx, cv, m, d_nonces + off * ql, (uint32_t)ql, nullptr, S[SG_KG], S[SG_STKG], s)) {   // W = [k]G
			return -1;
		}
		B.n = m;
		B.privs = d_privs + off * ql;
		B.nonces = d_nonces + off * ql;
		B.W = S[SG_KG];
		B.stW = S[SG_STKG];
		B.out = d_sigs + (size_t)off * siglen;
		B.status = d_status + off;
		B.sign = 1;
		if (bign_message_digests(ctx, hash_type, m, d_in + (size_t)off * stride, stride, B, s) || bign_stage_belt(ctx, B, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_bign_sign(cv->qnw, B, s));
		return 0;
	});
}

static int bign_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *a, const void *b,
			const void *c, const void *d, const void *e, uint32_t stride, const uint8_t *oid, uint32_t oid_len)
{
	if (!ecbign::alg_known(alg)) {
		return fail(std::string(fn) + ": alg must be ECAMD_SIG_BIGN or ECAMD_SIG_DBIGN");
	}
	if (hash_type != 0 && ecbign::hash_size(hash_type) == 0) {
		return fail(std::string(fn) + ": hash_type must be 0 (inputs are digests), 1 .. 4 (SHA-224 / 256 / 384 / 512) or ECAMD_HASH_BELT");
	}
	if (oid_len > (uint32_t)ecbign::MAX_OID || (oid_len && !oid)) {
		return fail(std::string(fn) + ": oid_len must be 0 .. 64, and oid non-NULL when it is not 0");
	}
	if (!ctx || !cv || cv->ctx != ctx || (n && (!a || !b || !c || !d || !e))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->qslot < 0) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	if (hash_type == 0) {
		if (stride < 1 || stride > (uint32_t)ecbign::MAX_DIGEST) {
			return fail(std::string(fn) + ": hash_type 0 takes digests: stride must be the digest length, 1 .. 128");
		}
	} else if ((stride & 3u) || stride > 4096 || stride < 4) {
		return fail(std::string(fn) + ": stride must be a multiple of 4 in 4 .. 4096");
	}
	return 0;
}

extern "C" int ec_bign_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_pubkeys,
					const void *d_sigs, const void *d_inputs, uint32_t stride, const uint8_t *oid, uint32_t oid_len, void *d_result,
					void *hip_stream)
{
	if (bign_args_ok("ec_bign_verify_batch_dev", ctx, cv, alg, hash_type, n, d_pubkeys, d_sigs, d_inputs, d_result, d_result, stride, oid, oid_len)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return bign_verify_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_pubkeys, (const uint8_t *)d_sigs, (const uint8_t *)d_inputs, stride, oid,
					      oid_len, (uint8_t *)d_result, s);
	});
}

extern "C" int ec_bign_verify_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *pubkeys,
				    const uint8_t *sigs, const uint8_t *inputs, uint32_t stride, const uint8_t *oid, uint32_t oid_len, uint8_t *result)
{
	if (bign_args_ok("ec_bign_verify_batch", ctx, cv, alg, hash_type, n, pubkeys, sigs, inputs, result, result, stride, oid, oid_len)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const std::vector<HostArr> arrs = {{pubkeys, nullptr, (size_t)2 * cv->clen}, {sigs, nullptr, (size_t)ecbign::sig_len(cv->qlen)},
					   {inputs, nullptr, stride}, {nullptr, result, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return bign_verify_dev_locked(ctx, cv, hash_type, m, ip[0], ip[1], ip[2], stride, oid, oid_len, op[3], s);
	});
}

extern "C" int ec_bign_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_privs,
				      const void *d_nonces, const void *d_inputs, uint32_t stride, const uint8_t *oid, uint32_t oid_len, void *d_sigs,
				      void *d_status, void *hip_stream)
{
	if (bign_args_ok("ec_bign_sign_batch_dev", ctx, cv, alg, hash_type, n, d_privs, d_nonces, d_inputs, d_sigs, d_status, stride, oid, oid_len)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return bign_sign_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_nonces, (const uint8_t *)d_inputs, stride, oid,
					    oid_len, (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_bign_sign_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *privs,
				  const uint8_t *nonces, const uint8_t *inputs, uint32_t stride, const uint8_t *oid, uint32_t oid_len, uint8_t *sigs,
				  uint8_t *status)
{
	if (bign_args_ok("ec_bign_sign_batch", ctx, cv, alg, hash_type, n, privs, nonces, inputs, sigs, status, stride, oid, oid_len)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {nonces, nullptr, ql}, {inputs, nullptr, stride},
					   {nullptr, sigs, (size_t)ecbign::sig_len(cv->qlen)}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return bign_sign_dev_locked(ctx, cv, hash_type, m, ip[0], ip[1], ip[2], stride, oid, oid_len, op[3], op[4], s);
	});
}

// ------------------------------------------------------------------------------------------
// BIP0340 / ECFSDSA item by item (include/libecc_amd.h: ec_schnorr_verify_batch, ec_schnorr_sign_batch): the two schemes whose
// signature carries the commitment as a point.  Per chunk of at most max_chunk items, verification is
//   k_prj_import           projective keys only: prj_pt_import_from_buf + prj_pt_unique (affine keys are validated by the multiplication)
//   k_schnorr_item_prep    key status and ranges, r < p (W.x, W.y < p), s in range, the slot's length; the flag byte, the key as
//                          the equation uses it, s; the copy of the caller's slots patched with the signature's r (W) and the key's x
//   k_ptf (op 2)           ECFSDSA: W on the curve
//   k_sha2_slots, k_schnorr_ne   e = H(slot) mod q, then q - e
//   A = [s]G, B = [q - e]Y one fixed-base and one variable-base pass; on a cofactor curve [q]Y too, as ECDSA verification does
//   k_recover_fin / _redo  W' = A + B as affine bytes, one shared inversion per eight items; the exceptional pairs on the complete formulas
//   k_schnorr_item_cmp     BIP0340: finite, y even, x = r; ECFSDSA: finite, x || y = r
// and signing is [k]G (secret-scalar mode as the context says), BIP0340: Y = [x]G (the same) or the caller's key through k_ptf (op 2),
// k_schnorr_item_fill, k_sha2_slots, k_schnorr_item_sign.
// Frames: ST_ (ST_U holds s, ST_V q - e) with ST_SLOTS, ST_DIGESTS and SI_; signing SG_.  Only enqueues.
// ------------------------------------------------------------------------------------------
static bool schnorr_item_no_room(const ecamd_curve *cv, int alg, uint32_t hsize, uint32_t stride)
{
	return stride < 4u + (uint32_t)ecschnorr::fixed_len(alg, (int)hsize, cv->clen);
}

static void schnorr_item_args(EcamdSchnorrItemArgs &H, const ecamd_curve *cv, int alg, uint32_t hsize, uint32_t stride, uint32_t m)
{
	memset(&H, 0, sizeof(H));
	H.n = m;
	H.qlen = (uint32_t)cv->qlen;
	H.clen = (uint32_t)cv->clen;
	H.hsize = hsize;
	H.sstride = stride;
	H.qslot = cv->qslot;
	H.alg = alg;
	big_to_be(H.p_be, cv->clen, cv->p);
}

static int schnorr_item_verify_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *d_keys,
					  int key_fmt, const uint8_t *d_sig, const uint8_t *d_in, uint32_t stride, uint8_t *d_res, hipStream_t s)
{
	PublicScalars pub_scope(ctx);   // s, q - e and the group order are public
	const size_t cl = (size_t)cv->clen, plen = 2 * cl, ql = (size_t)cv->qlen;
	const uint32_t hsize = commit_hsize(hash_type);
	if (schnorr_item_no_room(cv, alg, hsize, stride)) {
		HIPCHK(hipMemsetAsync(d_res, 1, n, s));
		return 0;
	}
	const bool fs = alg == ECAMD_SIG_ECFSDSA, prj = key_fmt == ECAMD_PT_PROJECTIVE;
	const size_t siglen = (size_t)ecschnorr::r_len(alg, (int)cl) + ql, kw = (prj ? 3 : 2) * cl;
	const uint32_t chunk = chunk_items(ctx, n);
	if (verify_sum_need(ctx, cv, chunk) ||
	    stage_need(ctx, {{ST_SLOTS, (size_t)chunk * stride}, {ST_DIGESTS, (size_t)chunk * hsize}, {SI_KEY, chunk * plen},
			     {SI_PRJ_AFF, prj ? chunk * plen : 0}, {SI_PRJ_ST, prj ? chunk : 0}, {SI_WPT, fs ? chunk * plen : 0}, {SI_WST, fs ? chunk : 0}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	EcamdSchnorrNeArgs N;
	memset(&N, 0, sizeof(N));
	for (int w = 0; w < 18; w++) {
		N.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
	}
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *keys = d_keys + (size_t)off * kw, *kst = nullptr;
		if (prj) {
			EcamdPrjInArgs I;
			I.in = keys;
			I.aff = S[SI_PRJ_AFF];
			I.pre = S[SI_PRJ_ST];
			I.n = m;
			I.clen = (uint32_t)cl;
			I.for_mul = fs ? 1 : 0;   // (0 : 0 : 0): ECFSDSA multiplies the key as it is, BIP0340 takes its unique representative
			I.slot = cv->slot;
			HIPCHK(launch_prj_import(cv, I, s));
			keys = S[SI_PRJ_AFF];
			kst = S[SI_PRJ_ST];
		}
		// the caller's array is not modified: the patches go into a copy
		HIPCHK(hipMemcpyAsync(S[ST_SLOTS], d_in + (size_t)off * stride, (size_t)m * stride, hipMemcpyDeviceToDevice, s));
		EcamdSchnorrItemArgs H;
		schnorr_item_args(H, cv, alg, hsize, stride, m);
		H.keys = keys;
		H.kst = kst;
		H.gen = cv->d_gen;
		H.sigs = d_sig + (size_t)off * siglen;
		H.slots = S[ST_SLOTS];
		H.key_out = S[SI_KEY];
		H.s_out = S[ST_U];
		H.w_out = fs ? S[SI_WPT] : nullptr;
		H.flags = S[ST_FLAGS];
		H.wst = fs ? S[SI_WST] : nullptr;
		H.A = S[ST_A];
		H.stA = S[ST_STA];
		H.W = S[ST_W];
		H.stW = S[ST_STW];
		H.out = d_res + off;
		HIPCHK(ecamd_launch_schnorr_item_prep(cv->qnw, H, s));
		if (fs) {
			// "Reject the signature if r is not a valid point on the curve" (ecfsdsa.c:449-460): the on-curve test the point calls use
			EcamdPtfArgs T;
			memset(&T, 0, sizeof(T));
			T.p1 = S[SI_WPT];
			T.p2 = S[SI_WPT];
			T.out = S[SI_WPT];   // untouched by op 2
			T.status = S[SI_WST];
			T.n = m;
			T.clen = (uint32_t)cl;
			T.op = 2;
			T.slot = cv->slot;
			HIPCHK(ecamd_launch_ptf(cv->nw, T, s));
		}
		HIPCHK(commit_hash_launch(hash_type, S[ST_SLOTS], stride, m, S[ST_DIGESTS], hsize, s));
		N.dig = S[ST_DIGESTS];
		N.ne = S[ST_V];
		N.n = m;
		N.hlen = hsize;
		N.qlen = (uint32_t)ql;
		HIPCHK(ecamd_launch_schnorr_ne(cv->qnw, N, s));
		// k_recover_fin takes ANY non-zero flag as "no sum for this item": that holds for flag 2 too (ECFSDSA, the key at infinity),
		// whose verdict k_schnorr_item_cmp reads from A = [s]G and stA, not from W'
		if (verify_sum_dev(ctx, cv, m, S[SI_KEY], s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_schnorr_item_cmp(H, s));
		return 0;
	});
}

static int schnorr_item_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *d_privs,
					const uint8_t *d_pubs, const uint8_t *d_nonces, const uint8_t *d_in, uint32_t stride, uint8_t *d_sigs,
					uint8_t *d_status, hipStream_t s)
{
	const size_t cl = (size_t)cv->clen, plen = 2 * cl, ql = (size_t)cv->qlen;
	const uint32_t hsize = commit_hsize(hash_type);
	const size_t siglen = (size_t)ecschnorr::r_len(alg, (int)cl) + ql;
	if (schnorr_item_no_room(cv, alg, hsize, stride)) {
		HIPCHK(hipMemsetAsync(d_sigs, 0, n * siglen, s));
		HIPCHK(hipMemsetAsync(d_status, 1, n, s));
		return 0;
	}
	const bool bip = alg == ECAMD_SIG_BIP0340;
	const uint32_t chunk = chunk_items(ctx, n);
	if (stage_need(ctx, SG_KG, chunk * plen) || stage_need(ctx, SG_STKG, chunk) ||
	    stage_need(ctx, ST_FLAGS, chunk) || stage_need(ctx, ST_SLOTS, (size_t)chunk * stride) ||
	    stage_need(ctx, ST_DIGESTS, (size_t)chunk * hsize) ||
	    (bip && (stage_need(ctx, SG_Y, chunk * plen) || stage_need(ctx, SG_STY, chunk)))) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		if (smul_dev_locked(ctx, cv, m, d_nonces + off * ql, (uint32_t)ql, nullptr, S[SG_KG], S[SG_STKG], s)) {   // R = [k]G
			return -1;
		}
		EcamdSchnorrItemArgs H;
		schnorr_item_args(H, cv, alg, hsize, stride, m);
		if (bip && d_pubs) {
			// the key pair's public half as the caller holds it: coordinates < p and on the curve
			EcamdPtfArgs T;
			memset(&T, 0, sizeof(T));
			T.p1 = d_pubs + off * plen;
			T.p2 = T.p1;
			T.out = S[SG_Y];   // untouched by op 2
			T.status = S[SG_STY];
			T.n = m;
			T.clen = (uint32_t)cl;
			T.op = 2;
			T.slot = cv->slot;
			HIPCHK(ecamd_launch_ptf(cv->nw, T, s));
			H.keys = d_pubs + off * plen;
		} else if (bip) {
			if (smul_dev_locked(ctx, cv, m, d_privs + off * ql, (uint32_t)ql, nullptr, S[SG_Y], S[SG_STY], s)) {   // Y = [x]G
				return -1;
			}
			H.keys = S[SG_Y];
		}
		H.kst = bip ? S[SG_STY] : nullptr;
		H.privs = d_privs + off * ql;
		H.nonces = d_nonces + off * ql;
		H.slots = S[ST_SLOTS];
		H.flags = S[ST_FLAGS];
		H.W = S[SG_KG];
		H.stW = S[SG_STKG];
		H.dg = S[ST_DIGESTS];
		H.out = d_sigs + (size_t)off * siglen;
		H.status = d_status + off;
		HIPCHK(hipMemcpyAsync(S[ST_SLOTS], d_in + (size_t)off * stride, (size_t)m * stride, hipMemcpyDeviceToDevice, s));
		HIPCHK(ecamd_launch_schnorr_item_fill(H, s));
		HIPCHK(commit_hash_launch(hash_type, S[ST_SLOTS], stride, m, S[ST_DIGESTS], hsize, s));
		HIPCHK(ecamd_launch_schnorr_item_sign(cv->qnw, H, s));
		return 0;
	});
}

static int schnorr_item_args_ok(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *a,
				const void *b, const void *c, const void *d, const void *e, uint32_t stride)
{
	if (!ecschnorr::alg_known(alg)) {
		return fail(std::string(fn) + ": alg must be ECAMD_SIG_BIP0340 or ECAMD_SIG_ECFSDSA");
	}
	if (commit_hash_ok(fn, ht, hash_type)) {
		return -1;
	}
	if (!ctx || !cv || cv->ctx != ctx || (n && (!a || !b || !c || !d || !e))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->qslot < 0) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	if ((stride & 3u) || stride > 4096 || stride < 4) {
		return fail(std::string(fn) + ": stride must be a multiple of 4 in 4 .. 4096");
	}
	return 0;
}

static int schnorr_item_fmt_ok(const char *fn, int key_fmt)
{
	if (key_fmt != ECAMD_PT_AFFINE && key_fmt != ECAMD_PT_PROJECTIVE) {
		return fail(std::string(fn) + ": key_fmt must be ECAMD_PT_AFFINE or ECAMD_PT_PROJECTIVE");
	}
	return 0;
}

static int ec_schnorr_verify_batch_dev_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n,
					    const void *d_keys, int key_fmt, const void *d_sigs, const void *d_hash_slots, uint32_t stride,
					    void *d_result, void *hip_stream)
{
	if (schnorr_item_args_ok(fn, ht, ctx, cv, alg, hash_type, n, d_keys, d_sigs, d_hash_slots, d_result, d_result, stride) ||
	    schnorr_item_fmt_ok(fn, key_fmt)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return schnorr_item_verify_dev_locked(ctx, cv, alg, hash_type, n, (const uint8_t *)d_keys, key_fmt, (const uint8_t *)d_sigs,
						      (const uint8_t *)d_hash_slots, stride, (uint8_t *)d_result, s);
	});
}

static int ec_schnorr_verify_batch_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n,
					const uint8_t *keys, int key_fmt, const uint8_t *sigs, const uint8_t *hash_slots, uint32_t stride,
					uint8_t *result)
{
	if (schnorr_item_args_ok(fn, ht, ctx, cv, alg, hash_type, n, keys, sigs, hash_slots, result, result, stride) ||
	    schnorr_item_fmt_ok(fn, key_fmt)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t cl = (size_t)cv->clen, siglen = (size_t)ecschnorr::r_len(alg, cv->clen) + cv->qlen;
	const std::vector<HostArr> arrs = {{keys, nullptr, (key_fmt == ECAMD_PT_PROJECTIVE ? 3 : 2) * cl}, {sigs, nullptr, siglen},
					   {hash_slots, nullptr, stride}, {nullptr, result, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return schnorr_item_verify_dev_locked(ctx, cv, alg, hash_type, m, ip[0], key_fmt, ip[1], ip[2], stride, op[3], s);
	});
}

static int ec_schnorr_sign_batch_dev_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n,
					  const void *d_privs, const void *d_pubkeys_aff, const void *d_nonces, const void *d_hash_slots,
					  uint32_t stride, void *d_sigs, void *d_status, void *hip_stream)
{
	if (schnorr_item_args_ok(fn, ht, ctx, cv, alg, hash_type, n, d_privs, d_nonces, d_hash_slots, d_sigs, d_status, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return schnorr_item_sign_dev_locked(ctx, cv, alg, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_pubkeys_aff,
						    (const uint8_t *)d_nonces, (const uint8_t *)d_hash_slots, stride, (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

static int ec_schnorr_sign_batch_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n,
				      const uint8_t *privs, const uint8_t *pubkeys_aff, const uint8_t *nonces, const uint8_t *hash_slots,
				      uint32_t stride, uint8_t *sigs, uint8_t *status)
{
	if (schnorr_item_args_ok(fn, ht, ctx, cv, alg, hash_type, n, privs, nonces, hash_slots, sigs, status, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen, plen = (size_t)2 * cv->clen;
	const size_t siglen = (size_t)ecschnorr::r_len(alg, cv->clen) + ql;
	const bool with_pub = alg == ECAMD_SIG_BIP0340 && pubkeys_aff != nullptr;   // ECFSDSA ignores it
	std::vector<HostArr> arrs = {{privs, nullptr, ql}, {nonces, nullptr, ql}, {hash_slots, nullptr, stride}, {nullptr, sigs, siglen},
				     {nullptr, status, 1}};
	if (with_pub) {
		arrs.push_back({pubkeys_aff, nullptr, plen});
	}
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return schnorr_item_sign_dev_locked(ctx, cv, alg, hash_type, m, ip[0], with_pub ? ip[5] : nullptr, ip[1], ip[2], stride, op[3], op[4], s);
	});
}

// ------------------------------------------------------------------------------------------
// DBIGN and BIP0340 with the nonce derived ON THE DEVICE (include/libecc_amd.h: ec_dbign_nonce_batch, ec_dbign_sign_batch,
// ec_bip0340_nonce_batch, ec_bip0340_sign_batch): the two generators of ecamd_detnonce.hip in front of the signing cores above.
// Per chunk of at most max_chunk items
//   DBIGN    k_sha2_slots / k_belt_slots (hash_type != 0), k_dbign_nonce into SG_NONCES (the table scanned in secret-scalar mode),
//            bign_sign_dev_locked on the chunk (it hashes the chunk's messages again for its own frame: a compression or two per item)
//   BIP0340  Y = [x]G into SG_Y (or the on-curve test of the caller's keys), k_bip0340_nonce into SG_NONCES,
//            schnorr_item_sign_dev_locked on the chunk with Y as its supplied key (so [x]G is computed once)
// Every slot the cores size is sized here first, for the whole chunk, so no buffer moves between the generator and the core.
// SG_NONCES is secret: ensure() wipes what it frees, ecamd_ctx_wipe_scratch the rest.  Only enqueues.
// ------------------------------------------------------------------------------------------
static const uint32_t h_sha256_k[64] = {ECAMD_SHA256_K};
static const uint64_t h_sha512_k[80] = {ECAMD_SHA512_K};

static int det_order_ok(const char *fn, const ecamd_curve *cv)
{
	if (cv->qslot < 0 || big_bitlen(cv->q) < 2 || cv->q.size() > 17 || cv->qlen > ecrfc::MAX_QLEN ||
	    (uint32_t)cv->qlen != ((uint32_t)cv->qbits + 7) / 8 || cv->clen > ecbip::MAX_CLEN) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	return 0;
}

static int dbign_nonce_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_privs, const uint8_t *d_digests, uint32_t hlen,
				  const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, uint8_t *d_nonces, uint8_t *d_status,
				  hipStream_t s)
{
	EcamdDbignNonceArgs D;
	memset(&D, 0, sizeof(D));
	D.privs = d_privs;
	D.digests = d_digests;
	D.nonces = d_nonces;
	D.status = d_status;
	D.n = n;
	D.qlen = (uint32_t)cv->qlen;
	D.qbits = (uint32_t)cv->qbits;
	D.hlen = hlen;
	D.oid_len = oid_len;
	D.t_len = t_len;
	D.scan = ctx->secret_scalars ? 1 : 0;
	for (int w = 0; w < 17; w++) {
		D.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
	}
	if (oid_len) {
		memcpy(D.oid, oid, oid_len);
	}
	if (t_len) {
		memcpy(D.t, t, t_len);
	}
	HIPCHK(ecamd_launch_dbign_nonce(D, s));
	return 0;
}

static int dbign_common_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, const uint8_t *oid, uint32_t oid_len, const uint8_t *t,
			   uint32_t t_len)
{
	if (oid_len > (uint32_t)ecdbign::MAX_OID || (oid_len && !oid)) {
		return fail(std::string(fn) + ": oid_len must be 0 .. 64, and oid non-NULL when it is not 0");
	}
	if (t_len > (uint32_t)ecdbign::MAX_T || (t_len && !t)) {
		return fail(std::string(fn) + ": t_len must be 0 .. 64, and t non-NULL when it is not 0");
	}
	if (!ctx || !cv || cv->ctx != ctx) {
		return fail(std::string(fn) + ": bad argument");
	}
	return det_order_ok(fn, cv);
}

static int dbign_nonce_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *a, const void *b, uint32_t digest_len,
			       const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, const void *c, const void *d)
{
	if (digest_len < 1 || digest_len > (uint32_t)ecdbign::MAX_DIGEST) {
		return fail(std::string(fn) + ": digest_len must be 1 .. 128");
	}
	if (dbign_common_ok(fn, ctx, cv, oid, oid_len, t, t_len)) {
		return -1;
	}
	if (n && (!a || !b || !c || !d)) {
		return fail(std::string(fn) + ": bad argument");
	}
	return 0;
}

extern "C" int ec_dbign_nonce_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *d_privs, const void *d_digests,
					uint32_t digest_len, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, void *d_nonces,
					void *d_status, void *hip_stream)
{
	if (dbign_nonce_args_ok("ec_dbign_nonce_batch_dev", ctx, cv, n, d_privs, d_digests, digest_len, oid, oid_len, t, t_len, d_nonces, d_status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return dbign_nonce_dev_locked(ctx, cv, n, (const uint8_t *)d_privs, (const uint8_t *)d_digests, digest_len, oid, oid_len, t, t_len,
					      (uint8_t *)d_nonces, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_dbign_nonce_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *privs, const uint8_t *digests,
				    uint32_t digest_len, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, uint8_t *nonces,
				    uint8_t *status)
{
	if (dbign_nonce_args_ok("ec_dbign_nonce_batch", ctx, cv, n, privs, digests, digest_len, oid, oid_len, t, t_len, nonces, status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {digests, nullptr, digest_len}, {nullptr, nonces, ql}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return dbign_nonce_dev_locked(ctx, cv, m, ip[0], ip[1], digest_len, oid, oid_len, t, t_len, op[2], op[3], s);
	});
}

static int dbign_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_privs, const uint8_t *d_in,
				 uint32_t stride, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, uint8_t *d_sigs,
				 uint8_t *d_status, hipStream_t s)
{
	const size_t plen = (size_t)2 * cv->clen, ql = (size_t)cv->qlen, siglen = (size_t)ecbign::sig_len(cv->qlen);
	const uint32_t chunk = chunk_items(ctx, n);
	EcamdBignArgs B;
	bign_args(B, cv, hash_type, stride, oid, oid_len, chunk);
	if (stage_need(ctx, {{SG_NONCES, (size_t)chunk * ql}, {SG_KG, chunk * plen}, {SG_STKG, chunk}, {ST_SLOTS, (size_t)chunk * B.bstride},
			     {ST_DIGESTS, hash_type ? (size_t)chunk * B.hsize : 0}, {ST_BELT, (size_t)chunk * ecbign::DIGEST_BT}})) {
		return -1;
	}
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *in = d_in + (size_t)off * stride;
		B.n = m;
		if (bign_message_digests(ctx, hash_type, m, in, stride, B, s)) {
			return -1;
		}
		// (the generator's status lands in the caller's status bytes and is replaced by the signing core's: a zero nonce is status 1 there)
		if (dbign_nonce_dev_locked(ctx, cv, m, d_privs + off * ql, B.dg, B.hsize, oid, oid_len, t, t_len, ctx->stage[SG_NONCES], d_status + off, s) ||
		    bign_sign_dev_locked(ctx, cv, hash_type, m, d_privs + off * ql, ctx->stage[SG_NONCES], in, stride, oid, oid_len,
					 d_sigs + (size_t)off * siglen, d_status + off, s)) {
			return -1;
		}
		return 0;
	});
}

static int dbign_sign_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *a, const void *b,
			      uint32_t stride, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, const void *c, const void *d)
{
	if (bign_args_ok(fn, ctx, cv, ECAMD_SIG_DBIGN, hash_type, n, a, b, b, c, d, stride, oid, oid_len)) {
		return -1;
	}
	return dbign_common_ok(fn, ctx, cv, oid, oid_len, t, t_len);
}

extern "C" int ec_dbign_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs, const void *d_inputs,
				       uint32_t stride, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, void *d_sigs,
				       void *d_status, void *hip_stream)
{
	if (dbign_sign_args_ok("ec_dbign_sign_batch_dev", ctx, cv, hash_type, n, d_privs, d_inputs, stride, oid, oid_len, t, t_len, d_sigs, d_status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return dbign_sign_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_inputs, stride, oid, oid_len, t, t_len,
					     (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_dbign_sign_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *inputs,
				   uint32_t stride, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, uint8_t *sigs,
				   uint8_t *status)
{
	if (dbign_sign_args_ok("ec_dbign_sign_batch", ctx, cv, hash_type, n, privs, inputs, stride, oid, oid_len, t, t_len, sigs, status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {inputs, nullptr, stride}, {nullptr, sigs, (size_t)ecbign::sig_len(cv->qlen)},
					   {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return dbign_sign_dev_locked(ctx, cv, hash_type, m, ip[0], ip[1], stride, oid, oid_len, t, t_len, op[2], op[3], s);
	});
}

// the two tag hashes of the call's hash, as its words
template <int ALG, typename KT> static void bip0340_tags_of(EcamdBip0340NonceArgs &N, KT Kt)
{
	typename ecrfc::Alg<ALG>::W w[8];
	ecbip::tag_hash<ALG>("BIP0340/aux", 11, w, Kt);
	for (int t = 0; t < 8; t++) {
		N.tag_aux[t] = (uint64_t)w[t];
	}
	ecbip::tag_hash<ALG>("BIP0340/nonce", 13, w, Kt);
	for (int t = 0; t < 8; t++) {
		N.tag_nonce[t] = (uint64_t)w[t];
	}
}

static void bip0340_nonce_args(EcamdBip0340NonceArgs &N, const ecamd_curve *cv, int hash_type, uint32_t stride)
{
	memset(&N, 0, sizeof(N));
	N.qlen = (uint32_t)cv->qlen;
	N.qbits = (uint32_t)cv->qbits;
	N.clen = (uint32_t)cv->clen;
	N.stride = stride;
	for (int w = 0; w < 17; w++) {
		N.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
	}
	switch (hash_type) {
	case 1: bip0340_tags_of<224>(N, h_sha256_k); break;
	case 2: bip0340_tags_of<256>(N, h_sha256_k); break;
	case 3: bip0340_tags_of<384>(N, h_sha512_k); break;
	default: bip0340_tags_of<512>(N, h_sha512_k); break;
	}
}

// ---- the hashes k_bip0340_nonce does not have: the hash trait of ecamd_hmac.h, on the host for the two tag hashes of a call ----
static const uint64_t h_keccak_rc[24] = {ECAMD_KECCAK_RC};
static const uint64_t h_bash_rc[24] = {ECAMD_BASH_RC};
static const uint8_t h_sb_pi[256] = {ECAMD_STREEBOG_PI};
static const uint64_t h_sb_a[64] = {ECAMD_STREEBOG_A};
static const uint64_t h_sb_c[96] = {ECAMD_STREEBOG_C};
static uint64_t h_sb_T[ecsb::TABLE_WORDS];   // Streebog's combined table, built on first use

// what echm::Hash<ID>::hash reads its constants through
struct HostHashEnv {
	const uint32_t *k256;
	const uint64_t *k512, *keccak_rc, *bash_rc, *sb_T, *sb_C;
	void tick() const {}
};

static HostHashEnv host_hash_env()
{
	static std::once_flag once;
	std::call_once(once, [] {
		for (uint32_t e = 0; e < (uint32_t)ecsb::TABLE_WORDS; e++) {
			h_sb_T[e] = ecsb::table_entry(h_sb_pi, h_sb_a, e >> 8, e & 255u);
		}
	});
	return HostHashEnv{h_sha256_k, h_sha512_k, h_keccak_rc, h_bash_rc, h_sb_T, h_sb_c};
}

static void bip0340_nonce_ht_args(EcamdBip0340NonceHtArgs &N, const ecamd_curve *cv, int hash_type, uint32_t stride)
{
	memset(&N, 0, sizeof(N));
	N.qlen = (uint32_t)cv->qlen;
	N.qbits = (uint32_t)cv->qbits;
	N.clen = (uint32_t)cv->clen;
	N.stride = stride;
	for (int w = 0; w < 17; w++) {
		N.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
	}
	const HostHashEnv env = host_hash_env();
	switch (hash_type) {
#define BIP_TAGS(ID) \
	case ID: \
		ecbipht::tag_hash<echm::Hash<ID>>(env, "BIP0340/aux", 11, N.tag_aux); \
		ecbipht::tag_hash<echm::Hash<ID>>(env, "BIP0340/nonce", 13, N.tag_nonce); \
		break;
		ECHM_FOR_EACH_HASH(BIP_TAGS)
#undef BIP_TAGS
	default: break;
	}
}

// Y of one chunk: [x]G into SG_Y, or the caller's keys with their on-curve test; either way SG_STY holds the status.  *keys: where Y lies.
static int bip0340_keys_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t m, const uint8_t *d_privs, const uint8_t *d_pubs, const uint8_t **keys,
			    hipStream_t s)
{
	uint8_t **S = ctx->stage;
	if (d_pubs) {
		EcamdPtfArgs T;
		memset(&T, 0, sizeof(T));
		T.p1 = d_pubs;
		T.p2 = d_pubs;
		T.out = S[SG_Y];   // untouched by op 2
		T.status = S[SG_STY];
		T.n = m;
		T.clen = (uint32_t)cv->clen;
		T.op = 2;
		T.slot = cv->slot;
		HIPCHK(ecamd_launch_ptf(cv->nw, T, s));
		*keys = d_pubs;
		return 0;
	}
	*keys = S[SG_Y];
	return smul_dev_locked(ctx, cv, m, d_privs, (uint32_t)cv->qlen, nullptr, S[SG_Y], S[SG_STY], s);
}

// sign = false: the nonces go to d_out (n x qlen); true: into SG_NONCES, and the signatures (n x (clen + qlen)) to d_out
static int bip0340_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_privs, const uint8_t *d_pubs,
			      const uint8_t *d_aux, const uint8_t *d_in, uint32_t stride, uint8_t *d_out, uint8_t *d_status, bool sign, hipStream_t s)
{
	const size_t cl = (size_t)cv->clen, plen = 2 * cl, ql = (size_t)cv->qlen, siglen = cl + ql;
	const uint32_t hsize = commit_hsize(hash_type);
	if (sign && schnorr_item_no_room(cv, ECAMD_SIG_BIP0340, hsize, stride)) {
		HIPCHK(hipMemsetAsync(d_out, 0, n * siglen, s));
		HIPCHK(hipMemsetAsync(d_status, 1, n, s));
		return 0;
	}
	const uint32_t chunk = chunk_items(ctx, n);
	if (stage_need(ctx, {{SG_Y, chunk * plen}, {SG_STY, chunk}}) ||
	    (sign && stage_need(ctx, {{SG_NONCES, (size_t)chunk * ql}, {SG_KG, chunk * plen}, {SG_STKG, chunk}, {ST_FLAGS, chunk},
				      {ST_SLOTS, (size_t)chunk * stride}, {ST_DIGESTS, (size_t)chunk * hsize}}))) {
		return -1;
	}
	// 1 .. 4: k_bip0340_nonce, whichever name was called; the others: k_bip0340_nonce_ht<ID>
	const bool old_hash = hash_type >= 1 && hash_type <= 4;
	EcamdBip0340NonceArgs N;
	EcamdBip0340NonceHtArgs T;
	if (old_hash) {
		bip0340_nonce_args(N, cv, hash_type, stride);
	} else {
		bip0340_nonce_ht_args(T, cv, hash_type, stride);
	}
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *in = d_in + (size_t)off * stride, *privs = d_privs + off * ql, *keys = nullptr;
		uint8_t *nonces = sign ? ctx->stage[SG_NONCES] : d_out + off * ql;
		if (bip0340_keys_dev(ctx, cv, m, privs, d_pubs ? d_pubs + off * plen : nullptr, &keys, s)) {
			return -1;
		}
		// the status: when signing it is replaced by the core's, where a zero nonce is status 1
		if (old_hash) {
			N.n = m;
			N.privs = privs;
			N.keys = keys;
			N.kst = ctx->stage[SG_STY];
			N.aux = d_aux + off * ql;
			N.slots = in;
			N.nonces = nonces;
			N.status = d_status + off;
			HIPCHK(ecamd_launch_bip0340_nonce(hash_type, N, s));
		} else {
			T.n = m;
			T.privs = privs;
			T.keys = keys;
			T.kst = ctx->stage[SG_STY];
			T.aux = d_aux + off * ql;
			T.slots = in;
			T.nonces = nonces;
			T.status = d_status + off;
			HIPCHK(ecamd_launch_bip0340_nonce_ht(hash_type, T, s));
		}
		// the core takes Y as a supplied key ([x]G is computed once): derived here, it fails the core's on-curve test only as the point at infinity
		if (sign && schnorr_item_sign_dev_locked(ctx, cv, ECAMD_SIG_BIP0340, hash_type, m, privs, keys, nonces, in, stride,
							 d_out + (size_t)off * siglen, d_status + off, s)) {
			return -1;
		}
		return 0;
	});
}

static int bip0340_args_ok(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *privs, const void *aux,
			   const void *slots, const void *out, const void *status, uint32_t stride)
{
	if (schnorr_item_args_ok(fn, ht, ctx, cv, ECAMD_SIG_BIP0340, hash_type, n, privs, aux, slots, out, status, stride)) {
		return -1;
	}
	// the nonce hash absorbs t = d ^ mask: Streebog would look its table up by octets of it
	if (ctx->secret_scalars && (hash_type == 13 || hash_type == 14)) {
		return fail(std::string(fn) + ": Streebog (hash_type 13, 14) looks its table up by octets that depend on the secret: refused in secret-scalar mode");
	}
	return det_order_ok(fn, cv);
}

static int ec_bip0340_nonce_batch_dev_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n,
					   const void *d_privs, const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots,
					   uint32_t stride, void *d_nonces, void *d_status, void *hip_stream)
{
	if (bip0340_args_ok(fn, ht, ctx, cv, hash_type, n, d_privs, d_aux, d_hash_slots, d_nonces, d_status, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return bip0340_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_pubkeys_aff, (const uint8_t *)d_aux,
					  (const uint8_t *)d_hash_slots, stride, (uint8_t *)d_nonces, (uint8_t *)d_status, false, s);
	});
}

static int ec_bip0340_sign_batch_dev_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n,
					  const void *d_privs, const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots,
					  uint32_t stride, void *d_sigs, void *d_status, void *hip_stream)
{
	if (bip0340_args_ok(fn, ht, ctx, cv, hash_type, n, d_privs, d_aux, d_hash_slots, d_sigs, d_status, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return bip0340_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_pubkeys_aff, (const uint8_t *)d_aux,
					  (const uint8_t *)d_hash_slots, stride, (uint8_t *)d_sigs, (uint8_t *)d_status, true, s);
	});
}

static int bip0340_host(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *pubkeys_aff,
			const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *out, size_t outlen, uint8_t *status, bool sign)
{
	const size_t ql = (size_t)cv->qlen, plen = (size_t)2 * cv->clen;
	std::vector<HostArr> arrs = {{privs, nullptr, ql}, {aux, nullptr, ql}, {hash_slots, nullptr, stride}, {nullptr, out, outlen}, {nullptr, status, 1}};
	if (pubkeys_aff) {
		arrs.push_back({pubkeys_aff, nullptr, plen});
	}
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return bip0340_dev_locked(ctx, cv, hash_type, m, ip[0], pubkeys_aff ? ip[5] : nullptr, ip[1], ip[2], stride, op[3], op[4], sign, s);
	});
}

static int ec_bip0340_nonce_batch_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n,
				       const uint8_t *privs, const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots,
				       uint32_t stride, uint8_t *nonces, uint8_t *status)
{
	if (bip0340_args_ok(fn, ht, ctx, cv, hash_type, n, privs, aux, hash_slots, nonces, status, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return bip0340_host(ctx, cv, hash_type, n, privs, pubkeys_aff, aux, hash_slots, stride, nonces, (size_t)cv->qlen, status, false);
}

static int ec_bip0340_sign_batch_impl(const char *fn, bool ht, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs,
				      const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
				      uint8_t *status)
{
	if (bip0340_args_ok(fn, ht, ctx, cv, hash_type, n, privs, aux, hash_slots, sigs, status, stride)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return bip0340_host(ctx, cv, hash_type, n, privs, pubkeys_aff, aux, hash_slots, stride, sigs, (size_t)cv->clen + cv->qlen, status, true);
}

// The public names of the three families above.  name_batch: hash_type 1 .. 4; name_ht_batch: every hash of ec_digest_slots_batch
// (include/libecc_amd.h).  Each pair shares one implementation.
extern "C" int ec_sig_hashed_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_pubkeys,
					      const void *d_sigs, const void *d_inputs, uint32_t stride, void *d_result, void *hip_stream)
{
	return ec_sig_hashed_verify_batch_dev_impl("ec_sig_hashed_verify_batch_dev", false, ctx, cv, alg, hash_type, n, d_pubkeys, d_sigs, d_inputs,
						   stride, d_result, hip_stream);
}

extern "C" int ec_sig_hashed_verify_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_pubkeys,
						 const void *d_sigs, const void *d_inputs, uint32_t stride, void *d_result, void *hip_stream)
{
	return ec_sig_hashed_verify_batch_dev_impl("ec_sig_hashed_verify_ht_batch_dev", true, ctx, cv, alg, hash_type, n, d_pubkeys, d_sigs, d_inputs,
						   stride, d_result, hip_stream);
}

extern "C" int ec_sig_hashed_verify_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *pubkeys,
					  const uint8_t *sigs, const uint8_t *inputs, uint32_t stride, uint8_t *result)
{
	return ec_sig_hashed_verify_batch_impl("ec_sig_hashed_verify_batch", false, ctx, cv, alg, hash_type, n, pubkeys, sigs, inputs, stride,
					       result);
}

extern "C" int ec_sig_hashed_verify_ht_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *pubkeys,
					     const uint8_t *sigs, const uint8_t *inputs, uint32_t stride, uint8_t *result)
{
	return ec_sig_hashed_verify_batch_impl("ec_sig_hashed_verify_ht_batch", true, ctx, cv, alg, hash_type, n, pubkeys, sigs, inputs, stride,
					       result);
}

extern "C" int ec_sig_hashed_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_privs,
					    const void *d_nonces, const void *d_inputs, uint32_t stride, void *d_sigs, void *d_status,
					    void *hip_stream)
{
	return ec_sig_hashed_sign_batch_dev_impl("ec_sig_hashed_sign_batch_dev", false, ctx, cv, alg, hash_type, n, d_privs, d_nonces, d_inputs,
						 stride, d_sigs, d_status, hip_stream);
}

extern "C" int ec_sig_hashed_sign_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_privs,
					       const void *d_nonces, const void *d_inputs, uint32_t stride, void *d_sigs, void *d_status,
					       void *hip_stream)
{
	return ec_sig_hashed_sign_batch_dev_impl("ec_sig_hashed_sign_ht_batch_dev", true, ctx, cv, alg, hash_type, n, d_privs, d_nonces, d_inputs,
						 stride, d_sigs, d_status, hip_stream);
}

extern "C" int ec_sig_hashed_sign_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *privs,
					const uint8_t *nonces, const uint8_t *inputs, uint32_t stride, uint8_t *sigs, uint8_t *status)
{
	return ec_sig_hashed_sign_batch_impl("ec_sig_hashed_sign_batch", false, ctx, cv, alg, hash_type, n, privs, nonces, inputs, stride, sigs,
					     status);
}

extern "C" int ec_sig_hashed_sign_ht_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *privs,
					   const uint8_t *nonces, const uint8_t *inputs, uint32_t stride, uint8_t *sigs, uint8_t *status)
{
	return ec_sig_hashed_sign_batch_impl("ec_sig_hashed_sign_ht_batch", true, ctx, cv, alg, hash_type, n, privs, nonces, inputs, stride, sigs,
					     status);
}

extern "C" int ec_schnorr_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_keys, int key_fmt,
					   const void *d_sigs, const void *d_hash_slots, uint32_t stride, void *d_result, void *hip_stream)
{
	return ec_schnorr_verify_batch_dev_impl("ec_schnorr_verify_batch_dev", false, ctx, cv, alg, hash_type, n, d_keys, key_fmt, d_sigs,
						d_hash_slots, stride, d_result, hip_stream);
}

extern "C" int ec_schnorr_verify_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_keys,
					      int key_fmt, const void *d_sigs, const void *d_hash_slots, uint32_t stride, void *d_result,
					      void *hip_stream)
{
	return ec_schnorr_verify_batch_dev_impl("ec_schnorr_verify_ht_batch_dev", true, ctx, cv, alg, hash_type, n, d_keys, key_fmt, d_sigs,
						d_hash_slots, stride, d_result, hip_stream);
}

extern "C" int ec_schnorr_verify_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *keys, int key_fmt,
				       const uint8_t *sigs, const uint8_t *hash_slots, uint32_t stride, uint8_t *result)
{
	return ec_schnorr_verify_batch_impl("ec_schnorr_verify_batch", false, ctx, cv, alg, hash_type, n, keys, key_fmt, sigs, hash_slots, stride,
					    result);
}

extern "C" int ec_schnorr_verify_ht_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *keys, int key_fmt,
					  const uint8_t *sigs, const uint8_t *hash_slots, uint32_t stride, uint8_t *result)
{
	return ec_schnorr_verify_batch_impl("ec_schnorr_verify_ht_batch", true, ctx, cv, alg, hash_type, n, keys, key_fmt, sigs, hash_slots, stride,
					    result);
}

extern "C" int ec_schnorr_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_privs,
					 const void *d_pubkeys_aff, const void *d_nonces, const void *d_hash_slots, uint32_t stride, void *d_sigs,
					 void *d_status, void *hip_stream)
{
	return ec_schnorr_sign_batch_dev_impl("ec_schnorr_sign_batch_dev", false, ctx, cv, alg, hash_type, n, d_privs, d_pubkeys_aff, d_nonces,
					      d_hash_slots, stride, d_sigs, d_status, hip_stream);
}

extern "C" int ec_schnorr_sign_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_privs,
					    const void *d_pubkeys_aff, const void *d_nonces, const void *d_hash_slots, uint32_t stride, void *d_sigs,
					    void *d_status, void *hip_stream)
{
	return ec_schnorr_sign_batch_dev_impl("ec_schnorr_sign_ht_batch_dev", true, ctx, cv, alg, hash_type, n, d_privs, d_pubkeys_aff, d_nonces,
					      d_hash_slots, stride, d_sigs, d_status, hip_stream);
}

extern "C" int ec_schnorr_sign_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *privs,
				     const uint8_t *pubkeys_aff, const uint8_t *nonces, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
				     uint8_t *status)
{
	return ec_schnorr_sign_batch_impl("ec_schnorr_sign_batch", false, ctx, cv, alg, hash_type, n, privs, pubkeys_aff, nonces, hash_slots, stride,
					  sigs, status);
}

extern "C" int ec_schnorr_sign_ht_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *privs,
					const uint8_t *pubkeys_aff, const uint8_t *nonces, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
					uint8_t *status)
{
	return ec_schnorr_sign_batch_impl("ec_schnorr_sign_ht_batch", true, ctx, cv, alg, hash_type, n, privs, pubkeys_aff, nonces, hash_slots,
					  stride, sigs, status);
}

extern "C" int ec_bip0340_nonce_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs,
					  const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots, uint32_t stride, void *d_nonces,
					  void *d_status, void *hip_stream)
{
	return ec_bip0340_nonce_batch_dev_impl("ec_bip0340_nonce_batch_dev", false, ctx, cv, hash_type, n, d_privs, d_pubkeys_aff, d_aux,
					       d_hash_slots, stride, d_nonces, d_status, hip_stream);
}

extern "C" int ec_bip0340_nonce_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs,
					     const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots, uint32_t stride, void *d_nonces,
					     void *d_status, void *hip_stream)
{
	return ec_bip0340_nonce_batch_dev_impl("ec_bip0340_nonce_ht_batch_dev", true, ctx, cv, hash_type, n, d_privs, d_pubkeys_aff, d_aux,
					       d_hash_slots, stride, d_nonces, d_status, hip_stream);
}

extern "C" int ec_bip0340_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs,
					 const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots, uint32_t stride, void *d_sigs,
					 void *d_status, void *hip_stream)
{
	return ec_bip0340_sign_batch_dev_impl("ec_bip0340_sign_batch_dev", false, ctx, cv, hash_type, n, d_privs, d_pubkeys_aff, d_aux, d_hash_slots,
					      stride, d_sigs, d_status, hip_stream);
}

extern "C" int ec_bip0340_sign_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs,
					    const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots, uint32_t stride, void *d_sigs,
					    void *d_status, void *hip_stream)
{
	return ec_bip0340_sign_batch_dev_impl("ec_bip0340_sign_ht_batch_dev", true, ctx, cv, hash_type, n, d_privs, d_pubkeys_aff, d_aux,
					      d_hash_slots, stride, d_sigs, d_status, hip_stream);
}

extern "C" int ec_bip0340_nonce_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs,
				      const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *nonces,
				      uint8_t *status)
{
	return ec_bip0340_nonce_batch_impl("ec_bip0340_nonce_batch", false, ctx, cv, hash_type, n, privs, pubkeys_aff, aux, hash_slots, stride,
					   nonces, status);
}

extern "C" int ec_bip0340_nonce_ht_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs,
					 const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *nonces,
					 uint8_t *status)
{
	return ec_bip0340_nonce_batch_impl("ec_bip0340_nonce_ht_batch", true, ctx, cv, hash_type, n, privs, pubkeys_aff, aux, hash_slots, stride,
					   nonces, status);
}

extern "C" int ec_bip0340_sign_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs,
				     const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
				     uint8_t *status)
{
	return ec_bip0340_sign_batch_impl("ec_bip0340_sign_batch", false, ctx, cv, hash_type, n, privs, pubkeys_aff, aux, hash_slots, stride, sigs,
					  status);
}

extern "C" int ec_bip0340_sign_ht_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs,
					const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
					uint8_t *status)
{
	return ec_bip0340_sign_batch_impl("ec_bip0340_sign_ht_batch", true, ctx, cv, hash_type, n, privs, pubkeys_aff, aux, hash_slots, stride, sigs,
					  status);
}

// ------------------------------------------------------------------------------------------
// ECGDSA / ECRDSA / SM2 from messages (include/libecc_amd.h: ec_sig_verify_msg_batch, ec_sig_sign_msg_batch, ec_hash_slots_batch): the
// hashes of ecamd_hash.hip / ecamd_hash2.hip in front of the digest-level cores ecdsa_verify_dev_locked(.., alg) / sig_sign_dev_locked,
// which run unchanged.  Per chunk of at most max_chunk items:
//   (signing, SM2)     Y: the caller's keys through the on-curve test, or [x]G (bip0340_keys_dev: SG_Y, SG_STY)
//   k_sig_msg_bad      SM_BAD: the slot does not fit its stride, is shorter than SM2's blank, or the key did not import
//   (SM2) k_sm2_z      Z from the prefix midstate into SM_Z; a copy of the slots in ST_SLOTS; k_slot_patch puts Z into the blank
//   k_*_slots          the digests into ST_DIGESTS
//   the core           verdicts / signatures and status as for the digest-level call
//   k_reject_where / k_sig_msg_reject_sign   SM_BAD's items: result 1 / status 1 with zero bytes
// Frames: SM_ with ST_SLOTS and ST_DIGESTS around the core's own (ST_ / VP_ / SG_).  Only enqueues.
// ------------------------------------------------------------------------------------------
static int sig_msg_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t stride, const uint8_t *id,
			   uint32_t id_len)
{
	if (sig_alg_ok(fn, alg)) {
		return -1;
	}
	if (ecamd_hash_digest_len(hash_type) == 0) {
		return fail(std::string(fn) + ": hash_type must be 1 .. 4 (SHA-224 / 256 / 384 / 512), 11 (SM3), 13 or 14 (Streebog-256 / -512)");
	}
	if (stride < 4 || (stride & 3u) || stride > 4096) {
		return fail(std::string(fn) + ": stride must be a multiple of 4 in 4 .. 4096");
	}
	if (!ctx || !cv || cv->ctx != ctx) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->qslot < 0) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	if (alg == ECAMD_SIG_SM2) {
		if (ecsm2z::hash_size(hash_type) == 0) {
			return fail(std::string(fn) + ": SM2's Z is computed with SM3 or SHA-2 (hash_type 11 or 1 .. 4)");
		}
		if (id_len > (uint32_t)ecsm2z::MAX_ID) {
			return fail(std::string(fn) + ": id_len must be at most 1024");
		}
		if (id_len && !id) {
			return fail(std::string(fn) + ": id is NULL with a positive id_len");
		}
		if (cv->clen > ecsm2z::MAX_CLEN) {
			return fail(std::string(fn) + ": field not supported");
		}
	}
	return 0;
}

// the prefix of the call's Z (SM2 only; otherwise left alone)
static int sig_msg_prefix(const ecamd_curve *cv, int alg, int hash_type, const uint8_t *id, uint32_t id_len, ecsm2z::Prefix &P)
{
	if (alg != ECAMD_SIG_SM2) {
		return 0;
	}
	uint8_t a[ecsm2z::MAX_CLEN], b[ecsm2z::MAX_CLEN], gx[ecsm2z::MAX_CLEN], gy[ecsm2z::MAX_CLEN];
	big_to_be(a, cv->clen, cv->a);
	big_to_be(b, cv->clen, cv->b);
	big_to_be(gx, cv->clen, cv->gx);
	big_to_be(gy, cv->clen, cv->gy);
	if (ecsm2z::prefix_init(P, hash_type, id, id_len, a, b, gx, gy, (uint32_t)cv->clen, h_sha256_k, h_sha512_k)) {
		return fail("internal: Z prefix");
	}
	return 0;
}

// SM2: Z of the chunk's keys into the blank of a staged copy of its slots; *hin: the slots to hash
static int sig_msg_stage_z(ecamd_ctx *ctx, const ecsm2z::Prefix &P, uint32_t m, const uint8_t *d_keys, uint32_t plen, const uint8_t *d_in,
			   uint32_t stride, uint32_t hl, const uint8_t **hin, hipStream_t s)
{
	uint8_t **S = ctx->stage;
	HIPCHK(ecamd_launch_sm2_z(P, d_keys, plen, S[SM_Z], hl, m, s));
	HIPCHK(hipMemcpyAsync(S[ST_SLOTS], d_in, (size_t)m * stride, hipMemcpyDeviceToDevice, s));   // the caller's array is not modified
	HIPCHK(ecamd_launch_slot_patch(S[ST_SLOTS], stride, 0, S[SM_Z], hl, S[SM_BAD], m, s));
	*hin = S[ST_SLOTS];
	return 0;
}

static int sig_msg_verify_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *d_pub,
				     const uint8_t *d_sig, const uint8_t *d_in, uint32_t stride, const ecsm2z::Prefix &P, uint8_t *d_res, hipStream_t s,
				     const Between *between = nullptr)
{
	const size_t plen = (size_t)2 * cv->clen, sl = (size_t)2 * cv->qlen;
	const uint32_t hl = (uint32_t)ecamd_hash_digest_len(hash_type), blank = alg == ECAMD_SIG_SM2 ? hl : 0u;
	const bool sm2 = alg == ECAMD_SIG_SM2;
	if (stride < 4u + blank) {   // no slot can hold the blank: every item is rejected
		HIPCHK(hipMemsetAsync(d_res, 1, n, s));
		return 0;
	}
	const uint32_t chunk = chunk_items(ctx, n);
	if (stage_need(ctx, {{ST_DIGESTS, (size_t)chunk * hl}, {SM_BAD, chunk}, {ST_SLOTS, sm2 ? (size_t)chunk * stride : 0}, {SM_Z, sm2 ? (size_t)chunk * hl : 0}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *pub = d_pub + (size_t)off * plen, *in = d_in + (size_t)off * stride, *hin = in;
		HIPCHK(ecamd_launch_sig_msg_bad(in, stride, blank, nullptr, S[SM_BAD], m, s));
		if (sm2 && sig_msg_stage_z(ctx, P, m, pub, (uint32_t)plen, in, stride, hl, &hin, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_hash_slots(hash_type, hin, stride, m, S[ST_DIGESTS], hl, s));
		if (ecdsa_verify_dev_locked(ctx, cv, m, pub, d_sig + (size_t)off * sl, S[ST_DIGESTS], hl, d_res + off, s,
					    off + m == n ? between : nullptr, alg)) {
			return -1;
		}
		HIPCHK(ecamd_launch_reject_where(d_res + off, S[SM_BAD], m, s));
		return 0;
	});
}

static int sig_msg_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *d_privs,
				   const uint8_t *d_pubs, const uint8_t *d_nonces, const uint8_t *d_in, uint32_t stride, const ecsm2z::Prefix &P,
				   uint8_t *d_sigs, uint8_t *d_status, hipStream_t s)
{
	const size_t plen = (size_t)2 * cv->clen, ql = (size_t)cv->qlen, sl = 2 * ql;
	const uint32_t hl = (uint32_t)ecamd_hash_digest_len(hash_type), blank = alg == ECAMD_SIG_SM2 ? hl : 0u;
	const bool sm2 = alg == ECAMD_SIG_SM2;
	if (stride < 4u + blank) {
		HIPCHK(hipMemsetAsync(d_sigs, 0, n * sl, s));
		HIPCHK(hipMemsetAsync(d_status, 1, n, s));
		return 0;
	}
	const uint32_t chunk = chunk_items(ctx, n);
	if (stage_need(ctx, {{ST_DIGESTS, (size_t)chunk * hl}, {SM_BAD, chunk}, {ST_SLOTS, sm2 ? (size_t)chunk * stride : 0}, {SM_Z, sm2 ? (size_t)chunk * hl : 0},
			     {SG_Y, sm2 ? chunk * plen : 0}, {SG_STY, sm2 ? chunk : 0}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *in = d_in + (size_t)off * stride, *hin = in, *keys = nullptr;
		// SM2: Y for Z, supplied (with its on-curve test) or [x]G by the fixed-base multiplication in the context's secret-scalar mode
		if (sm2 && bip0340_keys_dev(ctx, cv, m, d_privs + off * ql, d_pubs ? d_pubs + off * plen : nullptr, &keys, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_sig_msg_bad(in, stride, blank, sm2 ? S[SG_STY] : nullptr, S[SM_BAD], m, s));
		if (sm2 && sig_msg_stage_z(ctx, P, m, keys, (uint32_t)plen, in, stride, hl, &hin, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_hash_slots(hash_type, hin, stride, m, S[ST_DIGESTS], hl, s));
		if (sig_sign_dev_locked(ctx, cv, alg, m, d_privs + off * ql, d_nonces + off * ql, S[ST_DIGESTS], hl, d_sigs + off * sl, d_status + off, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_sig_msg_reject_sign(d_sigs + off * sl, (uint32_t)sl, d_status + off, S[SM_BAD], m, s));
		return 0;
	});
}

extern "C" int ec_sig_verify_msg_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_pubkeys,
					   const void *d_sigs, const void *d_msg_slots, uint32_t stride, const uint8_t *id, uint32_t id_len,
					   void *d_result, void *hip_stream)
{
	ecsm2z::Prefix P;
	if (sig_msg_args_ok("ec_sig_verify_msg_batch_dev", ctx, cv, alg, hash_type, stride, id, id_len)) {
		return -1;
	}
	if (n && (!d_pubkeys || !d_sigs || !d_msg_slots || !d_result)) {
		return fail("ec_sig_verify_msg_batch_dev: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (sig_msg_prefix(cv, alg, hash_type, id, id_len, P)) {
		return -1;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return sig_msg_verify_dev_locked(ctx, cv, alg, hash_type, n, (const uint8_t *)d_pubkeys, (const uint8_t *)d_sigs, (const uint8_t *)d_msg_slots,
						 stride, P, (uint8_t *)d_result, s);
	});
}

extern "C" int ec_sig_verify_msg_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *pubkeys,
				       const uint8_t *sigs, const uint8_t *msg_slots, uint32_t stride, const uint8_t *id, uint32_t id_len,
				       uint8_t *result)
{
	ecsm2z::Prefix P;
	if (sig_msg_args_ok("ec_sig_verify_msg_batch", ctx, cv, alg, hash_type, stride, id, id_len)) {
		return -1;
	}
	if (n && (!pubkeys || !sigs || !msg_slots || !result)) {
		return fail("ec_sig_verify_msg_batch: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (sig_msg_prefix(cv, alg, hash_type, id, id_len, P)) {
		return -1;
	}
	const std::vector<HostArr> arrs = {{pubkeys, nullptr, (size_t)2 * cv->clen}, {sigs, nullptr, (size_t)2 * cv->qlen}, {msg_slots, nullptr, stride},
					   {nullptr, result, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &between) {
		return sig_msg_verify_dev_locked(ctx, cv, alg, hash_type, m, ip[0], ip[1], ip[2], stride, P, op[3], s, &between);
	});
}

extern "C" int ec_sig_sign_msg_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const void *d_privs,
					 const void *d_pubkeys, const void *d_nonces, const void *d_msg_slots, uint32_t stride, const uint8_t *id,
					 uint32_t id_len, void *d_sigs, void *d_status, void *hip_stream)
{
	ecsm2z::Prefix P;
	if (sig_msg_args_ok("ec_sig_sign_msg_batch_dev", ctx, cv, alg, hash_type, stride, id, id_len)) {
		return -1;
	}
	if (n && (!d_privs || !d_nonces || !d_msg_slots || !d_sigs || !d_status)) {
		return fail("ec_sig_sign_msg_batch_dev: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (sig_msg_prefix(cv, alg, hash_type, id, id_len, P)) {
		return -1;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return sig_msg_sign_dev_locked(ctx, cv, alg, hash_type, n, (const uint8_t *)d_privs, alg == ECAMD_SIG_SM2 ? (const uint8_t *)d_pubkeys : nullptr,
					       (const uint8_t *)d_nonces, (const uint8_t *)d_msg_slots, stride, P, (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_sig_sign_msg_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, int hash_type, uint32_t n, const uint8_t *privs,
				     const uint8_t *pubkeys, const uint8_t *nonces, const uint8_t *msg_slots, uint32_t stride, const uint8_t *id,
				     uint32_t id_len, uint8_t *sigs, uint8_t *status)
{
	ecsm2z::Prefix P;
	if (sig_msg_args_ok("ec_sig_sign_msg_batch", ctx, cv, alg, hash_type, stride, id, id_len)) {
		return -1;
	}
	if (n && (!privs || !nonces || !msg_slots || !sigs || !status)) {
		return fail("ec_sig_sign_msg_batch: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (sig_msg_prefix(cv, alg, hash_type, id, id_len, P)) {
		return -1;
	}
	const size_t ql = (size_t)cv->qlen;
	const bool with_keys = alg == ECAMD_SIG_SM2 && pubkeys;
	std::vector<HostArr> arrs = {{privs, nullptr, ql}, {nonces, nullptr, ql}, {msg_slots, nullptr, stride}, {nullptr, sigs, 2 * ql}, {nullptr, status, 1}};
	if (with_keys) {
		arrs.push_back({pubkeys, nullptr, (size_t)2 * cv->clen});
	}
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return sig_msg_sign_dev_locked(ctx, cv, alg, hash_type, m, ip[0], with_keys ? ip[5] : nullptr, ip[1], ip[2], stride, P, op[3], op[4], s);
	});
}

static int hash_slots_args_ok(const char *fn, ecamd_ctx *ctx, int hash_type, uint32_t n, const void *slots, uint32_t stride, const void *out)
{
	if (ecamd_hash_digest_len(hash_type) == 0) {
		return fail(std::string(fn) + ": hash_type must be 1 .. 4 (SHA-224 / 256 / 384 / 512), 11 (SM3), 13 or 14 (Streebog-256 / -512)");
	}
	if (stride < 4 || (stride & 3u) || stride > 4096) {
		return fail(std::string(fn) + ": stride must be a multiple of 4 in 4 .. 4096");
	}
	if (!ctx || (n && (!slots || !out))) {
		return fail(std::string(fn) + ": bad argument");
	}
	return 0;
}

static int hash_slots_dev_locked(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *d_slots, uint32_t stride, uint8_t *d_out, hipStream_t s)
{
	const uint32_t hl = (uint32_t)ecamd_hash_digest_len(hash_type);
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		HIPCHK(ecamd_launch_hash_slots(hash_type, d_slots + (size_t)off * stride, stride, m, d_out + (size_t)off * hl, hl, s));
		return 0;
	});
}

extern "C" int ec_hash_slots_batch_dev(ecamd_ctx *ctx, int hash_type, uint32_t n, const void *d_msg_slots, uint32_t stride, void *d_digests,
				       void *hip_stream)
{
	if (hash_slots_args_ok("ec_hash_slots_batch_dev", ctx, hash_type, n, d_msg_slots, stride, d_digests)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return hash_slots_dev_locked(ctx, hash_type, n, (const uint8_t *)d_msg_slots, stride, (uint8_t *)d_digests, s);
	});
}

extern "C" int ec_hash_slots_batch(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *msg_slots, uint32_t stride, uint8_t *digests)
{
	if (hash_slots_args_ok("ec_hash_slots_batch", ctx, hash_type, n, msg_slots, stride, digests)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const std::vector<HostArr> arrs = {{msg_slots, nullptr, stride}, {nullptr, digests, (size_t)ecamd_hash_digest_len(hash_type)}};
	return host_call(ctx, 256, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return hash_slots_dev_locked(ctx, hash_type, m, ip[0], stride, op[1], s);
	});
}

// ec_digest_slots_batch (include/libecc_amd.h): the bare hash over the whole table, ecamd_hash3.hip.  The calls above keep their sets.
static int digest_slots_args_ok(const char *fn, ecamd_ctx *ctx, int hash_type, uint32_t n, const void *slots, uint32_t stride, const void *out)
{
	if (ecamd_digest_len_any(hash_type) == 0) {
		return fail(std::string(fn) + ": hash_type must be 1 .. 11, 13 .. 15 or 17 .. 20 (every fixed-length hash of libecc's table but belt-hash)");
	}
	if (stride < 4 || (stride & 3u) || stride > 4096) {
		return fail(std::string(fn) + ": stride must be a multiple of 4 in 4 .. 4096");
	}
	if (!ctx || (n && (!slots || !out))) {
		return fail(std::string(fn) + ": bad argument");
	}
	return 0;
}

static int digest_slots_dev_locked(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *d_slots, uint32_t stride, uint8_t *d_out, hipStream_t s)
{
	const uint32_t dl = (uint32_t)ecamd_digest_len_any(hash_type);
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		HIPCHK(ecamd_launch_digest_slots(hash_type, d_slots + (size_t)off * stride, stride, m, d_out + (size_t)off * dl, dl, s));
		return 0;
	});
}

extern "C" int ecamd_digest_len(int hash_type)
{
	return ecamd_digest_len_any(hash_type);
}

extern "C" int ec_digest_slots_batch_dev(ecamd_ctx *ctx, int hash_type, uint32_t n, const void *d_msg_slots, uint32_t stride, void *d_digests,
					 void *hip_stream)
{
	if (digest_slots_args_ok("ec_digest_slots_batch_dev", ctx, hash_type, n, d_msg_slots, stride, d_digests)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return digest_slots_dev_locked(ctx, hash_type, n, (const uint8_t *)d_msg_slots, stride, (uint8_t *)d_digests, s);
	});
}

extern "C" int ec_digest_slots_batch(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *msg_slots, uint32_t stride, uint8_t *digests)
{
	if (digest_slots_args_ok("ec_digest_slots_batch", ctx, hash_type, n, msg_slots, stride, digests)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const std::vector<HostArr> arrs = {{msg_slots, nullptr, stride}, {nullptr, digests, (size_t)ecamd_digest_len_any(hash_type)}};
	return host_call(ctx, 256, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return digest_slots_dev_locked(ctx, hash_type, m, ip[0], stride, op[1], s);
	});
}


// ------------------------------------------------------------------------------------------
// HMAC and deterministic ECDSA over the whole hash table (include/libecc_amd.h: ec_hmac_slots_batch, ec_rfc6979_nonce_ht_batch,
// ec_decdsa_sign_ht_batch; ecamd_hmac.hip).  The _ht forms are ec_rfc6979_nonce_batch and ec_decdsa_sign_batch with every hash of
// ec_digest_slots_batch; 1 .. 4 run the kernel of the older names.  Per chunk of at most max_chunk items signing is
//   ecamd_launch_digest_slots   in_is_digest = 0: h1 = H(m) into ST_DIGESTS (a slot that does not fit: zeros)
//   k_rfc6979_nonce[_ht]        k into SG_NONCES (secret: ensure() wipes what it frees, ecamd_ctx_wipe_scratch the rest); a slot whose
//                               length does not fit gets k = 0
//   ecdsa_sign_dev_locked       [k]G as the context's secret-scalar mode says, r, s; k = 0 is status 1 with zero bytes
// Streebog's look-ups are indexed by key-dependent octets: the three calls refuse 13 and 14 in secret-scalar mode.  Only enqueues.
// ------------------------------------------------------------------------------------------
static int ht_hash_ok(const char *fn, const ecamd_ctx *ctx, int hash_type)
{
	if (!ecamd_hmac_served(hash_type)) {
		return fail(std::string(fn) + ": " + HT_SET);
	}
	if (ctx && ctx->secret_scalars && (hash_type == 13 || hash_type == 14)) {
		return fail(std::string(fn) + ": Streebog (hash_type 13, 14) looks its table up by octets that depend on the secret: refused in secret-scalar mode");
	}
	return 0;
}

static int hmac_slots_args_ok(const char *fn, ecamd_ctx *ctx, int hash_type, uint32_t n, const void *keys, uint32_t key_stride, const void *msgs,
			      uint32_t stride, const void *macs)
{
	if (ht_hash_ok(fn, ctx, hash_type)) {
		return -1;
	}
	if (key_stride < 4 || (key_stride & 3u) || key_stride > 4096 || stride < 4 || (stride & 3u) || stride > 4096) {
		return fail(std::string(fn) + ": key_stride and stride must be multiples of 4 in 4 .. 4096");
	}
	if (!ctx || (n && (!keys || !msgs || !macs))) {
		return fail(std::string(fn) + ": bad argument");
	}
	return 0;
}

static int hmac_slots_dev_locked(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *d_keys, uint32_t key_stride, const uint8_t *d_msgs,
				 uint32_t stride, uint8_t *d_macs, hipStream_t s)
{
	const uint32_t dl = (uint32_t)ecamd_digest_len_any(hash_type);
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		HIPCHK(ecamd_launch_hmac_slots(hash_type, d_keys + (size_t)off * key_stride, key_stride, d_msgs + (size_t)off * stride, stride, m,
					       d_macs + (size_t)off * dl, s));
		return 0;
	});
}

extern "C" int ec_hmac_slots_batch_dev(ecamd_ctx *ctx, int hash_type, uint32_t n, const void *d_key_slots, uint32_t key_stride,
				       const void *d_msg_slots, uint32_t stride, void *d_macs, void *hip_stream)
{
	if (hmac_slots_args_ok("ec_hmac_slots_batch_dev", ctx, hash_type, n, d_key_slots, key_stride, d_msg_slots, stride, d_macs)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return hmac_slots_dev_locked(ctx, hash_type, n, (const uint8_t *)d_key_slots, key_stride, (const uint8_t *)d_msg_slots, stride,
					     (uint8_t *)d_macs, s);
	});
}

extern "C" int ec_hmac_slots_batch(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *key_slots, uint32_t key_stride,
				   const uint8_t *msg_slots, uint32_t stride, uint8_t *macs)
{
	if (hmac_slots_args_ok("ec_hmac_slots_batch", ctx, hash_type, n, key_slots, key_stride, msg_slots, stride, macs)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const std::vector<HostArr> arrs = {{key_slots, nullptr, key_stride}, {msg_slots, nullptr, stride},
					   {nullptr, macs, (size_t)ecamd_digest_len_any(hash_type)}};
	return host_call(ctx, 256, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return hmac_slots_dev_locked(ctx, hash_type, m, ip[0], key_stride, ip[1], stride, op[2], s);
	});
}

static int rfc6979_ht_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type)
{
	if (ht_hash_ok(fn, ctx, hash_type)) {
		return -1;
	}
	if (!ctx || !cv || cv->ctx != ctx) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->qslot < 0 || big_bitlen(cv->q) < 2 || cv->q.size() > 17 || cv->qlen > ecrfc::MAX_QLEN ||
	    (uint32_t)cv->qlen != ((uint32_t)cv->qbits + 7) / 8) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	return 0;
}

static int rfc6979_ht_nonce_dev_locked(const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_privs, const uint8_t *d_digests,
				       const uint8_t *d_slots, uint32_t stride, uint8_t *d_nonces, uint8_t *d_status, hipStream_t s)
{
	EcamdRfc6979Args R;
	memset(&R, 0, sizeof(R));
	R.privs = d_privs;
	R.digests = d_digests;
	R.slots = d_slots;
	R.stride = stride;
	R.nonces = d_nonces;
	R.status = d_status;
	R.n = n;
	R.qlen = (uint32_t)cv->qlen;
	R.qbits = (uint32_t)cv->qbits;
	for (int w = 0; w < 17; w++) {
		R.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
	}
	HIPCHK(ecamd_launch_rfc6979_nonce_ht(hash_type, R, s));
	return 0;
}

extern "C" int ec_rfc6979_nonce_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs,
					     const void *d_digests, void *d_nonces, void *d_status, void *hip_stream)
{
	if (rfc6979_ht_args_ok("ec_rfc6979_nonce_ht_batch_dev", ctx, cv, hash_type)) {
		return -1;
	}
	if (n && (!d_privs || !d_digests || !d_nonces || !d_status)) {
		return fail("ec_rfc6979_nonce_ht_batch_dev: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		const size_t ql = (size_t)cv->qlen, dl = (size_t)ecamd_digest_len_any(hash_type);
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return rfc6979_ht_nonce_dev_locked(cv, hash_type, m, (const uint8_t *)d_privs + off * ql, (const uint8_t *)d_digests + off * dl, nullptr, 0,
							   (uint8_t *)d_nonces + off * ql, (uint8_t *)d_status + off, s);
		});
	});
}

extern "C" int ec_rfc6979_nonce_ht_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs,
					 const uint8_t *digests, uint8_t *nonces, uint8_t *status)
{
	if (rfc6979_ht_args_ok("ec_rfc6979_nonce_ht_batch", ctx, cv, hash_type)) {
		return -1;
	}
	if (n && (!privs || !digests || !nonces || !status)) {
		return fail("ec_rfc6979_nonce_ht_batch: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen, dl = (size_t)ecamd_digest_len_any(hash_type);
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {digests, nullptr, dl}, {nullptr, nonces, ql}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return for_chunks(ctx, m, [&](uint32_t off, uint32_t c) -> int {
			return rfc6979_ht_nonce_dev_locked(cv, hash_type, c, ip[0] + off * ql, ip[1] + off * dl, nullptr, 0, op[2] + off * ql, op[3] + off, s);
		});
	});
}

static int decdsa_ht_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_privs, const uint8_t *d_in,
				     uint32_t stride, int in_is_digest, uint8_t *d_sigs, uint8_t *d_status, hipStream_t s)
{
	const size_t ql = (size_t)cv->qlen;
	const uint32_t hlen = (uint32_t)ecamd_digest_len_any(hash_type);
	const size_t chunk = chunk_items(ctx, n);
	if (stage_need(ctx, {{SG_NONCES, chunk * ql}, {ST_DIGESTS, in_is_digest ? 0 : chunk * hlen}})) {
		return -1;
	}
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const uint8_t *in = d_in + (size_t)off * stride, *d_dig = in;
		if (!in_is_digest) {
			HIPCHK(ecamd_launch_digest_slots(hash_type, in, stride, m, ctx->stage[ST_DIGESTS], hlen, s));
			d_dig = ctx->stage[ST_DIGESTS];
		}
		// (the nonce kernel's status lands in the caller's status bytes and is replaced by the signing core's: a zero nonce is status 1 there)
		if (rfc6979_ht_nonce_dev_locked(cv, hash_type, m, d_privs + off * ql, d_dig, in_is_digest ? nullptr : in, stride, ctx->stage[SG_NONCES],
						d_status + off, s)) {
			return -1;
		}
		return ecdsa_sign_dev_locked(ctx, cv, m, d_privs + off * ql, ctx->stage[SG_NONCES], d_dig, hlen, d_sigs + off * 2 * ql, d_status + off, s);
	});
}

static int decdsa_ht_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *a, const void *b,
			     uint32_t stride, int in_is_digest, const void *c, const void *d)
{
	if (rfc6979_ht_args_ok(fn, ctx, cv, hash_type)) {
		return -1;
	}
	if (in_is_digest != 0 && in_is_digest != 1) {
		return fail(std::string(fn) + ": in_is_digest must be 0 or 1");
	}
	if (in_is_digest ? stride != (uint32_t)ecamd_digest_len_any(hash_type) : (stride < 4 || (stride & 3u) || stride > 4096)) {
		return fail(std::string(fn) + ": in_stride must be the digest length (in_is_digest = 1) or a multiple of 4 in 4 .. 4096 (message slots)");
	}
	if (n && (!a || !b || !c || !d)) {
		return fail(std::string(fn) + ": bad argument");
	}
	return 0;
}

extern "C" int ec_decdsa_sign_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs, const void *d_in,
					   uint32_t in_stride, int in_is_digest, void *d_sigs, void *d_status, void *hip_stream)
{
	if (decdsa_ht_args_ok("ec_decdsa_sign_ht_batch_dev", ctx, cv, hash_type, n, d_privs, d_in, in_stride, in_is_digest, d_sigs, d_status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return decdsa_ht_sign_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_in, in_stride, in_is_digest,
						 (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_decdsa_sign_ht_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *in,
				       uint32_t in_stride, int in_is_digest, uint8_t *sigs, uint8_t *status)
{
	if (decdsa_ht_args_ok("ec_decdsa_sign_ht_batch", ctx, cv, hash_type, n, privs, in, in_stride, in_is_digest, sigs, status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {in, nullptr, in_stride}, {nullptr, sigs, 2 * ql}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return decdsa_ht_sign_dev_locked(ctx, cv, hash_type, m, ip[0], ip[1], in_stride, in_is_digest, op[2], op[3], s);
	});
}


// ------------------------------------------------------------------------------------------
// The ragged message array (include/libecc_amd.h: ec_digest_msgs_batch, ec_ecdsa_verify_msgs_batch, ec_decdsa_sign_msgs_batch;
// ecamd_digest_msgs.hip).  k_digest_msgs<ID> validates every item against the array's length itself, so the _dev forms only enqueue:
//   ecamd_launch_digest_msgs    the digests, and 0 / 1 per item
// and the two protocol calls put that launch in front of the cores that exist, per chunk of at most max_chunk items:
//   ec_ecdsa_verify_msgs_*      digests into ST_DIGESTS, status into DM_BAD; ecdsa_verify_dev_locked; k_reject_where: DM_BAD's items are result 1
//   ec_decdsa_sign_msgs_*       the same two; decdsa_ht_sign_dev_locked on the digests; k_sig_msg_reject_sign: status 1 with zero bytes
// The host forms (msgs_host_call) stage PIECES of the array: a run of items whose messages span at most MSGS_CHUNK_BYTES octets and
// that has at most max_chunk items, with offsets rebased to the piece.  The per-item arrays go through ctx->hbuf[0], the piece and its
// offsets through DM_MSGS / DM_OFFS; ecamd_ctx_wipe_scratch covers both.  One piece at a time: copy in, core, copy out, synchronise.
// ------------------------------------------------------------------------------------------
static const uint64_t MSGS_CHUNK_BYTES = 1ull << 28;   // octets of the message array staged per piece (a longer single message: a piece of its own)

// $ECAMD_MSGS_CHUNK_BYTES: a smaller cap (tests, measurements), read per call like $ECAMD_HOST_SCHEDULE
static uint64_t msgs_chunk_bytes()
{
	if (const char *e = getenv("ECAMD_MSGS_CHUNK_BYTES")) {
		const uint64_t v = strtoull(e, nullptr, 10);
		if (v >= 1 && v < MSGS_CHUNK_BYTES) {
			return v;
		}
	}
	return MSGS_CHUNK_BYTES;
}

static int msgs_hash_ok(const char *fn, int hash_type)
{
	if (ecamd_digest_len_any(hash_type) == 0 || !ecamd_hmac_served(hash_type)) {
		return fail(std::string(fn) + ": " + HT_SET);
	}
	return 0;
}

// the launch: items [off, off + m) of an array of msgs_len octets
static int digest_msgs_launch(int hash_type, EcamdDigestMsgsArgs A, uint32_t off, uint32_t m, uint8_t *d_digests, uint8_t *d_status, hipStream_t s)
{
	A.offsets += off;
	if (A.item_prefix_len) {
		A.item_prefixes += (size_t)off * A.item_prefix_stride;
	}
	A.n = m;
	A.digests = d_digests;
	A.status = d_status;
	HIPCHK(ecamd_launch_digest_msgs(hash_type, A, s));
	return 0;
}

static EcamdDigestMsgsArgs digest_msgs_args(const void *d_msgs, uint64_t msgs_len, const void *d_offsets, const uint8_t *call_prefix, uint32_t cpl,
					    const void *d_item_prefixes, uint32_t ipl, uint32_t ips)
{
	EcamdDigestMsgsArgs A;
	memset(&A, 0, sizeof(A));
	A.msgs = (const uint32_t *)d_msgs;
	A.msgs_len = msgs_len;
	A.offsets = (const uint64_t *)d_offsets;
	A.item_prefixes = ipl ? (const uint8_t *)d_item_prefixes : nullptr;
	A.item_prefix_len = ipl;
	A.item_prefix_stride = ipl ? ips : 0;
	A.call_prefix_len = cpl;
	if (cpl) {
		memcpy(A.call_prefix, call_prefix, cpl);
	}
	return A;
}

static int msgs_prefix_ok(const char *fn, uint32_t n, const uint8_t *call_prefix, uint32_t cpl, const void *item_prefixes, uint32_t ipl, uint32_t ips)
{
	if (cpl > 256 || ipl > 256) {
		return fail(std::string(fn) + ": call_prefix_len and item_prefix_len must be at most 256");
	}
	if ((cpl && !call_prefix) || (n && ipl && !item_prefixes)) {
		return fail(std::string(fn) + ": a prefix is NULL with a positive length");
	}
	if (ipl && ips < ipl) {
		return fail(std::string(fn) + ": item_prefix_stride must be at least item_prefix_len");
	}
	return 0;
}

int ecamd_host::msgs_dev_ptr_ok(const char *fn, const void *d_msgs, uint64_t msgs_len, const void *d_offsets)
{
	if (((uintptr_t)d_msgs & 3u) || ((uintptr_t)d_offsets & 7u)) {
		return fail(std::string(fn) + ": d_msgs must be 4-byte aligned and d_offsets 8-byte aligned");
	}
	if (msgs_len && !d_msgs) {
		return fail(std::string(fn) + ": d_msgs is NULL with a positive msgs_len");
	}
	return 0;
}

// (MsgsArr, MsgsCore: ecamd_host_internal.h -- EdDSA's ragged calls in ecamd_host_eddsa.cpp stage their pieces through this too)
int ecamd_host::msgs_host_call(const char *fn, ecamd_ctx *ctx, uint32_t n, const uint8_t *msgs, const uint64_t *offsets, const std::vector<MsgsArr> &arrs,
			  const MsgsCore &core)
{
	const size_t na = arrs.size();
	if (na > 6) {
		return fail("internal: too many host arrays");
	}
	const uint64_t total = offsets[n], cap = msgs_chunk_bytes();
	if (total && !msgs) {
		return fail(std::string(fn) + ": msgs is NULL with a positive offsets[n]");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	std::vector<uint64_t> reb;
	for (uint32_t off = 0; off < n;) {
		// the piece: items are added while the span [lo, hi) of the usable ones (off0 <= off1 <= offsets[n]) stays within the cap
		uint64_t lo = 0, hi = 0;
		bool any = false;
		uint32_t m = 0;
		while (off + m < n && m < ctx->max_chunk) {
			const uint64_t a = offsets[off + m], b = offsets[off + m + 1];
			if (a <= b && b <= total) {
				const uint64_t nlo = any && lo < a ? lo : a, nhi = any && hi > b ? hi : b;
				if (m > 0 && nhi - nlo > cap) {
					break;
				}
				lo = nlo;
				hi = nhi;
				any = true;
			}
			m++;
		}
		// offsets rebased to the piece; a value outside it belongs to unusable items only and stays unusable
		const uint64_t len = hi - lo;
		reb.resize((size_t)m + 1);
		for (uint32_t j = 0; j <= m; j++) {
			const uint64_t v = offsets[off + j];
			reb[j] = (any && v >= lo && v <= hi) ? v - lo : ~0ull;
		}
		if (stage_need(ctx, {{DM_MSGS, (size_t)((len + 3) & ~3ull)}, {DM_OFFS, ((size_t)m + 1) * 8}})) {
			return -1;
		}
		for (size_t k = 0; k < na; k++) {
			if (ensure(&ctx->hbuf[0][k], &ctx->hbuf_bytes[0][k], (size_t)m * arrs[k].stride)) {
				return -1;
			}
		}
		if (len) {
			HIPCHK(hipMemcpyAsync(ctx->stage[DM_MSGS], msgs + lo, (size_t)len, hipMemcpyHostToDevice, s));
		}
		HIPCHK(hipMemcpyAsync(ctx->stage[DM_OFFS], reb.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
		DevIn ip(na, nullptr);
		DevOut op(na, nullptr);
		for (size_t k = 0; k < na; k++) {
			const size_t bytes = (size_t)(m - 1) * arrs[k].stride + arrs[k].len;
			if (arrs[k].in && arrs[k].len) {
				HIPCHK(hipMemcpyAsync(ctx->hbuf[0][k], arrs[k].in + (size_t)off * arrs[k].stride, bytes, hipMemcpyHostToDevice, s));
				ip[k] = ctx->hbuf[0][k];
			}
			op[k] = arrs[k].out ? ctx->hbuf[0][k] : nullptr;
		}
		if (core(m, ctx->stage[DM_MSGS], len, (const uint64_t *)ctx->stage[DM_OFFS], ip, op, s)) {
			(void)hipStreamSynchronize(s);
			return -1;
		}
		for (size_t k = 0; k < na; k++) {
			if (arrs[k].out) {
				HIPCHK(hipMemcpyAsync(arrs[k].out + (size_t)off * arrs[k].stride, ctx->hbuf[0][k], (size_t)m * arrs[k].stride, hipMemcpyDeviceToHost, s));
			}
		}
		HIPCHK(hipStreamSynchronize(s));
		off += m;
	}
	return 0;
}

extern "C" int ec_digest_msgs_batch_dev(ecamd_ctx *ctx, int hash_type, uint32_t n, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
					const uint8_t *call_prefix, uint32_t call_prefix_len, const void *d_item_prefixes, uint32_t item_prefix_len,
					uint32_t item_prefix_stride, void *d_digests, void *d_status, void *hip_stream)
{
	const char *fn = "ec_digest_msgs_batch_dev";
	if (msgs_hash_ok(fn, hash_type) || msgs_prefix_ok(fn, n, call_prefix, call_prefix_len, d_item_prefixes, item_prefix_len, item_prefix_stride)) {
		return -1;
	}
	if (!ctx || (n && (!d_offsets || !d_digests))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (msgs_dev_ptr_ok(fn, d_msgs, msgs_len, d_offsets)) {
		return -1;
	}
	const EcamdDigestMsgsArgs A = digest_msgs_args(d_msgs, msgs_len, d_offsets, call_prefix, call_prefix_len, d_item_prefixes, item_prefix_len, item_prefix_stride);
	const size_t dl = (size_t)ecamd_digest_len_any(hash_type);
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return digest_msgs_launch(hash_type, A, off, m, (uint8_t *)d_digests + off * dl, d_status ? (uint8_t *)d_status + off : nullptr, s);
		});
	});
}

extern "C" int ec_digest_msgs_batch(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *msgs, const uint64_t *offsets, const uint8_t *call_prefix,
				    uint32_t call_prefix_len, const uint8_t *item_prefixes, uint32_t item_prefix_len, uint32_t item_prefix_stride,
				    uint8_t *digests, uint8_t *status)
{
	const char *fn = "ec_digest_msgs_batch";
	if (msgs_hash_ok(fn, hash_type) || msgs_prefix_ok(fn, n, call_prefix, call_prefix_len, item_prefixes, item_prefix_len, item_prefix_stride)) {
		return -1;
	}
	if (!ctx || (n && (!offsets || !digests))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t dl = (size_t)ecamd_digest_len_any(hash_type);
	const std::vector<MsgsArr> arrs = {{item_prefix_len ? item_prefixes : nullptr, nullptr, item_prefix_len ? item_prefix_stride : 0, item_prefix_len},
					   {nullptr, digests, dl, dl}, {nullptr, status, 1, 1}};
	return msgs_host_call(fn, ctx, n, msgs, offsets, arrs,
			      [&](uint32_t m, const uint8_t *d_msgs, uint64_t len, const uint64_t *d_offs, const DevIn &ip, const DevOut &op, hipStream_t s) {
		const EcamdDigestMsgsArgs A = digest_msgs_args(d_msgs, len, d_offs, call_prefix, call_prefix_len, ip[0], item_prefix_len, item_prefix_stride);
		return digest_msgs_launch(hash_type, A, 0, m, op[1], op[2], s);
	});
}

// ---- ECDSA verification and deterministic ECDSA signing from the ragged array ----
static int msgs_curve_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type)
{
	if (msgs_hash_ok(fn, hash_type)) {
		return -1;
	}
	if (!ctx || !cv || cv->ctx != ctx) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->qslot < 0) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	return 0;
}

static int ecdsa_verify_msgs_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig,
					const uint8_t *d_msgs, uint64_t msgs_len, const uint64_t *d_offsets, uint8_t *d_res, hipStream_t s)
{
	const size_t plen = (size_t)2 * cv->clen, sl = (size_t)2 * cv->qlen;
	const uint32_t hl = (uint32_t)ecamd_digest_len_any(hash_type), chunk = chunk_items(ctx, n);
	if (stage_need(ctx, {{ST_DIGESTS, (size_t)chunk * hl}, {DM_BAD, chunk}})) {
		return -1;
	}
	const EcamdDigestMsgsArgs A = digest_msgs_args(d_msgs, msgs_len, d_offsets, nullptr, 0, nullptr, 0, 0);
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		if (digest_msgs_launch(hash_type, A, off, m, S[ST_DIGESTS], S[DM_BAD], s) ||
		    ecdsa_verify_dev_locked(ctx, cv, m, d_pub + off * plen, d_sig + off * sl, S[ST_DIGESTS], hl, d_res + off, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_reject_where(d_res + off, S[DM_BAD], m, s));
		return 0;
	});
}

extern "C" int ec_ecdsa_verify_msgs_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_pubkeys_aff,
					      const void *d_sigs, const void *d_msgs, uint64_t msgs_len, const void *d_offsets, void *d_result,
					      void *hip_stream)
{
	const char *fn = "ec_ecdsa_verify_msgs_batch_dev";
	if (msgs_curve_ok(fn, ctx, cv, hash_type)) {
		return -1;
	}
	if (n && (!d_pubkeys_aff || !d_sigs || !d_offsets || !d_result)) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (msgs_dev_ptr_ok(fn, d_msgs, msgs_len, d_offsets)) {
		return -1;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return ecdsa_verify_msgs_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_pubkeys_aff, (const uint8_t *)d_sigs, (const uint8_t *)d_msgs, msgs_len,
						    (const uint64_t *)d_offsets, (uint8_t *)d_result, s);
	});
}

extern "C" int ec_ecdsa_verify_msgs_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *pubkeys_aff, const uint8_t *sigs,
					  const uint8_t *msgs, const uint64_t *offsets, uint8_t *result)
{
	const char *fn = "ec_ecdsa_verify_msgs_batch";
	if (msgs_curve_ok(fn, ctx, cv, hash_type)) {
		return -1;
	}
	if (n && (!pubkeys_aff || !sigs || !offsets || !result)) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t plen = (size_t)2 * cv->clen, sl = (size_t)2 * cv->qlen;
	const std::vector<MsgsArr> arrs = {{pubkeys_aff, nullptr, plen, plen}, {sigs, nullptr, sl, sl}, {nullptr, result, 1, 1}};
	return msgs_host_call(fn, ctx, n, msgs, offsets, arrs,
			      [&](uint32_t m, const uint8_t *d_msgs, uint64_t len, const uint64_t *d_offs, const DevIn &ip, const DevOut &op, hipStream_t s) {
		return ecdsa_verify_msgs_dev_locked(ctx, cv, hash_type, m, ip[0], ip[1], d_msgs, len, d_offs, op[2], s);
	});
}

static int decdsa_sign_msgs_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_privs, const uint8_t *d_msgs,
				       uint64_t msgs_len, const uint64_t *d_offsets, uint8_t *d_sigs, uint8_t *d_status, hipStream_t s)
{
	const size_t ql = (size_t)cv->qlen, sl = 2 * ql;
	const uint32_t hl = (uint32_t)ecamd_digest_len_any(hash_type), chunk = chunk_items(ctx, n);
	if (stage_need(ctx, {{ST_DIGESTS, (size_t)chunk * hl}, {DM_BAD, chunk}})) {
		return -1;
	}
	const EcamdDigestMsgsArgs A = digest_msgs_args(d_msgs, msgs_len, d_offsets, nullptr, 0, nullptr, 0, 0);
	uint8_t **S = ctx->stage;
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		// (an unusable item's digest is zero: it is signed like any other and then replaced)
		if (digest_msgs_launch(hash_type, A, off, m, S[ST_DIGESTS], S[DM_BAD], s) ||
		    decdsa_ht_sign_dev_locked(ctx, cv, hash_type, m, d_privs + off * ql, S[ST_DIGESTS], hl, 1, d_sigs + off * sl, d_status + off, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_sig_msg_reject_sign(d_sigs + off * sl, (uint32_t)sl, d_status + off, S[DM_BAD], m, s));
		return 0;
	});
}

extern "C" int ec_decdsa_sign_msgs_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs, const void *d_msgs,
					     uint64_t msgs_len, const void *d_offsets, void *d_sigs, void *d_status, void *hip_stream)
{
	const char *fn = "ec_decdsa_sign_msgs_batch_dev";
	if (rfc6979_ht_args_ok(fn, ctx, cv, hash_type)) {
		return -1;
	}
	if (n && (!d_privs || !d_offsets || !d_sigs || !d_status)) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (msgs_dev_ptr_ok(fn, d_msgs, msgs_len, d_offsets)) {
		return -1;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return decdsa_sign_msgs_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_msgs, msgs_len, (const uint64_t *)d_offsets,
						   (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_decdsa_sign_msgs_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *msgs,
					 const uint64_t *offsets, uint8_t *sigs, uint8_t *status)
{
	const char *fn = "ec_decdsa_sign_msgs_batch";
	if (rfc6979_ht_args_ok(fn, ctx, cv, hash_type)) {
		return -1;
	}
	if (n && (!privs || !offsets || !sigs || !status)) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<MsgsArr> arrs = {{privs, nullptr, ql, ql}, {nullptr, sigs, 2 * ql, 2 * ql}, {nullptr, status, 1, 1}};
	return msgs_host_call(fn, ctx, n, msgs, offsets, arrs,
			      [&](uint32_t m, const uint8_t *d_msgs, uint64_t len, const uint64_t *d_offs, const DevIn &ip, const DevOut &op, hipStream_t s) {
		return decdsa_sign_msgs_dev_locked(ctx, cv, hash_type, m, ip[0], d_msgs, len, d_offs, op[1], op[2], s);
	});
}
