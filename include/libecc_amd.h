/*
 * include/libecc_amd.h -- C ABI of the MI355X batched short-Weierstrass scalar-multiplication
 * engine.  This is the drop-in boundary for libecc's hot path: plain C, plain pointers and
 * sizes, libecc's wire formats (big-endian octet strings) and libecc's 0 / -1 return
 * convention (utils/utils.h:80,137-143).  File:line references are relative to
 * /root/reference/src.
 *
 * libecc performs ONE scalar multiplication per call (curves/prj_pt.h:61); a GPU only pays off
 * on batches, so each entry point below is the batch form of the libecc call chain it
 * replaces, with a per-item status byte mirroring the scalar API's 0 / -1:
 *
 *   ECAMD_OK  (0)  the libecc chain would have returned 0 and produced these bytes
 *   ECAMD_ERR (1)  some call of the chain would have returned -1 (coordinate >= p, point not
 *                  on the curve, r/s out of range, ...); the output bytes are zero
 *   ECAMD_INF (2)  only for point results: the result is the point at infinity (prj_pt_mul
 *                  returns 0 with Z = 0; prj_pt_unique / prj_pt_to_aff then return -1,
 *                  curves/prj_pt.c:246-247); the output bytes are zero
 *
 * Every function returns 0 on success and -1 on failure of the call itself (bad argument, no
 * device, HIP error); ecamd_last_error() then describes it.  There is NO CPU fallback: without
 * a gfx950 device ecamd_ctx_create() fails.
 *
 * Threads: a context serialises its calls with a mutex; use one context per thread (or per GPU) for
 * concurrency -- any number of contexts may share a device (the __constant__ curve slots are managed per
 * device, not per context).  Streams: a context owns ONE set of scratch buffers, so its calls execute one
 * after the other on the device even when they are enqueued on different streams (each call makes its stream
 * wait for the previous call's last kernel); use two contexts for two concurrent streams.  Memory: scratch grows with the largest batch seen (about 3 KB per item of a chunk of
 * <= 2^20 items for 256-bit curves, 7 KB for 521 bits); a curve handle that has served a fixed-base batch of >= 4096 items keeps a table of
 * multiples of the generator in HBM (42 MB for 256-bit curves, 183 MB for 521 bits).
 *
 * Environment (read when a context / curve handle is created; for measurements and fallbacks):
 *   ECAMD_HOST_CHUNK=<items>      chunk size of the host-pointer entry points (default 2^19)
 *   ECAMD_HOST_RAMP_MIN=<items>   a call of several chunks starts with a short one, max(chunk / 8, this) items (default 2^16); ECAMD_NO_HOST_RAMP: equal chunks
 *   ECAMD_COMB_MIN_BATCH=<items>  smallest fixed-base batch that builds / uses the generator table (default 4096)
 *   ECAMD_MSM_MIN=<items>, ECAMD_MSM_K=<items per lane>   initial values of ecamd_ctx_set_eddsa_msm (default 2^17, chosen from the batch size)
 *   ECAMD_NO_COMB, ECAMD_NO_FAST_PATH, ECAMD_NO_P25519, ECAMD_NO_K256, ECAMD_NO_P448, ECAMD_NO_MPINV1, ECAMD_NO_ISO, ECAMD_NO_X25519_LADDER,
 *   ECAMD_NO_EDWARDS_SMUL, ECAMD_NO_ED_LATE_MAP, ECAMD_NO_G448_DECODE, ECAMD_NO_X448_LADDER   route around one fast path each (results are identical;
 *                                 ECAMD_NO_MPINV1: secp384r1 on the dense 384-bit unit instead of its signed sparse reduction)
 *   ECAMD_NO_ED_FIN_G             EdDSA verification: the final additions / doublings on the saturated-word kernel instead of the unit's own field
 *   ECAMD_NO_SIDE_STREAM          secp256r1 ECDSA verification: k_ecdsa_prep on the caller's stream instead of the context's second stream
 */
#ifndef LIBECC_AMD_H
#define LIBECC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECAMD_OK 0
#define ECAMD_ERR 1
#define ECAMD_INF 2

typedef struct ecamd_ctx ecamd_ctx;     /* one GPU: device id, stream, scratch buffers */
typedef struct ecamd_curve ecamd_curve; /* ec_params equivalent (curves/ec_params.h:51-87) */

/* ---- context ---- */
int ecamd_device_count(void);
int ecamd_ctx_create(ecamd_ctx **ctx, int device);
void ecamd_ctx_destroy(ecamd_ctx *ctx);
const char *ecamd_last_error(void);
/* Upper bound on the items processed per kernel launch (bounds the per-lane window-table
 * scratch: 16 * 3 * 4*ceil(|p|/32) bytes per item).  Default 2^20. */
int ecamd_ctx_set_max_chunk(ecamd_ctx *ctx, uint32_t max_items);
/* Ed25519 whole-batch verification (ec_eddsa_verify_all_batch) through the multi-scalar multiplication: mode 0 never, 1 for
 * batches of at least min_items (default; min_items = 0 keeps the current threshold, initially 2^17 or $ECAMD_MSM_MIN),
 * 2 always.  items_per_lane: signatures that share one lane's doublings, 0 = chosen from the batch size (1 .. 8). */
int ecamd_ctx_set_eddsa_msm(ecamd_ctx *ctx, int mode, uint32_t min_items, uint32_t items_per_lane);
/* Key of the random z_i of the NEXT whole-batch verification on this context (used once, then wiped): 32 bytes from the caller's
 * own randomness source instead of getrandom -- libsign_amd.so passes bytes of the application's get_random, the import libecc's
 * own batch verifier draws its z_i from (sig/eddsa.c:2388), so a seeded test harness makes the combination reproducible. */
int ecamd_ctx_set_msm_seed(ecamd_ctx *ctx, const uint8_t seed[32]);
/* Drops a seed that no whole-batch call has consumed (a seed keys ONE call: every ec_*_verify_all_batch entry point discards what is
 * left when it returns, and the ecamd_multi_* forms call this for the ranks that received no shard). */
int ecamd_ctx_discard_msm_seed(ecamd_ctx *ctx);
/* Secret scalars.  By default the kernels index their window / comb tables with the scalar's digits (fastest; fine for public
 * scalars: verification, public-key checks).  With this switch on, every multiplication by a caller-supplied scalar issued through
 * the context -- ec_prj_pt_mul_batch*, and inside ec_ecdsa_sign_batch, ec_ecccdh_derive_batch ([d]Q), ec_eddsa_sign_R_batch, key-pair
 * import -- uses constant-address table look-ups (every entry read, the wanted one kept by masking: the posture of the reference's
 * masked ladder, curves/prj_pt.c:1225-1260, and nn_tabselect, nn/nn.c:564), a fixed window count and no digit-indexed comb table (fixed-base
 * multiplications use a 4-bit comb whose windows are scanned whole: k_p256_comb4m, k_comb_g<.., SCAN4>; ECAMD_NO_SECRET_COMB: the scanned window loop).  The
 * radix-2^29 pipelines stay in use: k_p256_loop<KW, MASKED> / k_loop_g<.., MASKED> scan the item's eight affine entries (secp256k1:
 * its eight Jacobian ones); only scalars longer than those kernels take (8 NW + 4 bytes) run on the complete-formula kernel with
 * sixteen-entry scans.  One branch remains: a lane whose accumulator met an exceptional pair of the incomplete addition
 * (probability about 2^-|q| per window for a random scalar) is recomputed by the complete-formula kernel.
 * Scalars that are public by construction -- u1, u2 of ECDSA verification, h and S of EdDSA verification, the group order and
 * cofactor of subgroup checks -- keep the fast look-ups in either mode.  Results are identical; DESIGN.md 2.3 has the cost.
 * X25519 / X448 ladders are address-independent in either mode. */
int ecamd_ctx_set_secret_scalars(ecamd_ctx *ctx, int on);
/* Zero every scratch buffer of the context in HBM (window tables, recoded scalars, staged copies of the caller's arrays): after
 * calls that handled secret scalars nothing derived from them stays behind.  Waits for the context's work; synchronous. */
int ecamd_ctx_wipe_scratch(ecamd_ctx *ctx);
/* The context's own stream (a hipStream_t), the one the *_dev entry points use when given NULL. */
void *ecamd_ctx_stream(ecamd_ctx *ctx);
/* Page-locked host memory (valid for every device) for arrays passed to the host-pointer entry points: their copies then run as
 * asynchronous DMA at PCIe rate.  NULL on failure.  Any host memory works; this is only faster. */
void *ecamd_host_alloc(size_t bytes);
void ecamd_host_free(void *p);
/* Producer hook of the host-pointer entry points.  Those stage the caller's arrays through the device in chunks of host_chunk items
 * (ECAMD_HOST_CHUNK), chunk c+1's copies overlapping chunk c's kernels; a caller that is still FILLING its input arrays while the call
 * runs registers fn, which the call invokes -- on the calling thread, with the context's lock held -- before it reads items
 * [first, first + count) of the call's input arrays, and which returns once that range is complete.  libsign_amd.so uses it so that
 * its host threads marshal libecc structures into the tail of a batch while the GPU already works on its head (it is the whole of the
 * overlap between the typed layer's packing and the device: one call per batch, no quarter-batch launches).  NULL clears it; the
 * hook stays until cleared and applies to every host-pointer call on the context.  fn must not call into the context. */
typedef void (*ecamd_host_ready_fn)(void *arg, uint32_t first, uint32_t count);
int ecamd_ctx_set_host_ready_hook(ecamd_ctx *ctx, ecamd_host_ready_fn fn, void *arg);
/* Measurement hook: when enabled, HIP events are recorded (on the stream the kernels run on) around
 * the kernels of the next ec_prj_pt_mul_batch[_dev] call; ecamd_ctx_kernel_times() waits for them and
 * returns the 4 durations in ms: table, table->affine, window loop, finalisation (the generic
 * radix-2^29 path reports 0, 0, loop, finalisation). */
int ecamd_ctx_enable_kernel_timing(ecamd_ctx *ctx, int on);
int ecamd_ctx_kernel_times(ecamd_ctx *ctx, double *ms, int n);
/* The same hook for the protocol entry points: duration (ms) of the dominant kernel of the last call made with timing enabled --
 * the interleaved window loop of secp256r1 ECDSA verification, the X25519 / X448 ladder, the Edwards window loop of Ed25519
 * verification.  (ECDSA verification on other curves is two scalar multiplications: ecamd_ctx_kernel_times covers them.) */
int ecamd_ctx_dominant_kernel_ms(ecamd_ctx *ctx, double *ms);

/* ---- curves: ec_get_curve_params_by_name (curves/curves.h:21) + import_params
 *      (curves/ec_params.h:89).  Same 44 names as libecc's ec_maps[] ("SECP256R1", ...). ---- */
int ecamd_curve_by_name(ecamd_ctx *ctx, const char *name, ecamd_curve **curve);
/* User-defined curve from big-endian domain parameters (the ec_str_params fields,
 * curves/known/ec_params_external.h:42-102; Montgomery constants are derived here). */
int ecamd_curve_from_params(ecamd_ctx *ctx, const uint8_t *p, uint32_t p_len, const uint8_t *a,
			    uint32_t a_len, const uint8_t *b, uint32_t b_len,
			    const uint8_t *curve_order, uint32_t curve_order_len, const uint8_t *gx,
			    uint32_t gx_len, const uint8_t *gy, uint32_t gy_len,
			    const uint8_t *gen_order, uint32_t gen_order_len, ecamd_curve **curve);
void ecamd_curve_free(ecamd_curve *curve);
int ecamd_curve_coord_len(const ecamd_curve *curve); /* BYTECEIL(p_bitlen): 32 / 48 / 66 ... */
int ecamd_curve_order_len(const ecamd_curve *curve); /* BYTECEIL(bitlen(generator order)) */
int ecamd_curve_words(const ecamd_curve *curve);     /* 32-bit words per field element */

/*
 * ---- the hot path: batched prj_pt_mul ----
 * Replaces, per item i:
 *   nn_init_from_buf(m, scalars + i*scalar_len, scalar_len)            nn/nn.c:479
 *   prj_pt_import_from_aff_buf(P, points + i*2*clen, 2*clen, crv)      curves/prj_pt.c:511
 *     (points == NULL: P = the generator, params->ec_gen)
 *   prj_pt_mul(Q, m, P)                                                curves/prj_pt.c:1759
 *   prj_pt_unique(Q, Q)                                                curves/prj_pt.c:241
 *   prj_pt_export_to_aff_buf(Q, out + i*2*clen, 2*clen)                curves/prj_pt.c:600
 * scalars: n x scalar_len big-endian, ANY value (m >= q is fine, as in libecc).
 * points / out: n x 2*clen, affine X || Y, big-endian.   status: n bytes (ECAMD_*).
 * Host-pointer form: synchronous (H2D, kernel, D2H).
 */
int ec_prj_pt_mul_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n,
			const uint8_t *scalars, uint32_t scalar_len, const uint8_t *points_aff,
			uint8_t *out_aff, uint8_t *status);
/* Batch form of prj_pt_mul_blind (curves/prj_pt.c:1782-1822): per item the scalar actually multiplied is m + b * #E (#E = the curve
 * order, cofactor included), b = blinds + i*blind_len big-endian, supplied by the caller (the reference draws b at random in
 * [1, #E); randomness stays on the host here, as for nonces).  Since [#E]P is the point at infinity the result equals
 * ec_prj_pt_mul_batch's; what changes is the scalar the device walks through -- about 2 |q| bits, which on secp256r1 still runs on
 * the radix-2^29 window kernel.  status ECAMD_ERR also where b = 0 or b >= #E. */
int ec_prj_pt_mul_blind_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *scalars, uint32_t scalar_len,
			      const uint8_t *blinds, uint32_t blind_len, const uint8_t *points_aff, uint8_t *out_aff, uint8_t *status);
/* Device-pointer form: all four buffers already live in HBM; the kernel is enqueued on
 * hip_stream (a hipStream_t, NULL = the context's stream) and the call returns without
 * synchronising. */
int ec_prj_pt_mul_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n,
			    const void *d_scalars, uint32_t scalar_len, const void *d_points_aff,
			    void *d_out_aff, void *d_status, void *hip_stream);
int ecamd_ctx_synchronize(ecamd_ctx *ctx);

/* ---- group law: batched prj_pt_add (curves/prj_pt.c:1204) / prj_pt_dbl (:1132) on affine
 *      encoded inputs, affine encoded output (host pointers) ---- */
int ec_prj_pt_add_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *p1_aff,
			const uint8_t *p2_aff, uint8_t *out_aff, uint8_t *status);
int ec_prj_pt_dbl_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *p_aff,
			uint8_t *out_aff, uint8_t *status);

/* ---- field level: batched fp ops on libecc's limb layout: n x nlimbs little-endian 64-bit
 *      words per operand, nlimbs = ceil(|p|/64) (nn/nn.h:42-45).  Inputs must be < p.
 *   ECAMD_FP_MUL_MONTY  fp_mul_monty = nn_mul_redc1: a*b*2^(-64*nlimbs) mod p
 *                       (fp/fp_montgomery.c:44, nn/nn_mul_redc1.c:246)
 *   ECAMD_FP_ADD / SUB  fp_add / fp_sub (fp/fp_add.c:23,69)
 *   ECAMD_FP_MUL        plain fp_mul (fp/fp_mul.c:23)
 *   ECAMD_FP_INV        fp_inv (fp/fp_mul.c:51), b ignored; inv(0) = 0 ---- */
#define ECAMD_FP_MUL_MONTY 0
#define ECAMD_FP_ADD 1
#define ECAMD_FP_SUB 2
#define ECAMD_FP_MUL 3
#define ECAMD_FP_INV 4
int ec_fp_op_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int op, uint32_t n, const uint64_t *a,
		   const uint64_t *b, uint64_t *out);

/*
 * ---- protocol callers of the hot path ----
 * ECDSA verification, batch of independent (public key, signature, digest) triples: per item
 *   ec_pub_key_import_from_aff_buf(pub, params, pubkeys + i*2*clen, 2*clen, ECDSA)   sig/ec_key.c:181
 *   ec_verify(sig, 2*qlen, pub, m, mlen, ECDSA, hash, NULL, 0)                       sig/sig_algs.c:655
 * where the caller supplies h = H(m) (hashing stays on the host; the reference exposes the same
 * split as ecdsa_verify_raw, sig/fuzzing_ecdsa.h).  sigs: n x 2*qlen (r || s big-endian),
 * digests: n x digest_len.  result[i] = 0 accept / 1 reject (ec_verify's 0 / -1).
 */
int ec_ecdsa_verify_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *pubkeys_aff,
			  const uint8_t *sigs, const uint8_t *digests, uint32_t digest_len, uint8_t *result);
/*
 * ECDSA public-key recovery, batch of independent (signature, digest) pairs: per item
 *   ecdsa_public_key_from_sig(pub1, pub2, params, sig, 2*qlen, h, hlen)              sig/ecdsa.c (decdsa_public_key_from_sig: sig/decdsa.c)
 *     -> __ecdsa_public_key_from_sig                                                 sig/ecdsa_common.c:867-1049
 *   ec_pub_key_export_to_aff_buf(pub1 / pub2, out, 2*clen)                           sig/ec_key.c
 * the call libecc's self tests make after every ECDSA / DECDSA signature (tests/ec_self_tests_core.c:423, :839).
 * sigs: n x 2*qlen (r || s big-endian), digests: n x digest_len (1 .. 128 bytes).  pub1_aff / pub2_aff: n x 2*clen, the affine
 * X || Y of the reference's two candidate keys Y1 = [v](r, y1) + [u]G and Y2 = [v](r, y2) + [u]G, u = -(e / r), v = s / r mod q,
 * (y1, y2) the roots in aff_pt_y_from_x's order.  status1[i] / status2[i]: ECAMD_ERR in both (zero bytes) where the reference
 * returns -1 -- r or s outside [1, q - 1], r >= p, r no abscissa of the curve (the reference's "restart" with r + 2q never
 * succeeds: :908-925 with fp_set_nn, fp/fp.c:204-220) --; otherwise, per key, ECAMD_OK or ECAMD_INF (zero bytes: that key is
 * the point at infinity, which the reference returns without complaint).  No recovery id: the reference has none.  On curves with
 * a cofactor the signer's key is mostly not among the two, as the reference's own comment says; the bytes are the reference's.
 * Every multiplier is public, so the call runs its public-scalar kernels whatever ecamd_ctx_set_secret_scalars says.
 */
int ec_ecdsa_recover_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *sigs, const uint8_t *digests,
			   uint32_t digest_len, uint8_t *pub1_aff, uint8_t *pub2_aff, uint8_t *status1, uint8_t *status2);
/* The same with a choice of public-key format: ECAMD_PT_PROJECTIVE keys are n x 3*clen, X || Y || Z as ec_pub_key_export_to_buf
 * writes pub_key->y (sig/ec_key.c:254): imported like prj_pt_import_from_buf, normalised on the device.  A key that is the point
 * at infinity is a key for libecc (its import accepts (0 : 1 : 0)); verification against it is W' = uG, reproduced here. */
int ec_ecdsa_verify_batch_fmt(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *pubkeys, int pub_fmt,
			      const uint8_t *sigs, const uint8_t *digests, uint32_t digest_len, uint8_t *result);
/* Verification from MESSAGES instead of digests (round 4): the hash is computed on the device.  Item i's message sits in a slot of
 * msg_stride bytes (one stride per call, a multiple of 4, at most 4096): a little-endian u32 length, then the bytes
 * (4 + length <= msg_stride).  hash_type: libecc's hash_alg_type numbers (hash/hash_algs.h) 1 = SHA224, 2 = SHA256, 3 = SHA384,
 * 4 = SHA512 -- the digests are FIPS 180-4's, the bytes libecc's hfunc_* produce.  Everything else is ec_ecdsa_verify_batch_fmt /
 * ec_eddsa_verify_batch; for EdDSA the slot holds what the verifier hashes, dom2 || R || A || PH(M) (Ed25519: SHA-512).
 * Why: end to end, a libecc application spends more host time hashing short messages (0.3 - 0.5 us each in portable C) than on
 * everything else it does per signature; a million short messages are less than 0.1 ms of one kernel. */
int ec_ecdsa_verify_msg_batch_fmt(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *pubkeys, int pub_fmt,
				  const uint8_t *sigs, int hash_type, const uint8_t *msg_slots, uint32_t msg_stride, uint8_t *result);
int ec_eddsa_verify_msg_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
			      const uint8_t *hash_slots, uint32_t stride, uint8_t *result);
/* (The two entry points below also take the WEI448 handle: Ed448, 57-octet encodings, 114-octet signatures, SHAKE256 with 114 octets of
 * output -- 64 for the pre-hash --, keys n x 3*56 bytes.)
 * The same from the PROJECTIVE key an ec_pub_key holds (n x 3*32 bytes X || Y || Z on WEI25519, the layout of ec_pub_key_export_to_buf's
 * payload): the key is imported and normalised as prj_pt_import_from_buf / prj_pt_unique do, encoded as eddsa_export_pub_key does
 * (sig/eddsa.c:795), and the 32 octets are written into the item's hash input at message offset a_offset (bytes 4 + a_offset .. of its
 * slot, which the caller leaves blank and counts in the slot's length; the caller's array is not modified) before hashing -- what
 * ec_eddsa_encode_point_batch, a copy back, and ec_eddsa_verify_msg_batch would do in three steps.  An item whose key does not import
 * is rejected (result 1); a key at infinity encodes as (0, 1) and is rejected by the small-order test like in the reference. */
int ec_eddsa_verify_msg_prj_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
				  const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, uint8_t *result);
/* ec_verify_batch's ONE bit for plain Ed25519 / Ed25519ctx from the same inputs (round 6): the front end per staging chunk as above, then
 * the reference's batch equation over the whole batch as one multi-scalar multiplication per max_chunk items (by buckets from 2^18 items
 * on; Ed448 on the WEI448 handle: 57-octet encodings, SHAKE256, the combination of ec_eddsa_verify_all_batch's Ed448 form).  *all_valid = 0
 * means "not decided here" -- a bad signature, a key that does not import or has no encoding, or a handle without the form: verify
 * item by item (ec_eddsa_verify_msg_prj_batch).  Ed25519, one piece, by buckets: the decodings, the scalars and the filing run on every
 * staging chunk (2^17 items) as it lands, the bucket sums and their reduction after the last ($ECAMD_NO_ED_STREAM: everything after the last). */
int ec_eddsa_verify_msg_prj_all_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
				      const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, int *all_valid);
/* The pre-hashed variant (EDDSA25519PH, sig/eddsa.c:1049-1080, :1995-2045): the hash input is dom2(1, context) || R || A || PH(M) with
 * PH(M) = SHA-512(M).  The caller leaves 96 blank octets at message offset a_offset (A, then PH(M)) and hands the messages over in
 * slots of their own (msg_slots, msg_stride: u32 length + bytes); both hashes run on the device. */
int ec_eddsa_verify_ph_prj_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
				 const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, const uint8_t *msg_slots, uint32_t msg_stride,
				 uint8_t *result);
/* ECDSA signing with caller-supplied nonces: per item the tail of ec_sign / __ecdsa_sign_finalize
 * (sig/ecdsa_common.c:318-586) -- kG = prj_pt_mul(k, G), r = kG.x mod q, s = k^-1 (x r + e) mod q --
 * with h = H(m) and the nonce k supplied by the caller (random; for RFC 6979 see ec_decdsa_sign_batch, which derives
 * k on the device; the reference's KAT harness injects k through the same ctx->rand hook).  privs, nonces: n x qlen;
 * sigs: n x 2*qlen.  status[i] = 1 where the reference would fail or restart (private key >= q, k not in [1, q-1],
 * r = 0, e == x r, s = 0). */
int ec_ecdsa_sign_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *privs,
			const uint8_t *nonces, const uint8_t *digests, uint32_t digest_len, uint8_t *sigs,
			uint8_t *status);
/*
 * ECGDSA, ECRDSA and SM2: the three other schemes of libecc's table whose verification has ECDSA's shape -- range checks, two
 * public multipliers from a little algebra mod q, W' = [u]G + [v]Y, a comparison of W'.x mod q -- and whose signing is one
 * fixed-base [k]G plus algebra with the private key.  alg: libecc's ec_alg_type numbers (lib_ecc_types.h); any other value is
 * a call-level error (-1).  Per item, verification is
 *   ec_pub_key_import_from_aff_buf(pub, params, pubkeys + i*2*clen, 2*clen, alg)     sig/ec_key.c:181
 *   ec_verify(sig, 2*qlen, pub, m, mlen, alg, hash, adata, adata_len)                sig/sig_algs.c:655
 * with result[i] = 0 / 1 for its 0 / -1, for every input: a key that does not import (coordinate >= p, off the curve, outside
 * the subgroup on a cofactor curve), r or s outside [1, q - 1], SM2's r + s = q, W' at infinity.  Signing is the tail of
 * _ec_sign (_ecgdsa_sign_finalize sig/ecgdsa.c:181-376, _ecrdsa_sign_finalize sig/ecrdsa.c:196-378, _sm2_sign_finalize
 * sig/sm2.c:310-483) with the nonce k supplied by the caller, as for ec_ecdsa_sign_batch; status[i] = 1 with zero signature
 * bytes where ec_key_pair_import_from_priv_key_buf refuses the private key (x >= q; ECGDSA x = 0, its public key being
 * [1/x]G; SM2 x >= q - 1, where 1 + x has no inverse) or _ec_sign fails on it (SM2 x = 0: a key at infinity has no Z), k is not in [1, q - 1], or the reference restarts (r = 0, s = 0).
 * Private keys are x itself (ECGDSA's public key is [1/x]G, the other two [x]G).
 * `digests` are the bytes the scheme's finalize turns into an integer, digest_len (1 .. 128) each; hashing stays with the caller:
 *   ECGDSA, ECRDSA  H(m)
 *   SM2             H(Z || m),  Z = H(ENTL || ID || a || b || xG || yG || xY || yY)                 sig/sm2.c:121-205
 *                   (ENTL: the bit length of the signer's id ID on two bytes, big-endian; the curve's a and b, the generator
 *                   and the signer's key Y as big-endian field elements of clen bytes; libecc passes ID as `adata`)
 * and are read by the scheme's rule: ECGDSA big-endian, the leftmost |q| bits when longer (ECDSA's rule); ECRDSA byte-reversed
 * (libecc's default build, without USE_ISO14888_3_ECRDSA), the whole digest mod q, 0 becoming 1; SM2 big-endian, the whole
 * digest mod q.  libecc accepts any of its hashes with the three schemes, and so do these calls.
 * Layouts, chunking by ecamd_ctx_set_max_chunk, n = 0 and argument errors as ec_ecdsa_verify_batch / ec_ecdsa_sign_batch.
 * Verification multiplies by public values only, whatever ecamd_ctx_set_secret_scalars says; signing's [k]G honours it.
 */
#define ECAMD_SIG_ECGDSA 6
#define ECAMD_SIG_ECRDSA 7
#define ECAMD_SIG_SM2 8
int ec_sig_verify_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const uint8_t *pubkeys_aff,
			const uint8_t *sigs, const uint8_t *digests, uint32_t digest_len, uint8_t *result);
int ec_sig_sign_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const uint8_t *privs,
		      const uint8_t *nonces, const uint8_t *digests, uint32_t digest_len, uint8_t *sigs, uint8_t *status);
/*
 * The same three schemes from MESSAGES: the hashes they are deployed with run on the device, SM2's Z too, in front of the
 * digest-level cores above, for the reason given at ec_ecdsa_verify_msg_batch_fmt (a portable-C Streebog or SM3 on the host costs
 * more per item than everything else).  Verdicts, signature bytes and status are those of ec_sig_verify_batch / ec_sig_sign_batch
 * fed with libecc's digests.
 *   hash_type  libecc's hash_alg_type numbers: 1 .. 4 (SHA-224 / 256 / 384 / 512), 11 (SM3), 13, 14 (Streebog-256 / -512; octet
 *              order of message and digest as libecc's hash/streebog.c).  SM2's Z is computed with SM3 or SHA-2: SM2 with 13 or 14,
 *              and any other alg or hash_type, is a call-level error (-1, ecamd_last_error()).
 *   msg_slots  the slots of ec_ecdsa_verify_msg_batch_fmt: a little-endian u32 length, then the bytes; stride a multiple of 4 in
 *              4 .. 4096.  For SM2 the hash input is <blank> || m: the caller leaves hsize octets empty in front of the message and
 *              counts them in the length, as for ECSDSA; the device writes Z into a staged copy.  The caller's array is never
 *              modified.  A slot that does not fit its stride (4 + length > stride), or for SM2 is shorter than the blank, is
 *              result / status 1 (signing: with zero signature bytes).
 *   id, id_len SM2 only (ignored otherwise): the signer's ID of Z, ONE HOST pointer per call, in the _dev forms too (as DBIGN's t);
 *              0 .. 1024 octets (libecc: SM2_MAX_ID_LEN 8191).  id == NULL with id_len > 0, or a longer id, is a call-level error.
 *              Z takes xY || yY as the octets of the affine key; ENTL || ID || a || b || xG || yG is absorbed once per call on the
 *              host and the kernel starts from its midstate.
 *   pubkeys_aff of signing: SM2 only (ignored otherwise), for Z: n x 2 clen, or NULL -- then Y = [x]G is computed on the device with the
 *              fixed-base multiplication, which honours ecamd_ctx_set_secret_scalars.  An SM2 item whose key does not import (off the
 *              curve, a coordinate >= p, Y at infinity) or whose x the digest-level rules refuse is status 1 with zero bytes.
 * ec_hash_slots_batch is the bare hash: n x hsize digests of the slots (for 11, 13, 14 a slot that does not fit its stride gets
 * an all-zero digest; 1 .. 4 run the kernel of ec_ecdsa_verify_msg_batch_fmt, which hashes what fits).
 * Key rules, n = 0, NULL arguments, foreign handles, chunking by ecamd_ctx_set_max_chunk as ec_decdsa_sign_batch; ecamd_ctx_wipe_scratch
 * covers the staged slots.  Not here: SHA-3, SHA-512/t, RIPEMD-160 and BASH in these message-level calls (the device hashes them
 * through ec_digest_slots_batch below, in front of the digest-level _dev forms), the ecamd_multi_* wrappers, the libecc-typed
 * boundary (libsign_amd), and ECKCDSA's z prefix.
 */
int ec_sig_verify_msg_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *pubkeys_aff,
			    const uint8_t *sigs, const uint8_t *msg_slots, uint32_t stride, const uint8_t *id, uint32_t id_len,
			    uint8_t *result);
int ec_sig_verify_msg_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_pubkeys_aff,
				const void *d_sigs, const void *d_msg_slots, uint32_t stride, const uint8_t *id, uint32_t id_len,
				void *d_result, void *hip_stream);
int ec_sig_sign_msg_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *privs,
			  const uint8_t *pubkeys_aff, const uint8_t *nonces, const uint8_t *msg_slots, uint32_t stride, const uint8_t *id,
			  uint32_t id_len, uint8_t *sigs, uint8_t *status);
int ec_sig_sign_msg_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_privs,
			      const void *d_pubkeys_aff, const void *d_nonces, const void *d_msg_slots, uint32_t stride, const uint8_t *id,
			      uint32_t id_len, void *d_sigs, void *d_status, void *hip_stream);
int ec_hash_slots_batch(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *msg_slots, uint32_t stride, uint8_t *digests);
int ec_hash_slots_batch_dev(ecamd_ctx *ctx, int hash_type, uint32_t n, const void *d_msg_slots, uint32_t stride, void *d_digests,
			    void *hip_stream);
/*
 * The bare hash over the WHOLE table: every fixed-length hash of libecc's hash_alg_type except belt-hash, on the device, of the same
 * message slots (a little-endian u32 length, then the bytes; stride a multiple of 4 in 4 .. 4096).
 *   hash_type  1 .. 4 (SHA-224 / 256 / 384 / 512), 5 .. 8 (SHA3-224 / 256 / 384 / 512), 9, 10 (SHA-512/224, SHA-512/256), 11 (SM3),
 *              13, 14 (Streebog-256 / -512), 15 (RIPEMD-160), 17 .. 20 (BASH224 / 256 / 384 / 512, STB 34.101.77).  Not served:
 *              0, 12 (SHAKE256 is no fixed-length hash here; Ed448's entry points use it), 16 (belt-hash: ec_bign_* hash with it
 *              themselves) and anything outside 1 .. 20.
 *   digests    n x ecamd_digest_len(hash_type) octets, the bytes libecc's hfunc_* produce.  ecamd_digest_len: 28 .. 64, 20 for
 *              RIPEMD-160, 0 for a number that is not served.
 *   a slot that does not fit its stride (4 + length > stride) gets an all-zero digest, for EVERY served number (ec_hash_slots_batch
 *              with 1 .. 4 hashes what fits instead).
 * The older entry points keep the hash sets they accept -- ec_hash_slots_batch, ec_sig_*_msg_batch, ec_bign_*, ec_dbign_*, ec_bip0340_*,
 * ec_decdsa_*, ec_rfc6979_* and the rest refuse 5 .. 10, 15 and 17 .. 20 as before, a behaviour their callers and tests rely on.  The
 * new hashes reach the protocols by COMPOSITION on the device: ec_digest_slots_batch_dev into a device buffer, then the digest-level
 * _dev call on the same stream -- ec_ecdsa_verify_batch_dev / ec_ecdsa_sign_batch_dev, ec_sig_verify_batch_dev / ec_sig_sign_batch_dev
 * (digest_len = ecamd_digest_len), ec_bign_verify_batch_dev / ec_bign_sign_batch_dev and ec_dbign_sign_batch_dev with hash_type 0 and
 * stride = the digest length.  The digests never leave device memory.  That is how BIGN runs with BASH384 on bign384v1 and BASH512 on
 * bign512v1, the standard's configuration, and ECDSA with SHA-3.
 * Everything hashed is public: nothing differs under ecamd_ctx_set_secret_scalars.  n = 0, NULL arguments, foreign handles, chunking
 * by ecamd_ctx_set_max_chunk, and the _dev form only enqueueing, as ec_hash_slots_batch[_dev]; any other hash_type or stride is a
 * call-level error (-1, ecamd_last_error()).
 * Out of scope: the accepted hash sets of every existing entry point (HMAC and RFC 6979 over the whole table have entry points of
 * their own: ec_hmac_slots_batch, ec_rfc6979_nonce_ht_batch, ec_decdsa_sign_ht_batch); SM2's Z, the commitment
 * hashes of ECSDSA / ECOSDSA / ECKCDSA / BIP0340 / ECFSDSA and EdDSA with the new hashes; SHAKE256 as a fixed-length hash (12); the
 * ecamd_multi_* wrappers and the libecc-typed layer.
 */
int ecamd_digest_len(int hash_type);
int ec_digest_slots_batch(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *msg_slots, uint32_t stride, uint8_t *digests);
int ec_digest_slots_batch_dev(ecamd_ctx *ctx, int hash_type, uint32_t n, const void *d_msg_slots, uint32_t stride, void *d_digests,
			      void *hip_stream);
/*
 * The same hashes over VARIABLE-LENGTH messages: one packed array of octets and n + 1 offsets in place of fixed-stride slots, so a message
 * may have any length (up to 2^28 octets), a batch of unequal messages uploads its octets and nothing else, and the prefixes libecc's
 * schemes put in front of a message are given once, not copied into every item.  Item i hashes
 *     call_prefix || item_prefixes[i] || msgs[offsets[i] .. offsets[i + 1])
 *   hash_type    the set of ec_digest_slots_batch: 1 .. 11, 13 .. 15, 17 .. 20; anything else is a call-level error.
 *   msgs         the messages one behind the other.  offsets: n + 1 uint64_t in host byte order (little-endian), offsets[n] the
 *                array's length in the host form.  Offsets need not be contiguous or increasing from item to item: each item stands
 *                alone.
 *   call_prefix  0 .. 256 octets, the same for every item; a HOST pointer in both forms (as SM2's id is).  NULL with length 0.
 *   item_prefixes  item_prefix_len octets (0 .. 256, one length per call) at item_prefixes + i * item_prefix_stride
 *                (item_prefix_stride >= item_prefix_len; any alignment).  NULL with length 0.
 *   digests      n x ecamd_digest_len(hash_type) octets.  status (n octets, may be NULL): 0, or 1 with an ALL-ZERO digest for an item
 *                that is unusable: offsets[i] > offsets[i + 1], offsets[i + 1] > the array's length, or an input (both prefixes
 *                and the message) above 2^28 octets.  Nothing of msgs is read for such an item.
 * A prefix length above 256, a NULL pointer with a positive length or a stride below the length is a call-level error (-1,
 * ecamd_last_error()).  n = 0 (returns 0, touches nothing), NULL arguments, a foreign context as for ec_digest_slots_batch; everything
 * hashed is public and nothing differs under ecamd_ctx_set_secret_scalars.
 * _dev form: d_msgs must be 4-byte aligned and readable up to round_up(msgs_len, 4) (the kernel reads aligned 32-bit words, and only
 * words that hold an octet of the item's own message); d_offsets 8-byte aligned; the kernel validates every item against msgs_len
 * itself.  It only enqueues, in pieces of at most ecamd_ctx_set_max_chunk items.
 * Host form: a piece of the batch ends at ecamd_ctx_set_max_chunk items or when the messages of its usable items span more than
 * 2^28 octets of the array (MSGS_CHUNK_BYTES in ecamd_host_sigfam.cpp), whichever comes first; a single longer message is a piece of
 * its own.  Each piece is staged with offsets rebased to it; ecamd_ctx_wipe_scratch covers the staging.
 *
 * COMPOSITION, as above: every digest-level _dev call takes these digests on the same stream, and the two prefixes are what libecc's
 * schemes hash in front of the message --
 *   ECKCDSA   item_prefix = z (the key's certificate data, BLOCK octets of the hash), then ec_sig_hashed_verify_ht_batch_dev /
 *             ec_sig_hashed_sign_ht_batch_dev with the digests as their input
 *   SM2       item_prefix = Z, then ec_sig_verify_batch_dev / ec_sig_sign_batch_dev
 * EdDSA needs no composition: ec_eddsa_verify_msgs_batch, ec_eddsa_verify_msgs_all_batch and ec_eddsa_sign_msgs_batch (below) take this
 * format for all five variants, Ed448's SHAKE256 and the pre-hashed variants included.
 * Out of scope: the slot formats of ECSDSA, ECOSDSA, ECFSDSA and BIP0340 (their message sits behind a point that exists only inside
 * the call), SHAKE256 and belt-hash, HMAC over this format, the ecamd_multi_* wrappers and the libecc-typed layer.
 */
int ec_digest_msgs_batch(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *msgs, const uint64_t *offsets, const uint8_t *call_prefix,
			 uint32_t call_prefix_len, const uint8_t *item_prefixes, uint32_t item_prefix_len, uint32_t item_prefix_stride,
			 uint8_t *digests, uint8_t *status);
int ec_digest_msgs_batch_dev(ecamd_ctx *ctx, int hash_type, uint32_t n, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
			     const uint8_t *call_prefix, uint32_t call_prefix_len, const void *d_item_prefixes, uint32_t item_prefix_len,
			     uint32_t item_prefix_stride, void *d_digests, void *d_status, void *hip_stream);
/*
 * Two protocols straight from that format (no prefixes), so that a signature is reached without the caller handling digests:
 *   ec_ecdsa_verify_msgs_batch   ec_pub_key_import_from_aff_buf + ec_verify(ECDSA) per item with any hash of ec_digest_msgs_batch: the
 *              verdicts of ec_ecdsa_verify_batch fed with libecc's digests; an unusable item (see status above) is result 1.
 *   ec_decdsa_sign_msgs_batch    ec_decdsa_sign_ht_batch with msgs / offsets in place of slots: key rules, the restart rule, the wiped
 *              nonce scratch and the refusal of Streebog (13, 14) in secret-scalar mode unchanged; an unusable item is status 1 with
 *              zero bytes.
 * Layouts of keys, signatures, result and status as for ec_ecdsa_verify_batch and ec_decdsa_sign_ht_batch; msgs, offsets, msgs_len,
 * alignment, pieces and n = 0 as for ec_digest_msgs_batch[_dev].  The _dev forms only enqueue.
 */
int ec_ecdsa_verify_msgs_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *pubkeys_aff,
			       const uint8_t *sigs, const uint8_t *msgs, const uint64_t *offsets, uint8_t *result);
int ec_ecdsa_verify_msgs_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_pubkeys_aff,
				   const void *d_sigs, const void *d_msgs, uint64_t msgs_len, const void *d_offsets, void *d_result,
				   void *hip_stream);
int ec_decdsa_sign_msgs_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *msgs,
			      const uint64_t *offsets, uint8_t *sigs, uint8_t *status);
int ec_decdsa_sign_msgs_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs, const void *d_msgs,
				  uint64_t msgs_len, const void *d_offsets, void *d_sigs, void *d_status, void *hip_stream);
/*
 * ECSDSA, ECOSDSA and ECKCDSA: the schemes of libecc's table that hash AFTER the multiplication.  The verifier computes
 * W' = [u]G + [v]Y, hashes its affine coordinates on the device and compares the digest with the signature's r byte for byte; the
 * signer hashes W = [k]G and derives e = digest mod q.  alg: libecc's ec_alg_type numbers; hash_type: libecc's hash_alg_type
 * numbers 1 .. 4 (SHA-224, SHA-256, SHA-384, SHA-512; hsize = 28, 32, 48, 64).  Any other alg or hash_type is a call-level
 * error (-1, ecamd_last_error()).
 *   sigs     n x (r_len + qlen), r then s big-endian.  r_len = hsize for ECSDSA and ECOSDSA (sig/ecsdsa.h:28),
 *            min(hsize, qlen) for ECKCDSA (sig/eckcdsa.h:28).
 *   inputs   ECSDSA, ECOSDSA: message slots in the format of ec_ecdsa_verify_msg_batch_fmt -- a little-endian u32 length, then
 *            the hash input <blank> || m; stride a multiple of 4, at most 4096, 4 + length <= stride.  The caller leaves the
 *            blank empty and counts it in the length: 2*clen octets for ECSDSA (W'x || W'y), clen for ECOSDSA (W'x)
 *            (sig/ecsdsa_common.c:509-518).  The device writes the coordinates into a staged copy; the caller's array is not
 *            modified.  A slot whose length is shorter than the blank or does not fit the stride is result / status 1.
 *            ECKCDSA: n x hsize digests h = H(z || m), stride = hsize; z is the first block-size octets of Yx || Yy, zero
 *            padded (sig/eckcdsa.c:225-252), and is hashed by the caller, as SM2's Z is.  The device hashes FE2OS(W'x).
 * Per item, verification is ec_pub_key_import_from_aff_buf + ec_verify with result[i] = 0 / 1 for 0 / -1, for every input:
 *   ECSDSA / ECOSDSA (sig/ecsdsa_common.c:474-607): s in [1, q - 1]; e = -(OS2I(r) mod q) mod q over all hsize bytes of r, e != 0;
 *            W' = [s]G + [e]Y not at infinity; accept iff H(W'x [|| W'y] || m) = r.
 *   ECKCDSA (sig/eckcdsa.c:589-800): s in [1, q - 1]; h' = the last r_len bytes of h; e = OS2I(r XOR h') mod q (0 allowed);
 *            W' = [s]Y + [e]G not at infinity; accept iff the last r_len bytes of H(FE2OS(W'x)) = r.
 * Signing is _ec_sign with the nonce k supplied by the caller (k in [1, q - 1]), W = [k]G:
 *   ECSDSA / ECOSDSA (sig/ecsdsa_common.c:180-371): r = H(Wx [|| Wy] || m), e = OS2I(r) mod q, s = (k + e x) mod q; e = 0 or s = 0 fails.
 *   ECKCDSA (sig/eckcdsa.c:340-471): r = the last r_len bytes of H(FE2OS(Wx)), e = OS2I(r XOR h') mod q, s = x (k - e) mod q;
 *            s = 0 restarts, which a fixed nonce cannot get past.
 * status[i] = 1 with zero signature bytes where ec_key_pair_import_from_priv_key_buf or _ec_sign returns -1 or would restart.
 * ECKCDSA: x = 0 or x >= q (its public key is [1/x]G).  ECSDSA and ECOSDSA check no range in the reference, which signs with x = 0
 * and with any x >= q of qlen bytes, s = (k + e x) mod q; so do these calls.
 * Private keys are x itself.  Chunking by ecamd_ctx_set_max_chunk, n = 0 and NULL arguments as ec_sig_verify_batch /
 * ec_sig_sign_batch.  Verification multiplies by public values only; signing's [k]G honours ecamd_ctx_set_secret_scalars, and
 * ecamd_ctx_wipe_scratch covers the staged W and slots.
 */
#define ECAMD_SIG_ECKCDSA 2
#define ECAMD_SIG_ECSDSA 3
#define ECAMD_SIG_ECOSDSA 4
int ec_sig_hashed_verify_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n,
			       const uint8_t *pubkeys_aff, const uint8_t *sigs, const uint8_t *inputs, uint32_t stride, uint8_t *result);
int ec_sig_hashed_sign_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *privs,
			     const uint8_t *nonces, const uint8_t *inputs, uint32_t stride, uint8_t *sigs, uint8_t *status);
/* BIP0340 and ECFSDSA ITEM BY ITEM: the two Schnorr-type schemes whose signature carries the commitment as a point, with a verdict
 * per item -- what ec_schnorr_verify_all_batch / ec_schnorr_verify_msg_all_batch cannot give ("valid" or "not decided" for the whole
 * batch) -- and their signing.  alg: libecc's ec_alg_type numbers (lib_ecc_types.h); hash_type 1 .. 4 (SHA-224 / 256 / 384 / 512);
 * any other alg or hash_type is a call-level -1 with ecamd_last_error().
 *
 * Verification is, per item, ec_pub_key_import_from_aff_buf (key_fmt ECAMD_PT_AFFINE: keys n x 2*clen X || Y) or
 * ec_pub_key_import_from_buf (ECAMD_PT_PROJECTIVE: n x 3*clen X || Y || Z) followed by ec_verify; result[i] = 0 / 1 for its 0 / -1, for
 * EVERY input.  Keys, signatures (r_len + qlen bytes, r_len = clen for BIP0340 and 2*clen for ECFSDSA) and hash slots have the formats of
 * ec_schnorr_verify_msg_all_batch, so a caller whose whole-batch call came back "not decided" hands the same arrays to this call.
 * A slot is a little-endian u32 length, then the scheme's hash input, `stride` bytes in all (a multiple of 4 in 4 .. 4096):
 *   BIP0340  H(tag) || H(tag) || r || <blank clen> || m     tag = "BIP0340/challenge" (sig/bip0340.c:437-441)
 *   ECFSDSA  W.x || W.y || m                               (sig/ecfsdsa.c:472-482)
 * The caller's array is never modified: in a staged copy the device writes the key's x into the blank and OVERWRITES the commitment
 * field with the signature's own r (W) bytes, so the verdict depends on key, signature and message only.  A slot whose length does not
 * hold the fixed fields or does not fit the stride rejects its item; a stride too small for the fixed fields rejects every item.
 *   BIP0340 (sig/bip0340.c:383-560): the key's unique representative (a key at infinity fails), then the one with an even y; r < p,
 *     s < q (s = 0 is NOT refused by the range check); e = H(slot) mod q over the whole digest; R = [s]G + [q - e]Y must be finite, have
 *     an even y and R.x = r.
 *   ECFSDSA (sig/ecfsdsa.c:404-607): W.x, W.y < p and W on the curve, s in [1, q - 1]; e = H(W.x || W.y || m) mod q; W' = [s]G + [q - e]Y
 *     must be finite and both affine coordinates equal the signature's bytes.  A key at infinity (0 : y : 0) is used as it is (W' = [s]G);
 *     (0 : 0 : 0) imports but cannot be multiplied: rejected.
 * On cofactor curves the key import's subgroup check ([q]Y = infinity) applies.  There is no prime-order restriction and no radix-2^29
 * requirement: every handle ec_prj_pt_mul_batch serves is served, ecamd_curve_from_params handles included.  Every multiplier is public
 * (whatever ecamd_ctx_set_secret_scalars says).
 *
 * Signing is _ec_sign with the nonce supplied by the caller, as for every other signing call here.
 *   nonces  n x qlen: the value k the scheme multiplies G by, k in [1, q - 1], otherwise status 1.  For BIP0340 that is the reference's
 *           H_nonce(...) mod q (sig/bip0340.c:237-294); THIS call takes it from the caller.  ec_bip0340_sign_batch below derives it on
 *           the device from the aux value (the "BIP0340/aux" and "BIP0340/nonce" tagged hashes), as ec_decdsa_sign_batch does for ECDSA.
 *   privs   n x qlen: x itself.  BIP0340: 0 < x < q, ECFSDSA: x < q (the reference signs with x = 0: s = k), otherwise status 1.
 *   pubkeys_aff  BIP0340: the key pair's public half, n x 2*clen -- its x is hashed and the parity of its y decides d <-> q - d.  NULL:
 *           the device derives Y = [x]G (fixed-base, honours secret-scalar mode).  Non-NULL: imported (coordinates < p, on the curve,
 *           otherwise status 1) and used as the reference uses key_pair->pub_key (not compared with [x]G).  ECFSDSA ignores it.
 *   slots   BIP0340: H(tag) || H(tag) || <blank clen: r> || <blank clen: Y.x> || m;  ECFSDSA: <blank 2*clen: W> || m; the blanks are
 *           counted in the length.  Unusable slots and a stride too small: as in verification, status 1.
 *   BIP0340: R = [k]G, affine; R.y odd: k <- q - k; Y.y odd: d = q - x, else d = x; r = R.x, e = H(slot) mod q, s = (k + e d) mod q.
 *   ECFSDSA: W = [k]G, r = W.x || W.y, e = H(r || m) mod q, s = (k + e x) mod q; s = 0 is status 1.
 * A status 1 item has all-zero signature bytes.  [k]G (and [x]G) honour ecamd_ctx_set_secret_scalars.
 * Chunking by ecamd_ctx_set_max_chunk, n = 0, NULL arguments and a handle of another context behave as for ec_sig_hashed_*;
 * ecamd_ctx_wipe_scratch covers the staged slots, keys and commitments. */
#define ECAMD_SIG_ECFSDSA 5
#define ECAMD_SIG_BIP0340 20
int ec_schnorr_verify_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *keys, int key_fmt,
			    const uint8_t *sigs, const uint8_t *hash_slots, uint32_t stride, uint8_t *result);
int ec_schnorr_sign_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *privs,
			  const uint8_t *pubkeys_aff, const uint8_t *nonces, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
			  uint8_t *status);
/* BIGN and DBIGN (STB 34.101.45; sig/bign_common.c): the scheme that hashes its commitment with belt-hash (STB 34.101.31),
 * whatever hash the message had.  alg: libecc's ec_alg_type numbers 18 / 19 -- the two verify and sign identically here; they differ
 * in where the nonce comes from: THESE calls take it from the caller under either alg.  ec_dbign_sign_batch below runs DBIGN's generator
 * (__bign_determinitic_nonce) on the device, as ec_decdsa_sign_batch does for ECDSA.
 * Any other alg is a call-level error (-1, ecamd_last_error()).
 *   lengths  qlen = ceil(|q| / 8), l = qlen / 2 (integer division).  sigs: n x (l + qlen), s0 (l bytes) then s1 (qlen bytes),
 *            both LITTLE-ENDIAN, as the reference writes them (the digest read as a number and W's coordinates in the hash input
 *            are little-endian too).  privs and nonces are n x qlen BIG-ENDIAN, like every other signing call here.
 *   inputs   hash_type 0: n x stride digests H(m), stride = the digest length in 1 .. 128, as for ec_sig_verify_batch (the caller
 *            hashed).  hash_type 1 .. 4 (SHA-224 / 256 / 384 / 512) or ECAMD_HASH_BELT (16): message slots in the format of
 *            ec_ecdsa_verify_msg_batch_fmt -- a little-endian u32 length, then the message; stride a multiple of 4 in 4 .. 4096 --
 *            and the device computes H(m) first.  bign256v1 with belt-hash is the standard's own configuration.  A slot whose
 *            length does not fit the stride is result / status 1.  Any other hash_type is a call-level error.
 *   oid      the OID octets of the message's hash (NOT libecc's adata framing oid_len || t_len || oid || t), the same for all items,
 *            a HOST pointer in the _dev forms too; oid_len in 0 .. 64, otherwise (or oid NULL with oid_len > 0) a call-level error.
 * Per item, verification is ec_pub_key_import_from_aff_buf + ec_verify with result[i] = 0 / 1 for 0 / -1, for every input
 * (sig/bign_common.c:742-962): s1 < q (s0 has no range check); hbar = the whole digest, little-endian, mod q; u = s1 + hbar (0 is
 * legal), v = s0 + 2^(8l); W = [u]G + [v]Y not at infinity; t = the first min(l, 32) bytes of
 * belt-hash(oid || first 2l bytes of LE(W.x) || LE(W.y) || digest), zero-padded to l bytes; accept iff t = s0 over all l bytes (on a
 * 521-bit order l = 33: byte 32 of an acceptable s0 is 0).  On cofactor curves the key import's subgroup check applies.
 * Signing is _ec_sign with the nonce k supplied by the caller (sig/bign_common.c:468-690): x < q (x = 0 signs), k in [1, q - 1],
 * W = [k]G, s0 = t as above, s1 = (k - hbar - (s0 + 2^(8l)) x) mod q.  No restart, no test of s1.  status[i] = 1 with zero signature
 * bytes otherwise.  Verification multiplies by public values only; signing's [k]G honours ecamd_ctx_set_secret_scalars (belt-hash's
 * inputs are public: W is recomputed by every verifier), and ecamd_ctx_wipe_scratch covers the staged W, slots and digests.
 * Chunking by ecamd_ctx_set_max_chunk, n = 0, NULL arguments and a handle of another context behave as for ec_sig_hashed_*. */
#define ECAMD_SIG_BIGN 18
#define ECAMD_SIG_DBIGN 19
#define ECAMD_HASH_BELT 16
int ec_bign_verify_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *pubkeys_aff,
			 const uint8_t *sigs, const uint8_t *inputs, uint32_t stride, const uint8_t *oid, uint32_t oid_len, uint8_t *result);
int ec_bign_sign_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *privs,
		       const uint8_t *nonces, const uint8_t *inputs, uint32_t stride, const uint8_t *oid, uint32_t oid_len, uint8_t *sigs,
		       uint8_t *status);
/* nn_get_random_mod (nn/nn_rand.c:92-150) given its random bytes.  The reference draws 2 * qlen bytes with get_random straight into the
 * limb array of an nn (they read as a little-endian integer on the little-endian hosts libecc and this library run on), reduces modulo
 * q - 1 and adds one.  raw: n x 2*qlen bytes from the caller's own randomness source; out: n x qlen big-endian, each in [1, q - 1].  The
 * reduction is libecc's constant-time division on the host otherwise -- about a microsecond of a host thread per value. */
int ec_nn_random_mod_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *raw, uint8_t *out);
/* ec_ecdsa_sign_batch from MESSAGES and RAW nonce material: per item k = the nn_get_random_mod value of its 2*qlen random bytes (what
 * __ecdsa_sign_finalize draws through ctx->rand = nn_get_random_mod, sig/ecdsa_common.c:424-470), h = SHA-224 / 256 / 384 / 512 of its
 * message slot (hash_type 1 .. 4; slots as for ec_ecdsa_verify_msg_batch_fmt), or hash_type 0: the slots are the digests themselves,
 * msg_stride bytes each.  Signature bytes equal those of ec_ecdsa_sign_batch fed with the reduced nonces and the digests. */
int ec_ecdsa_sign_msg_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *privs, const uint8_t *nonce_raw,
			    int hash_type, const uint8_t *msg_slots, uint32_t msg_stride, uint8_t *sigs, uint8_t *status);
/* Deterministic ECDSA (DECDSA, libecc's ec_alg_type 14): the nonce of RFC 6979 section 3.2 derived ON THE DEVICE, as the reference's
 * __ecdsa_rfc6979_nonce runs it (sig/ecdsa_common.c:48-169, called from __ecdsa_sign_finalize at :450), HMAC through the hash of the
 * message (hmac/hmac.c).  hash_type 1 .. 4 (SHA-224 / 256 / 384 / 512, libecc's hash_alg_type numbers) names BOTH the message hash and
 * the HMAC, as in libecc; any other value is a call-level error (-1, ecamd_last_error()).
 *   ec_rfc6979_nonce_batch   privs n x qlen big-endian (int2octets(x) is these octets as given: nn_export_to_buf of the imported key,
 *            :77), digests n x hsize (h1 = H(m), hsize = 28 / 32 / 48 / 64); nonces n x qlen big-endian.  V = 01.., K = 00..;
 *            bits2octets(h1) = the digest as a big-endian integer, >> (8 hsize - qbits) when longer, mod q (:89-94); steps d - g (:78-116);
 *            step h: V = HMAC_K(V) appended to T until 8 |T| >= qbits, k = the first qlen octets of T >> (8 qlen - qbits), accepted iff
 *            k < q, otherwise K = HMAC_K(V || 00), V = HMAC_K(V) and again (:136-165).  As in the reference k = 0 is NOT rejected here (the
 *            signing step refuses it).  status[i] = 0; 1 with a zero nonce only after 1000 rejected candidates, which no libecc curve
 *            reaches (none rejects more than half).  The nonces are SECRET: this call hands them to the caller, who owns their wiping.
 *   ec_decdsa_sign_batch     ec_key_pair_import_from_priv_key_buf + _ec_sign(DECDSA) per item (sig/sig_algs.c, sig/decdsa.c:46-90).
 *            in_is_digest = 0: `in` holds message slots as for ec_ecdsa_sign_msg_batch (u32 length + bytes, in_stride a multiple of 4 in
 *            4 .. 4096), hashed on the device; a slot whose length does not fit the stride is status 1.  in_is_digest = 1: `in` is
 *            n x hsize digests and in_stride must equal hsize.  Anything else is a call-level error.  Then the nonce as above, into a
 *            scratch buffer that never leaves the device (wiped when it is freed and by ecamd_ctx_wipe_scratch, like the nonces of
 *            ec_ecdsa_sign_msg_batch), then ec_ecdsa_sign_batch's core: signature bytes and status are those of ec_ecdsa_sign_batch fed with
 *            the derived k.  Key rules are ec_ecdsa_sign_batch's, which are the reference's (recorded in tests/golden/decdsa.json): x = 0
 *            imports and signs, x >= q does not import -- status 1, zero bytes.  The reference RESTARTS on r = 0, e = x r or s = 0
 *            (:492, :516, :548) and would derive the same k for ever; here that is status 1 with zero bytes.
 * [k]G honours ecamd_ctx_set_secret_scalars; the nonce kernel looks nothing up by a secret and branches on one only in the RFC's own
 * retry.  Chunking by ecamd_ctx_set_max_chunk, n = 0 (returns 0, touches nothing), NULL arguments and a handle of another context
 * (-1) as for ec_ecdsa_sign_batch.  Orders of at most 528 bits (qlen <= 66). */
int ec_rfc6979_nonce_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs,
			   const uint8_t *digests, uint8_t *nonces, uint8_t *status);
int ec_decdsa_sign_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *in,
			 uint32_t in_stride, int in_is_digest, uint8_t *sigs, uint8_t *status);
/* HMAC and deterministic ECDSA over the WHOLE hash table: libecc's hmac() (hash/hmac.c) and _ec_sign(DECDSA) with any fixed-length hash
 * of hash_alg_type, where the HMAC of __ecdsa_rfc6979_nonce runs through the hash of the message.  Unlike the digest-first schemes this
 * cannot be composed from ec_digest_slots_batch: the HMAC sits between the private key and the multiplication.
 *   hash_type  the set of ec_digest_slots_batch: 1 .. 11, 13 .. 15, 17 .. 20.  0, 12 (SHAKE256), 16 (belt-hash) and anything else is a
 *              call-level error (-1, ecamd_last_error()).  The HMAC's block sizes are libecc's block_size fields: 64 / 64 / 128 / 128
 *              (SHA-2), 144 / 136 / 104 / 72 (SHA-3), 128 (SHA-512/t), 64 (SM3, Streebog, RIPEMD-160), 136 / 128 / 96 / 64 (BASH).
 *   ec_hmac_slots_batch   macs[i] = HMAC(key i, message i), n x ecamd_digest_len(hash_type) octets.  Keys and messages are slots in the
 *              format of ec_digest_slots_batch (a little-endian u32 length, then the bytes), key_stride and stride multiples of 4 in
 *              4 .. 4096.  A key longer than the block is hashed first, as in hmac_init.  A key slot or a message slot that does not
 *              fit its stride gets an all-zero MAC (ec_digest_slots_batch's rule).
 *   ec_rfc6979_nonce_ht_batch, ec_decdsa_sign_ht_batch   ec_rfc6979_nonce_batch and ec_decdsa_sign_batch, argument for argument, for
 *              every hash_type above: digests n x hsize with hsize = ecamd_digest_len(hash_type) (20 for RIPEMD-160: T then takes
 *              ceil(qlen / 20) values of V, four on a 521-bit order); in_is_digest with in_stride = hsize; message slots hashed on the
 *              device by the kernels of ec_digest_slots_batch; a slot that does not fit is status 1 with zero bytes; x = 0 signs,
 *              x >= q is status 1; the reference's restart conditions are status 1; qlen <= 66; the derived nonces stay in a wiped
 *              scratch buffer.  hash_type 1 .. 4 run the kernel of the older names: the same bytes at the same speed.  The older
 *              names keep refusing 5 .. 20.  A signature verifies by the composition documented at ec_digest_slots_batch:
 *              ec_digest_slots_batch_dev, then ec_ecdsa_verify_batch_dev.
 * SECRET-SCALAR MODE.  Streebog's table look-ups are indexed by state octets, and in these three calls the state depends on the HMAC
 * key or the private key.  A scan of a 16 KiB table per look-up is not offered: after ecamd_ctx_set_secret_scalars(ctx, 1) all three
 * calls (and their _dev forms) refuse hash_type 13 and 14 with a call-level -1, and ecamd_last_error() says why.  Every other served
 * hash looks nothing up by data; its kernels are the same in both modes.  [k]G honours the mode as in ec_decdsa_sign_batch.
 * n = 0 (returns 0, touches nothing), NULL arguments, a handle of another context (-1) and chunking by ecamd_ctx_set_max_chunk as for
 * ec_decdsa_sign_batch; the _dev forms take device pointers and only enqueue on hip_stream (NULL: the context's stream).
 * Out of scope: the ecamd_multi_* wrappers, the libecc-typed layer (libsign_amd) and belt-hash; the commitment schemes (ECSDSA,
 * ECOSDSA, ECKCDSA, BIP0340, ECFSDSA) have their own _ht names below. */
int ec_hmac_slots_batch(ecamd_ctx *ctx, int hash_type, uint32_t n, const uint8_t *key_slots, uint32_t key_stride,
			const uint8_t *msg_slots, uint32_t stride, uint8_t *macs);
int ec_hmac_slots_batch_dev(ecamd_ctx *ctx, int hash_type, uint32_t n, const void *d_key_slots, uint32_t key_stride,
			    const void *d_msg_slots, uint32_t stride, void *d_macs, void *hip_stream);
int ec_rfc6979_nonce_ht_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs,
			      const uint8_t *digests, uint8_t *nonces, uint8_t *status);
int ec_rfc6979_nonce_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs,
				  const void *d_digests, void *d_nonces, void *d_status, void *hip_stream);
int ec_decdsa_sign_ht_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *in,
			    uint32_t in_stride, int in_is_digest, uint8_t *sigs, uint8_t *status);
int ec_decdsa_sign_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs, const void *d_in,
				uint32_t in_stride, int in_is_digest, void *d_sigs, void *d_status, void *hip_stream);
/* Deterministic BIGN (DBIGN, libecc's ec_alg_type 19) with the nonce of STB 34.101.45 section 6.3.3 derived ON THE DEVICE, as the
 * reference's __bign_determinitic_nonce runs it (sig/bign_common.c:200-342), its non-standard choices included.
 *   ec_dbign_nonce_batch   privs n x qlen big-endian, digests n x digest_len (H(m), digest_len in 1 .. 128); nonces n x qlen big-endian.
 *            theta = belt-hash(oid || the first 2 l octets of the key written to qlen octets and byte-reversed || t), l = qlen / 2 (an odd
 *            qlen -- 29, 66 -- drops the key's top octet); r = the digest, zero-padded; n = digest_len / 16, raised to 2 when it is 0 or 1;
 *            i = 1, 2, ..: s = r_1 ^ .. ^ r_(n-1), the first n - 2 blocks move left, r_(n-1) = F_theta(s) ^ r_n ^ <i>_128, r_n = s; the
 *            candidate is the first qlen octets of r, little-endian, cut to the bits of q when qlen < 16 n, and the first 16 n octets
 *            otherwise; accepted when i >= 2 n and 0 < k < q.  status[i] = 0; 1 with a zero nonce only after 1000 candidates rejected at
 *            i >= 2 n (the reference goes on until i wraps; the worst libecc order rejects 15 in 16).  The nonces are SECRET: the caller
 *            owns their wiping.
 *   ec_dbign_sign_batch    ec_key_pair_import_from_priv_key_buf + _ec_sign(DBIGN) per item.  hash_type, inputs, stride and oid follow
 *            ec_bign_sign_batch's rules.  t: STB's optional additional data, the same for all items, a HOST pointer in the _dev form too;
 *            t_len in 0 .. 64, otherwise (or t NULL with t_len > 0) a call-level error.  Per chunk: the digests, the nonces into a scratch
 *            buffer that never leaves the device (wiped when freed and by ecamd_ctx_wipe_scratch), then ec_bign_sign_batch's core:
 *            bytes and status are those of ec_bign_sign_batch fed with the derived k; its key rules too (x < q, x = 0 signs).
 * UNLIKE everything else BelT does here, the generator's substitution indices depend on the private key.  In the default mode the
 * kernel gathers from a table in LDS; after ecamd_ctx_set_secret_scalars(ctx, 1) every look-up reads the whole table at addresses that
 * do not depend on the index.  Both give the same bytes.  n = 0, NULL arguments, a handle of another context, a bad hash_type or
 * stride and chunking behave as for ec_decdsa_sign_batch.  Orders of at most 528 bits (qlen <= 66). */
int ec_dbign_nonce_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *privs, const uint8_t *digests,
			 uint32_t digest_len, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, uint8_t *nonces,
			 uint8_t *status);
int ec_dbign_sign_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *inputs,
			uint32_t stride, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, uint8_t *sigs,
			uint8_t *status);
/* BIP0340 signing with the semi-deterministic nonce derived ON THE DEVICE, as _bip0340_sign runs it (sig/bip0340.c:213-294).  hash_type
 * 1 .. 4 (the reference does not fix BIP0340 to SHA-256) is the hash of both tagged hashes and of the challenge.  privs, pubkeys_aff
 * (NULL: Y = [x]G on the device), hash_slots and stride are exactly ec_schnorr_sign_batch's for BIP0340.
 *   aux      n x qlen big-endian, REQUIRED: the value libecc draws below 2^(8 qlen) through its `rand` hook.  All-zero is legal.
 *   nonce    d = x, or q - x when Y.y is odd; mask = H(H(tag_aux) || H(tag_aux) || aux); t = d ^ mask over max(qlen, hsize) octets (the
 *            reference's two length cases); k = OS2I(H(H(tag_nonce) || H(tag_nonce) || t || Y.x || m)) mod q over the whole digest, m being
 *            the slot's bytes behind its fixed fields.  status 1 with a zero nonce: x = 0 or x >= q, a key that does not import, k = 0,
 *            a slot that does not hold the fixed fields or does not fit the stride.
 *   ec_bip0340_nonce_batch   hands the SECRET nonces (n x qlen big-endian) to the caller, who owns their wiping.
 *   ec_bip0340_sign_batch    Y, then the nonce into a scratch buffer that never leaves the device, then ec_schnorr_sign_batch's core:
 *            signature bytes (clen + qlen) and status are those of ec_schnorr_sign_batch fed with that k.
 * The generator looks nothing up by a secret; [k]G and [x]G honour ecamd_ctx_set_secret_scalars.  n = 0, NULL arguments (aux
 * included), a handle of another context, a bad hash_type or stride and chunking behave as for ec_decdsa_sign_batch. */
int ec_bip0340_nonce_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs,
			   const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *nonces,
			   uint8_t *status);
int ec_bip0340_sign_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs,
			  const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
			  uint8_t *status);
/* ECKCDSA / ECSDSA / ECOSDSA / ECFSDSA / BIP0340 OVER THE WHOLE HASH TABLE.  These five schemes hash AFTER their multiplication: the
 * hash input holds the commitment (r = H(Wx || Wy || m), H(Wx || m), H(FE2OS(Wx)); e = H(Wx || Wy || m); e = H(H(tag) || H(tag) || r ||
 * Yx || m) and the two tagged hashes of BIP0340's nonce), which exists only inside the call, so they cannot be composed from
 * ec_digest_slots_batch the way ECDSA, BIGN, ECGDSA, ECRDSA and SM2 can.  The reference sets no limit on the hash beyond
 * digest_size <= MAX_DIGEST_SIZE and block_size <= MAX_BLOCK_SIZE (sig/ecsdsa_common.c:79, sig/eckcdsa.c:90, sig/ecfsdsa.c:68,
 * sig/bip0340.c:143).  Each name below is the name without _ht, argument for argument: slot formats, blanks, status and result rules,
 * chunking, n = 0, NULL and foreign-handle behaviour are those documented there.  What differs:
 *   hash_type  the set of ec_digest_slots_batch: 1 .. 11, 13 .. 15, 17 .. 20.  0, 12 (SHAKE256), 16 (belt-hash) and anything else is a
 *              call-level error (-1, ecamd_last_error()).
 *   lengths    hsize = ecamd_digest_len(hash_type), 20 for RIPEMD-160.  ECSDSA / ECOSDSA: r_len = hsize; ECKCDSA: r_len = min(hsize,
 *              qlen) -- with hsize < qlen (RIPEMD-160 on every curve here, any 64-octet hash on a 521-bit order) r is the whole digest
 *              and nothing is truncated.  Signatures are r_len + qlen octets.  ECKCDSA's inputs are digests h = H(z || m) of hsize
 *              octets (stride = hsize).  BIP0340's slot carries 2 hsize octets of tag hashes in front of r.  e is the WHOLE digest mod q
 *              for every hsize beside every qlen.
 *   1 .. 4     run the kernels the names without _ht run: the same bytes at the same speed.  Those names keep refusing 5 .. 20.
 *   ec_bip0340_nonce_ht_batch, ec_bip0340_sign_ht_batch   t = (d || 0 ..) ^ (mask || 0 ..) over max(qlen, hsize) octets (hsize 20 beside
 *              qlen 66 at the extreme); both tagged hashes and the challenge use hash_type.
 * ECKCDSA from messages without leaving the device.  z is the first BLOCK octets (libecc's block_size of the hash: 64 / 64 / 128 / 128
 * SHA-2, 144 / 136 / 104 / 72 SHA-3, 128 SHA-512/t, 64 SM3, Streebog, RIPEMD-160, 136 / 128 / 96 / 64 BASH) of the caller's own
 * public-key octets Yx || Yy, zero-padded when 2 clen < BLOCK.  The caller lays out slots `u32 length | z | m`, runs
 * ec_digest_slots_batch_dev(ctx, hash_type, n, d_slots, stride, d_h, stream) and hands d_h to
 * ec_sig_hashed_verify_ht_batch_dev(ctx, curve, ECAMD_SIG_ECKCDSA, hash_type, n, d_pubkeys, d_sigs, d_h, hsize, d_result, stream) (or to
 * the signing call) on the same stream: h never leaves device memory.
 * SECRET-SCALAR MODE.  ec_bip0340_nonce_ht_batch and ec_bip0340_sign_ht_batch (and their _dev forms) refuse Streebog (hash_type 13, 14)
 * after ecamd_ctx_set_secret_scalars(ctx, 1), with a call-level -1 and a message: the nonce hash absorbs t, which depends on the private
 * key, and Streebog indexes its table by state octets.  Every other call here accepts Streebog in either mode and gives the same bytes
 * in both: it hashes commitments and messages only, which a verifier recomputes.  No other served hash looks anything up by data.
 * [k]G and [x]G honour the mode as in the names without _ht.
 * Out of scope: the whole-batch forms ec_schnorr_verify_all_batch / ec_schnorr_verify_msg_all_batch (SHA-2 only; they answer "valid" or
 * "not decided", and the item form here gives the verdict), the ecamd_multi_* wrappers, the libecc-typed layer (libsign_amd), belt-hash
 * and SHAKE256 as commitment hashes. */
int ec_sig_hashed_verify_ht_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n,
				  const uint8_t *pubkeys, const uint8_t *sigs, const uint8_t *inputs, uint32_t stride, uint8_t *result);
int ec_sig_hashed_sign_ht_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *privs,
				const uint8_t *nonces, const uint8_t *inputs, uint32_t stride, uint8_t *sigs, uint8_t *status);
int ec_schnorr_verify_ht_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *keys, int key_fmt,
			       const uint8_t *sigs, const uint8_t *hash_slots, uint32_t stride, uint8_t *result);
int ec_schnorr_sign_ht_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const uint8_t *privs,
			     const uint8_t *pubkeys_aff, const uint8_t *nonces, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
			     uint8_t *status);
int ec_bip0340_nonce_ht_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs,
			      const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *nonces,
			      uint8_t *status);
int ec_bip0340_sign_ht_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const uint8_t *privs,
			     const uint8_t *pubkeys_aff, const uint8_t *aux, const uint8_t *hash_slots, uint32_t stride, uint8_t *sigs,
			     uint8_t *status);
int ec_sig_hashed_verify_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_pubkeys,
				      const void *d_sigs, const void *d_inputs, uint32_t stride, void *d_result, void *hip_stream);
int ec_sig_hashed_sign_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_privs,
				    const void *d_nonces, const void *d_inputs, uint32_t stride, void *d_sigs, void *d_status, void *hip_stream);
int ec_schnorr_verify_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_keys, int key_fmt,
				   const void *d_sigs, const void *d_hash_slots, uint32_t stride, void *d_result, void *hip_stream);
int ec_schnorr_sign_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_privs,
				 const void *d_pubkeys_aff, const void *d_nonces, const void *d_hash_slots, uint32_t stride, void *d_sigs,
				 void *d_status, void *hip_stream);
int ec_bip0340_nonce_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs,
				  const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots, uint32_t stride, void *d_nonces,
				  void *d_status, void *hip_stream);
int ec_bip0340_sign_ht_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs,
				 const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots, uint32_t stride, void *d_sigs,
				 void *d_status, void *hip_stream);
/* ec_key_pair_gen's generic rule (sig/ec_key.c:594-610): x = nn_get_random_mod(q) from the item's 2*qlen random bytes, Y = [x]G.
 * priv_out: n x qlen big-endian; pub_out: n x 2*clen affine X || Y; status as ec_prj_pt_mul_batch.  (Secret scalars: see
 * ecamd_ctx_set_secret_scalars; the private keys cross the bus on their way back, as supplied ones do on their way in.) */
int ec_key_pair_gen_raw_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *raw, uint8_t *priv_out,
			      uint8_t *pub_out_aff, uint8_t *status);
/* ECC-CDH, batch form of ecccdh_derive_secret (ecdh/ecccdh.c:167): privs n x qlen, peers n x 2*clen
 * affine, secrets n x clen (x coordinate of d*Q), status[i] = 0 ok / 1 the reference returns -1.
 * Cofactor curves: subgroup check of the peer key and the [h]Q step as in the reference. */
int ec_ecccdh_derive_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *privs,
			   const uint8_t *peers_aff, uint8_t *secrets, uint8_t *status);

/* X25519 / X448, batch form of x25519() / x448() (ecdh/x25519_448.c:380-425): curve must be WEI25519
 * (32-byte strings) or WEI448 (56-byte strings), the Weierstrass models libecc itself computes on.
 * k, u, out: n x len little-endian (RFC 7748 wire format).  status[i] = 1 where the reference returns
 * -1: non-canonical u (>= p), u on the twist, small-order point, zero result (libecc deliberately
 * rejects these, x25519_448.c:219-276). */
int ec_xdh_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *k, const uint8_t *u,
		 uint8_t *out, uint8_t *status);

/* EdDSA verification, batch form of eddsa_import_pub_key (sig/eddsa.c:862) + ec_verify (_eddsa_verify_init :1846,
 * _eddsa_verify_finalize :2130), on the Weierstrass models libecc itself computes on:
 *   curve = WEI25519: EDDSA25519 / EDDSA25519CTX / EDDSA25519PH.  pubkeys n x 32 (RFC 8032 encoding of A), sigs n x 64
 *     (R || S), hram n x 64 = SHA-512(dom2 || R || A || PH(M)), hram_len = 64;
 *   curve = WEI448:   EDDSA448 / EDDSA448PH.  pubkeys n x 57, sigs n x 114, hram n x 114 =
 *     SHAKE256(dom4 || R || A || PH(M), 114), hram_len = 114.
 * The hash is computed by the caller (the variants differ only in that hash input).  Note for Ed448: libecc stores
 * [4^-1 mod q]A and hashes the key RE-ENCODED from it, which differs from the given bytes when A has a torsion
 * component; hash those bytes to reproduce it (for keys in the prime-order subgroup they are the key itself).
 * result[i] = 0 accept / 1 where the reference returns -1: non-canonical or undecodable A or R, the neutral point,
 * S >= q, [cofactor]A = infinity, or [cofactor]([S]G - R - [h]A) != infinity (libecc checks the cofactored equation). */
int ec_eddsa_verify_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *pubkeys,
			  const uint8_t *sigs, const uint8_t *hram, uint32_t hram_len, uint8_t *result);

/* Whole-batch predicate of ec_verify_batch (sig/sig_algs.c:675; eddsa_verify_batch sig/eddsa.c:2904,
 * _eddsa_verify_batch_no_memory :2278) for the EdDSA variants: *all_valid = 1 iff libecc's batch verification accepts.
 * libecc rejects num = 0, as this does (-1).  first_rejected (may be NULL) receives the lowest rejected index, n if none --
 * the reference gives no such hint and callers re-verify one by one.  Same inputs as ec_eddsa_verify_batch.
 *   Ed25519 batches of at least 2^17 items (ecamd_ctx_set_eddsa_msm): the reference's own equation
 *     [8]([-sum z_i S_i]B + sum [z_i h_i]A_i + sum [z_i]R_i) = 0, z_i 128 random bits (ChaCha20 on the device, keyed by 32
 *     bytes of getrandom per call), after the reference's per-item rejections (decoding, S >= q, [8]A_i = 0) -- evaluated as
 *     ONE multi-scalar multiplication on the Edwards curve (Straus, the 256 doublings shared by up to 8 signatures per lane).
 *     Like libecc's, this test accepts a batch with a bad signature with probability ~2^-128.  A batch it rejects is then
 *     verified item by item, which yields first_rejected.
 *   Ed448 batches of at least 2^17 items (round 6): the same equation on the Weierstrass model WEI448 the reference computes on -- A_i, R_i
 *     decoded as for ec_eddsa_verify_batch, the Schnorr-type combination [sum z_i S_i]G + sum [z_i (q - h_i)]A_i - sum [z_i]R_i on the
 *     Goldilocks unit (buckets of 16-bit windows; the Straus loop below 2^17 items when ecamd_ctx_set_eddsa_msm says "always"), and the
 *     final test cofactored, [4](...) = infinity, as every point of the reference's combination enters multiplied by the cofactor
 *     (sig/eddsa.c:2580-2860).  [4] kills the torsion components, so the scalars may be taken mod q and the key may be the decoded A
 *     (libecc stores [4^-1 mod q]A); a key with [4]A = infinity, an undecodable key or commitment, S >= q, and a commitment that
 *     decodes to the neutral element (no affine Weierstrass form; the item form accepts it) make the combination "not decided" and
 *     the items are verified one by one.  Measured: 26 ms per 2^20 signatures against 70 ms item by item (profiles/r6_ed448_msm.md).
 *   otherwise (small batches): every item is verified; the bit is the exact conjunction. */
int ec_eddsa_verify_all_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *pubkeys,
			      const uint8_t *sigs, const uint8_t *hram, uint32_t hram_len, int *all_valid,
			      uint32_t *first_rejected);

/* Whole-batch predicate of ec_verify_batch for the Schnorr-type algorithms libecc verifies in batches on a short-Weierstrass curve --
 * BIP0340 (bip0340_verify_batch sig/bip0340.c:1296, _bip0340_verify_batch_no_memory :808-1025, _bip0340_verify_batch :1027-1294) and
 * ECFSDSA (ecfsdsa_verify_batch sig/ecfsdsa.c:1057, _ecfsdsa_verify_batch_no_memory :657-837) -- as ONE multi-scalar multiplication.  The item form of both is  [s_i]G + [q - e_i]Y_i = R_i  (bip0340.c:531-547,
 * ecfsdsa.c:561-576); the reference's batch form draws scalars a_i and accepts when
 *     [-sum a_i s_i]G + sum [a_i]R_i + sum [a_i e_i]Y_i   is the point at infinity (bip0340.c:925-1002).
 * Here: z_i = 128 bits of ChaCha20 (keyed by 32 bytes of getrandom per call, or ecamd_ctx_set_msm_seed), and
 *     T = [sum z_i s_i]G + sum ([z_i ne_i mod q]Y_i - [z_i]R_i),     *all_valid = 1 iff T is the point at infinity
 * evaluated on the radix-2^29 unit of the curve by a Straus loop whose doublings are shared by up to 8 signatures per lane (the R_i
 * only enter the low 33 windows).  s, ne: n x qlen big-endian, ne_i = q - e_i mod q as the item form multiplies it; keys_aff: n x 2*clen,
 * the keys Y_i as the item form uses them (BIP0340: after lift_x); r: r_fmt 0 = n x 2*clen affine points R_i (ECFSDSA: the signature's
 * W), r_fmt 1 = n x clen x coordinates, R_i = the point with that x and an EVEN y (BIP0340: lift_x of r_i, computed on the device;
 * fields with p = 3 mod 4).
 * *all_valid = 0 means "not decided here": some item fails the equation, or a point does not import / r_i is no abscissa / s_i >= q /
 * an addition met equal or opposite operands, or the handle has no such unit (ec_schnorr_verify_all_available) -- the caller then
 * verifies item by item, so the batch form never accepts or rejects anything the item form would not (a batch with a bad
 * signature passes with probability ~2^-128, as the reference's does).  That bound needs a group of PRIME order: on a curve with a
 * cofactor a commitment shifted by a point D of small order passes the combination whenever z_i D = O (probability 1 / ord(D)), so
 * handles with cofactor != 1 (WEI25519, WEI448) are never served -- ec_schnorr_verify_all_available is 0 and *all_valid stays 0
 * (the reference's own batch form has that weakness; a loop of ec_verify does not, and this form must not differ from the loop).
 * libecc rejects num = 0, as this does (-1). */
int ec_schnorr_verify_all_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *s, const uint8_t *ne,
				const uint8_t *keys_aff, const uint8_t *r, int r_fmt, int *all_valid);
int ec_schnorr_verify_all_available(const ecamd_curve *curve, int r_fmt);   /* 1: the multi-scalar form serves this handle */
/* The same verdict FROM keys, signatures and hash inputs (round 6) -- what an ec_verify_batch of BIP0340 / ECFSDSA signatures needs so that
 * only marshalling stays on the host.  keys: n points in key_fmt (ECAMD_PT_AFFINE X || Y or ECAMD_PT_PROJECTIVE X || Y || Z, what an
 * ec_pub_key holds; imported and normalised on the device); sigs: n x (rlen + qlen), the commitment then s, rlen = clen for r_fmt 1
 * (BIP0340: r, an abscissa) and 2 * clen for r_fmt 0 (ECFSDSA: the point W); hash_slots: per item a little-endian u32 length and the
 * scheme's hash input (stride a multiple of 4, at most 4096): for BIP0340  H(tag) || H(tag) || r || <blank of clen octets> || m  with
 * x_offset the blank's offset in the input -- the device writes the x of the key's unique representative there (sig/bip0340.c:437-494)
 * -- and for ECFSDSA  W.x || W.y || m  with x_offset = 0xffffffff (sig/ecfsdsa.c:520-540); hash_type 1 .. 4 (SHA-224 .. SHA-512).  The
 * device computes e = H(input) mod q and q - e, takes the key's even-y representative for r_fmt 1 (lift_x, bip0340.c:532-535), and
 * evaluates ec_schnorr_verify_all_batch's combination over the whole batch once the last chunk has arrived.  *all_valid = 0: not
 * decided here -- also when a key does not import or is the point at infinity.
 * A batch of one piece (n <= max_chunk) evaluated by buckets is FILED CHUNK BY CHUNK: the points' import, the scalars z_i, z_i (q - e_i)
 * and the filing of every staging chunk (2^17 items) run while the next chunk is on its way, and only the bucket sums and their reduction
 * wait for the last one; z_i is keyed by the item's index in the batch, so the verdict does not depend on the chunking
 * ($ECAMD_NO_SCHNORR_STREAM: the whole combination after the last chunk). */
int ec_schnorr_verify_msg_all_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *keys, int key_fmt,
				    const uint8_t *sigs, int r_fmt, int hash_type, const uint8_t *hash_slots, uint32_t stride,
				    uint32_t x_offset, int *all_valid);
/* The same combination on device pointers, one piece (n <= the context's max_chunk; a handle for which ec_schnorr_verify_all_available
 * is 0 is an error here): d_verdict[0] = 0 "the batch is valid" / 1 "not decided here".  Only enqueues on the stream. */
int ec_schnorr_verify_all_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_s, const void *d_ne,
				    const void *d_keys_aff, const void *d_r, int r_fmt, void *d_verdict, void *hip_stream);

/* eddsa_export_pub_key in batch (sig/eddsa.c:795-860): n projective Weierstrass points X || Y || Z (what ec_pub_key.y holds,
 * prj_pt_export_to_buf) of the WEI25519 / WEI448 handle -> prj_pt_shortw_to_aff_pt_edwards -> eddsa_encode_point: n x 32 / 57
 * octets, the public-key encoding the verifier hashes.  status ECAMD_ERR for a point that is not on the curve; the point at
 * infinity encodes the neutral element (0, 1) as in the reference. */
int ec_eddsa_encode_point_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *points_prj,
				uint8_t *enc, uint8_t *status);

/* The multi-scalar multiplication alone, device pointers (WEI25519 handle, hram_len 64; WEI448 handle, hram_len 114: round 6; any n > 0):
 * d_verdict[0] = 0 when libecc's batch equation holds and no item is rejected beforehand, 1 otherwise ("not decided here").  Only
 * enqueues on the stream. */
int ec_eddsa_verify_all_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_pubkeys,
				  const void *d_sigs, const void *d_hram, uint32_t hram_len, void *d_verdict, void *hip_stream);

/* Ed25519 signing (EDDSA25519 / EDDSA25519CTX / EDDSA25519PH on the WEI25519 handle), the device-side steps of ec_sign ->
 * _eddsa_sign (sig/eddsa.c:1554-1870) around the caller's two hashes -- the split ec_eddsa_verify_batch uses:
 *   1. the caller derives (a, prefix) from each key (eddsa_get_digest_from_priv_key :306 + eddsa_derive_priv_key :611: SHA-512, clamping) and hashes
 *      r_hash = SHA-512(dom2 || prefix || PH(M))                                          n x 64 bytes
 *   2. ec_eddsa_sign_R_batch: r = r_hash mod q (:1731), R = prj_pt_mul(r, G) (:1776), prj_pt_shortw_to_aff_pt_edwards +
 *      eddsa_encode_point (:1786-1791) -> R_enc n x 32 (the first half of each signature).  status 1 only if the
 *      multiplication failed (it cannot for the generator); r = 0 mod q encodes the neutral element as the reference does.
 *   3. the caller hashes hram = SHA-512(dom2 || R || A || PH(M))                           n x 64 bytes
 *   4. ec_eddsa_sign_S_batch: S = (r + hram a) mod q (:1847-1857), a_scalars n x 32 little-endian (the clamped secret
 *      scalars) -> S_out n x 32 little-endian (the second half).
 * Ed448 (EDDSA448 / EDDSA448PH) on the WEI448 handle, same two calls: r_hash and hram are n x 114 (SHAKE256 with 114 bytes of
 * output), R_enc, a_scalars and S_out n x 57; the device multiplies the generator by r / 4 mod q and encodes through the 4-isogeny
 * back to Edwards448, as _eddsa_sign does (:1737-1746, eddsa_encode_point :350-395). */
int ec_eddsa_sign_R_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *r_hash, uint8_t *R_enc,
			  uint8_t *status);
int ec_eddsa_sign_S_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *r_hash, const uint8_t *hram,
			  const uint8_t *a_scalars, uint8_t *S_out);

/* One-call EdDSA signing, every hash on the device: eddsa_import_key_pair_from_priv_key_buf (sig/eddsa.c:1028) + _ec_sign ->
 * _eddsa_sign (:1554-1870) per item.  alg: libecc's ec_alg_type (lib_ecc_types.h:49-55) -- EDDSA25519 (9), EDDSA25519CTX (10),
 * EDDSA25519PH (11) on the WEI25519 handle (klen 32, SHA-512); EDDSA448 (12), EDDSA448PH (13) on the WEI448 handle (klen 57, SHAKE256
 * with 114 octets of output, 64 for EDDSA448PH's pre-hash).  Any other alg, or an alg on the other handle, is a call-level error (-1).
 *   secret_keys  n x klen, the RFC 8032 secret key octets.  Per item h = H(octets as given), clamped as eddsa_derive_priv_key does
 *                (:611-688, the clamp at :649-671); a = the first half little-endian, prefix = the second half.
 *   pubkeys      n x klen encodings of A, hashed as they are -- like _eddsa_sign, this form does NOT check that a public key belongs
 *                to its secret key --, or NULL: A = encode([a]B) is computed here, the way R is (Ed448: a / 4 on WEI448 and the
 *                4-isogeny, as eddsa_init_pub_key :840 does).
 *   adata        ONE context for the call, host memory in both forms, adata_len in 0 .. 255: dom2 / dom4 (:55-130).  EDDSA25519
 *                hashes no dom and ignores both arguments.  EDDSA25519CTX with adata == NULL (:1683) and adata_len > 255 (:64) are
 *                call-level errors.  adata == NULL elsewhere hashes OLEN and no octets, as :79 does.
 *   msg_slots    as ec_decdsa_sign_batch's: per item a little-endian u32 length, then the bytes; msg_stride a multiple of 4 in
 *                4 .. 4096.  A length that does not fit the stride: status 1 and zero signature bytes for that item only.  The PH
 *                variants compute PH(M) here.
 *   sigs         n x 2 klen, R || S.  pub_out (n x klen, or NULL): the encoding of A of every item (given or derived).
 *   status       0 signed; 1 where the reference returns -1: a bad slot (a failed generator multiplication cannot happen).
 *                r = 0 mod q signs with the neutral element's encoding, as ec_eddsa_sign_R_batch documents.
 * r_hash = H(dom || prefix || PH(M)) (:1679-1707) and H(dom || R || A || PH(M)) (:1782-1835) are streamed over their segments; the
 * prefix never leaves the registers.  a and r_hash lie in the context's scratch between the kernels: wiped when freed and by
 * ecamd_ctx_wipe_scratch, like the RFC 6979 nonces.  [r]B and [a]B honour ecamd_ctx_set_secret_scalars; chunks follow
 * ecamd_ctx_set_max_chunk.  n = 0 touches nothing.
 * ec_eddsa_pub_key_batch: eddsa_import_key_pair_from_priv_key_buf + eddsa_export_pub_key (:970) alone; status as
 * ec_eddsa_sign_R_batch's. */
int ec_eddsa_sign_msg_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const uint8_t *secret_keys,
			    const uint8_t *pubkeys, const uint8_t *adata, uint32_t adata_len, const uint8_t *msg_slots,
			    uint32_t msg_stride, uint8_t *sigs, uint8_t *pub_out, uint8_t *status);
int ec_eddsa_pub_key_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *secret_keys, uint8_t *pub_out,
			   uint8_t *status);

/* EdDSA from keys, signatures, a context and messages of ANY length, all five variants, through one call: what eddsa_import_pub_key +
 * ec_verify and _ec_sign take.  The messages lie in ec_digest_msgs_batch's packed array -- msgs, offsets (n + 1 uint64_t), msgs_len,
 * alignment, pieces of the host forms ($ECAMD_MSGS_CHUNK_BYTES) and n = 0 exactly as documented there -- and every hash runs on the
 * device, streamed over its segments: nothing is assembled, on the host or in device memory.
 *   alg, adata, adata_len   as for ec_eddsa_sign_msg_batch: alg 9, 10, 11 on the WEI25519 handle, 12, 13 on the WEI448 handle, anything
 *                else a call-level error (-1); ONE context per call, host memory in both forms, with the same call-level errors.
 *   ec_eddsa_verify_msgs_batch      pubkeys n x klen, sigs n x 2 klen (klen 32 / 57).  Per item
 *                hram = H(dom || R_i || A_i || M_i), or H(dom || R_i || A_i || PH(M_i)) for alg 11 and 13 (PH(M_i) never leaves the
 *                registers), with R_i read from sigs + i * 2 klen and A_i from pubkeys + i * klen where they lie; then
 *                ec_eddsa_verify_batch_dev's core on the same stream.  result[i] is that core's verdict; an unusable item is result 1.
 *                A is hashed AS GIVEN: exact for Ed25519; for Ed448 exact whenever the key lies in the prime-order subgroup (libecc
 *                stores [4^-1 mod q]A and hashes the key RE-ENCODED from it, which differs from the given octets when A has a torsion
 *                component -- the note at ec_eddsa_verify_batch).
 *   ec_eddsa_verify_msgs_all_batch  the same inputs, ec_verify_batch's one bit: the same hram launch in front of
 *                ec_eddsa_verify_all_batch[_dev], whose rules (n = 0 is an error, which batches go through the combination) hold.
 *                Host form: *all_valid, and first_rejected (may be NULL) as there.  _dev form: d_all_valid[0] = 1 when the combination
 *                accepts and no item is unusable, else 0 ("not decided here / rejected"); it needs a handle the combination serves.  An
 *                unusable item makes the batch rejected exactly as a bad signature does; in the host form it counts for first_rejected.
 *   ec_eddsa_sign_msgs_batch        ec_eddsa_sign_msg_batch with msgs / offsets in place of slots: secret_keys, pubkeys (or NULL: derived),
 *                sigs, pub_out (or NULL), status, the key expansion, [r]B, [a]B, the mod-q finish, the secret scratch and its wiping,
 *                secret-scalar mode and chunking unchanged.  An unusable item is status 1 with zero signature bytes.
 * An item is UNUSABLE when offsets[i] > offsets[i + 1], offsets[i + 1] > the array's length, or the longest input hashed for it exceeds
 * 2^28 octets (dom || R || A || M; the message alone for alg 11 and 13).  Nothing of msgs is read for such an item, and for a usable
 * one no octet outside [offsets[i], offsets[i + 1]) is read: 8-octet loads inside the message, single octets at its ends.
 * The _dev forms only enqueue, in pieces of at most ecamd_ctx_set_max_chunk items.  Out of scope: the ecamd_multi_* wrappers, the
 * libecc-typed layer and projective keys. */
int ec_eddsa_verify_msgs_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
			       const uint8_t *adata, uint32_t adata_len, const uint8_t *msgs, const uint64_t *offsets, uint8_t *result);
int ec_eddsa_verify_msgs_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const void *d_pubkeys, const void *d_sigs,
				   const uint8_t *adata, uint32_t adata_len, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
				   void *d_result, void *hip_stream);
int ec_eddsa_verify_msgs_all_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
				   const uint8_t *adata, uint32_t adata_len, const uint8_t *msgs, const uint64_t *offsets, int *all_valid,
				   uint32_t *first_rejected);
int ec_eddsa_verify_msgs_all_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const void *d_pubkeys, const void *d_sigs,
				       const uint8_t *adata, uint32_t adata_len, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
				       void *d_all_valid, void *hip_stream);
int ec_eddsa_sign_msgs_batch(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const uint8_t *secret_keys, const uint8_t *pubkeys,
			     const uint8_t *adata, uint32_t adata_len, const uint8_t *msgs, const uint64_t *offsets, uint8_t *sigs,
			     uint8_t *pub_out, uint8_t *status);
int ec_eddsa_sign_msgs_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const void *d_secret_keys, const void *d_pubkeys,
				 const uint8_t *adata, uint32_t adata_len, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
				 void *d_sigs, void *d_pub_out, void *d_status, void *hip_stream);

/* Point wire formats (curves/prj_pt.c:462-624): affine X || Y (2*clen bytes, what the entry points above
 * use) and projective X || Y || Z (3*clen bytes: prj_pt_import_from_buf / prj_pt_export_to_buf, the format
 * of `ec_utils scalar_mult` and of structured public keys). */
#define ECAMD_PT_AFFINE 0
#define ECAMD_PT_PROJECTIVE 1
/* ec_prj_pt_mul_batch with a choice of formats: import (prj_pt_import_from_buf :462 or
 * prj_pt_import_from_aff_buf :511), prj_pt_mul, prj_pt_unique, export (prj_pt_export_to_buf :562 gives
 * X/Z || Y/Z || 1, or prj_pt_export_to_aff_buf :600).  Projective inputs: every coordinate < p and the
 * projective curve equation must hold; Z = 0 is the point at infinity (status ECAMD_INF); the degenerate
 * triple (0:0:0) passes the reference's import but fails in its ladder (status ECAMD_ERR). */
int ec_prj_pt_mul_batch_fmt(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *scalars,
			    uint32_t scalar_len, const uint8_t *points, int in_fmt, uint8_t *out, int out_fmt,
			    uint8_t *status);
/* prj_pt_import_from_[aff_]buf + prj_pt_unique / prj_pt_to_aff (:241, :218) + export: validates and
 * normalises n points (one inversion each on the device).  ECAMD_INF for Z = 0 (including (0:0:0),
 * which prj_pt_unique reports as infinity). */
int ec_prj_pt_unique_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *points, int in_fmt,
			   uint8_t *out, int out_fmt, uint8_t *status);

/* The group law, the on-curve test and the public-scalar multiplication in either wire format (round 4; SURVEY.md 8a rows a17, a18,
 * a21, a22 as callable batch operations).
 *   ec_prj_pt_op_batch_fmt: op ECAMD_PT_OP_ADD = prj_pt_add (curves/prj_pt.c:1204, the complete formulas of :971-1071; an
 *     "exceptional pair" -- the difference of the two points has order two, only possible on a curve of even order -- is the
 *     reference's -1, :1058-1060: ECAMD_ERR), ECAMD_PT_OP_DBL = prj_pt_dbl (:1132), ECAMD_PT_OP_ON_CURVE = prj_pt_is_on_curve (:144;
 *     status 0 on the curve / 1 not, out may be NULL).  Inputs as prj_pt_import_from_[aff_]buf takes them: every coordinate < p and
 *     the projective curve equation -- the reference's prj_pt_add / prj_pt_dbl do not test their operands, here a point off the
 *     curve is ECAMD_ERR; Z = 0 on the curve is the point at infinity, (0 : 0 : 0) included.  Output: the unique representative
 *     (prj_pt_unique: X / Z || Y / Z [|| 1]) or ECAMD_INF with zero bytes.
 *     (round 6) ECAMD_PT_OP_NEG = prj_pt_neg (:435): (X : -Y : Z), handed back as the unique representative like the sum.
 *     ECAMD_PT_OP_CMP = prj_pt_cmp (:303) and ECAMD_PT_OP_EQ_OR_OPP = prj_pt_eq_or_opp (:412) of p1[i] and p2[i]: `out` is ONE BYTE
 *     per item (out_fmt is ignored) -- CMP: 0 where the reference's *cmp is 0 (X1 Z2 = X2 Z1 and Y1 Z2 = Y2 Z1: the same point;
 *     like the reference no special case for Z = 0, so (0 : 0 : 0) compares equal to everything), 1 where it is not (the reference
 *     hands back the sign of a comparison of Montgomery residues in its word size; that sign is not reproduced); EQ_OR_OPP: the
 *     reference's *eq_or_opp, 1 for P = +-Q, else 0.  status 0, or ECAMD_ERR for an operand off the curve (out byte 0).
 *   ec_prj_pt_unprotected_mult_batch: _prj_pt_unprotected_mult (curves/prj_pt.c:1835-1880) statement for statement -- on-curve test,
 *     zero scalar -> infinity, out = in, then per bit below the top one a doubling and, when the bit is set, an addition whose
 *     exceptional pair is the call's -1 -- so that the batch form returns what the scalar function returns for EVERY public scalar
 *     and point (the window kernels return the same group element but never fail that way).  scalar_stride = scalar_len: one
 *     big-endian scalar per item; scalar_stride = 0: one scalar for every item, which is check_prj_pt_order (:1909) for PUBLIC_PT:
 *     "in_isorder is a multiple of the point's order" <=> status ECAMD_INF. */
#define ECAMD_PT_OP_ADD 0
#define ECAMD_PT_OP_DBL 1
#define ECAMD_PT_OP_ON_CURVE 2
#define ECAMD_PT_OP_NEG 3
#define ECAMD_PT_OP_CMP 4
#define ECAMD_PT_OP_EQ_OR_OPP 5
int ec_prj_pt_op_batch_fmt(ecamd_ctx *ctx, const ecamd_curve *curve, int op, uint32_t n, const uint8_t *p1, const uint8_t *p2, int in_fmt,
			   uint8_t *out, int out_fmt, uint8_t *status);
int ec_prj_pt_unprotected_mult_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *scalars, uint32_t scalar_len,
				     uint32_t scalar_stride, const uint8_t *points, int in_fmt, uint8_t *out, int out_fmt, uint8_t *status);

/* Structured public keys, batch form of ec_structured_pub_key_import_from_buf (sig/ec_key.c:312): each key is
 * 3 header bytes -- EC_PUBKEY (0), the ec_alg_type the key is for (ECDSA = 1, ...), libecc's ec_curve_type -- followed by
 * the projective X || Y || Z of ec_pub_key_export_to_buf.  Checks the header, imports (prj_pt_import_from_buf), checks the
 * subgroup on cofactor curves (ec_pub_key_import_from_buf :216) and hands back affine X || Y, the format the verification
 * entry points take.  status ECAMD_ERR where libecc returns -1, ECAMD_INF for a key that is the point at infinity (libecc
 * imports it; it has no affine form).  Built-in curves only (a user curve has no ec_curve_type). */
int ec_structured_pub_key_import_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *keys,
				       uint32_t key_len, int alg_type, uint8_t *out_aff, uint8_t *status);

/* Point decompression.  ec_aff_pt_y_from_x_batch is the batch form of aff_pt_y_from_x (curves/aff_pt.c:102): x n x clen big-endian ->
 * the two roots y1, y2 (n x clen each) of x^3 + a x + b IN THE REFERENCE'S ORDER -- y1 is the root its fp_sqrt (fp/fp_sqrt.c:107,
 * Tonelli-Shanks with the smallest non-residue) returns first, y2 = p - y1 (both 0 when the right-hand side is 0); status 1 where
 * the reference returns -1 (x >= p, not a square).  ec_point_decompress_batch takes SEC 1 compressed points (n x (1 + clen): 0x02 /
 * 0x03, then x) and writes the affine X || Y whose y has the parity the prefix asks for -- the format the other entry points take. */
int ec_aff_pt_y_from_x_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *x, uint8_t *y1, uint8_t *y2,
			     uint8_t *status);
int ec_point_decompress_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *compressed, uint8_t *out_aff,
			      uint8_t *status);
/* Structured signatures (ec_structured_sig_import_from_buf, sig/sig_algs.c:702: 3 bytes -- ec_alg_type, hash_alg_type, ec_curve_type --
 * in front of the raw signature): checks the three bytes against what the caller expects and the handle's curve, strips them
 * (raw_sigs: n x (structured_len - 3)); host-side framing, no device work.  Built-in curves only. */
int ec_structured_sig_import_batch(const ecamd_curve *curve, uint32_t n, const uint8_t *structured, uint32_t structured_len,
				   int alg_type, int hash_type, uint8_t *raw_sigs, uint8_t *status);
/* Structured private keys -> key pairs, batch form of ec_structured_key_pair_import_from_priv_key_buf (sig/ec_key.c:443) for the
 * algorithms whose public key is Y = xG (ECDSA, DECDSA: __ecdsa_init_pub_key, sig/ecdsa_common.c:172): each key is EC_PRIVKEY (1),
 * the ec_alg_type, the ec_curve_type, then the private scalar (key_len - 3 bytes, any length).  Header and x < q checked;
 * priv_out (may be NULL): n x qlen, the scalar as the signing entry points take it; pub_prj_out: n x 3*clen, Y = [x]G as
 * X || Y || 1 (the format of ec_pub_key_export_to_buf and of ec_ecdsa_verify_batch_fmt).  status ECAMD_ERR where libecc
 * returns -1, ECAMD_INF for x = 0 (libecc's key at infinity). */
int ec_structured_key_pair_import_batch(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *priv_keys,
					uint32_t key_len, int alg_type, uint8_t *priv_out, uint8_t *pub_prj_out, uint8_t *status);

/* Device-pointer forms of the verification / key-agreement entry points, for callers whose batches
 * already live in HBM (and for sharding a batch over GPUs, one context per device): same semantics and
 * layouts as the host-pointer forms above, every buffer a device pointer, kernels enqueued on
 * hip_stream (a hipStream_t; NULL = the context's stream).  They only enqueue (ec_ecdsa_verify_batch_dev included: the
 * items its interleaved secp256r1 loop could not finish are re-verified by kernels on the same stream) -- synchronise the
 * stream (or ecamd_ctx_synchronize for the context's stream) before reading.  The first call of a size may allocate
 * scratch (hipMalloc / hipFree, which synchronise the device); later calls of that size or smaller do not. */
int ec_ecdsa_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_pubkeys_aff,
			      const void *d_sigs, const void *d_digests, uint32_t digest_len, void *d_result,
			      void *hip_stream);
/* ec_ecdsa_recover_batch with device pointers: enqueue only, in pieces of at most ecamd_ctx_set_max_chunk items. */
int ec_ecdsa_recover_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_sigs, const void *d_digests,
			       uint32_t digest_len, void *d_pub1_aff, void *d_pub2_aff, void *d_status1, void *d_status2,
			       void *hip_stream);
int ec_eddsa_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_pubkeys,
			      const void *d_sigs, const void *d_hram, uint32_t hram_len, void *d_result,
			      void *hip_stream);
int ec_xdh_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_k, const void *d_u,
		     void *d_out, void *d_status, void *hip_stream);
/* ec_ecdsa_sign_batch / ec_ecccdh_derive_batch with device pointers: enqueue only. */
int ec_ecdsa_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_privs,
			    const void *d_nonces, const void *d_digests, uint32_t digest_len, void *d_sigs,
			    void *d_status, void *hip_stream);
int ec_ecccdh_derive_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_privs,
			       const void *d_peers_aff, void *d_secrets, void *d_status, void *hip_stream);
/* ec_sig_verify_batch / ec_sig_sign_batch with device pointers: enqueue only. */
int ec_sig_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const void *d_pubkeys_aff,
			    const void *d_sigs, const void *d_digests, uint32_t digest_len, void *d_result, void *hip_stream);
int ec_sig_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const void *d_privs,
			  const void *d_nonces, const void *d_digests, uint32_t digest_len, void *d_sigs, void *d_status,
			  void *hip_stream);
/* ec_sig_hashed_verify_batch / ec_sig_hashed_sign_batch with device pointers: enqueue only.  Scratch: besides what a verification
 * or signing call of the curve takes, ECSDSA / ECOSDSA stage a device-to-device copy of the slots of one chunk -- min(n, max_chunk)
 * x stride bytes (4 GiB at a chunk of 2^20 items and the largest stride of 4096; 92 MiB at the 92-byte stride of a 24-byte
 * message on a 256-bit curve) -- although only 4 + length bytes of a slot are hashed: choose the stride to fit the longest
 * message, or lower ecamd_ctx_set_max_chunk.  ECKCDSA stages 4 + clen bytes per item. */
int ec_sig_hashed_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n,
				   const void *d_pubkeys_aff, const void *d_sigs, const void *d_inputs, uint32_t stride, void *d_result,
				   void *hip_stream);
int ec_sig_hashed_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_privs,
				 const void *d_nonces, const void *d_inputs, uint32_t stride, void *d_sigs, void *d_status,
				 void *hip_stream);
/* ec_bign_verify_batch / ec_bign_sign_batch with device pointers (oid stays a host pointer): enqueue only.  Scratch: besides what a
 * verification or signing call of the curve takes, per item of a chunk belt-hash's slot (at most 4 + 64 + 66 + 128 bytes), its
 * 32-byte digest and, for hash_type != 0, the digest of the message.  Message slots are read where they lie: no copy. */
int ec_bign_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_pubkeys_aff,
			     const void *d_sigs, const void *d_inputs, uint32_t stride, const uint8_t *oid, uint32_t oid_len, void *d_result,
			     void *hip_stream);
int ec_bign_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_privs,
			   const void *d_nonces, const void *d_inputs, uint32_t stride, const uint8_t *oid, uint32_t oid_len, void *d_sigs,
			   void *d_status, void *hip_stream);
/* ec_rfc6979_nonce_batch / ec_decdsa_sign_batch with device pointers: enqueue only (sig/ecdsa_common.c:48-169 on the device, then the
 * core of ec_ecdsa_sign_batch_dev).  Scratch of the signing call: per item of a chunk the nonce (qlen bytes, secret), the digest when
 * in_is_digest = 0, and what ec_ecdsa_sign_batch_dev takes.  Message slots and digests are read where they lie: with in_is_digest = 0
 * d_in must be 4-byte aligned (the length word of a slot is read as one aligned word; in_stride is a multiple of 4), digests and keys
 * are read by octets and need no alignment.  d_nonces of the nonce call is the caller's buffer: secret, and the caller's to wipe. */
int ec_rfc6979_nonce_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs,
			       const void *d_digests, void *d_nonces, void *d_status, void *hip_stream);
int ec_decdsa_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs, const void *d_in,
			     uint32_t in_stride, int in_is_digest, void *d_sigs, void *d_status, void *hip_stream);
/* ec_dbign_nonce_batch / ec_dbign_sign_batch / ec_bip0340_nonce_batch / ec_bip0340_sign_batch with device pointers: enqueue only (oid and
 * t stay host pointers: they are copied into the kernel arguments before the call returns).  Scratch of the signing calls: per item of
 * a chunk the nonce (qlen bytes, secret) and what ec_bign_sign_batch_dev / ec_schnorr_sign_batch_dev take; the BIP0340 calls also Y and
 * its status.  Message slots must be 4-byte aligned (the length word is read as one aligned word); keys, aux values and digests are
 * read by octets.  d_pubkeys_aff may be NULL.  d_nonces of the nonce calls is the caller's buffer: secret, and the caller's to wipe. */
int ec_dbign_nonce_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_privs, const void *d_digests,
			     uint32_t digest_len, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, void *d_nonces,
			     void *d_status, void *hip_stream);
int ec_dbign_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs, const void *d_inputs,
			    uint32_t stride, const uint8_t *oid, uint32_t oid_len, const uint8_t *t, uint32_t t_len, void *d_sigs,
			    void *d_status, void *hip_stream);
int ec_bip0340_nonce_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs,
			       const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots, uint32_t stride, void *d_nonces,
			       void *d_status, void *hip_stream);
int ec_bip0340_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int hash_type, uint32_t n, const void *d_privs,
			      const void *d_pubkeys_aff, const void *d_aux, const void *d_hash_slots, uint32_t stride, void *d_sigs,
			      void *d_status, void *hip_stream);
/* ec_eddsa_sign_msg_batch / ec_eddsa_pub_key_batch with device pointers: enqueue only (sig/eddsa.c:611-688 and :1554-1870 on the
 * device).  adata stays host memory: it is copied into the kernel arguments before the call returns.  d_pubkeys and d_pub_out may be
 * NULL.  d_msg_slots must be 4-byte aligned (the length word is read as one aligned word); keys and encodings need no alignment.
 * Scratch per item of a chunk: a, r_hash, hram, R, S, PH(M) for the PH variants, and what ec_eddsa_sign_R_batch takes (twice when
 * the keys are derived here). */
int ec_eddsa_sign_msg_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, uint32_t n, const void *d_secret_keys,
				const void *d_pubkeys, const uint8_t *adata, uint32_t adata_len, const void *d_msg_slots,
				uint32_t msg_stride, void *d_sigs, void *d_pub_out, void *d_status, void *hip_stream);
int ec_eddsa_pub_key_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const void *d_secret_keys, void *d_pub_out,
			       void *d_status, void *hip_stream);
/* ec_schnorr_verify_batch / ec_schnorr_sign_batch with device pointers: enqueue only.  Scratch: besides what a verification or signing
 * call of the curve takes, a device-to-device copy of the slots of one chunk (min(n, max_chunk) x stride bytes: choose the stride to fit
 * the longest message, or lower ecamd_ctx_set_max_chunk).  d_pubkeys_aff may be NULL, as pubkeys_aff. */
int ec_schnorr_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_keys, int key_fmt,
				const void *d_sigs, const void *d_hash_slots, uint32_t stride, void *d_result, void *hip_stream);
int ec_schnorr_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *curve, int alg, int hash_type, uint32_t n, const void *d_privs,
			      const void *d_pubkeys_aff, const void *d_nonces, const void *d_hash_slots, uint32_t stride, void *d_sigs,
			      void *d_status, void *hip_stream);

/*
 * ---- several GPUs from C ----
 * One context and one host thread per device; a batch of n items is cut into contiguous shards (rank r of N owns
 * items [r*n/N, (r+1)*n/N): the work per item is constant, so equal counts are balanced); nothing is exchanged to
 * compute.  The host-pointer entry points below are the single-device ones run on every shard at once, each
 * device copying its results straight into the caller's arrays, so outputs and status bytes are exactly those of
 * the single-device call.  devices == NULL (or ndev <= 0): every visible device.  A device may be listed more than
 * once (one context and one shard per entry; they then share that GPU).
 */
typedef struct ecamd_multi ecamd_multi;
typedef struct ecamd_mcurve ecamd_mcurve; /* one ecamd_curve per rank */
int ecamd_multi_create(ecamd_multi **m, const int *devices, int ndev);
void ecamd_multi_destroy(ecamd_multi *m);
int ecamd_multi_size(const ecamd_multi *m);                 /* number of ranks */
int ecamd_multi_device(const ecamd_multi *m, int rank);     /* HIP device of a rank */
ecamd_ctx *ecamd_multi_ctx(ecamd_multi *m, int rank);       /* its context (device-pointer entry points, streams) */
void ecamd_multi_shard_range(uint32_t n, int rank, int nranks, uint32_t *lo, uint32_t *hi);
int ecamd_multi_curve_by_name(ecamd_multi *m, const char *name, ecamd_mcurve **curve);
int ecamd_multi_curve_from_params(ecamd_multi *m, const uint8_t *p, uint32_t p_len, const uint8_t *a, uint32_t a_len,
				  const uint8_t *b, uint32_t b_len, const uint8_t *curve_order, uint32_t curve_order_len,
				  const uint8_t *gx, uint32_t gx_len, const uint8_t *gy, uint32_t gy_len,
				  const uint8_t *gen_order, uint32_t gen_order_len, ecamd_mcurve **curve);
void ecamd_multi_curve_free(ecamd_mcurve *curve);
const ecamd_curve *ecamd_multi_curve_handle(const ecamd_mcurve *curve, int rank);
int ecamd_multi_curve_coord_len(const ecamd_mcurve *curve);
int ecamd_multi_curve_order_len(const ecamd_mcurve *curve);
/* sharded forms: same arguments and results as the single-device entry points of the same name */
int ecamd_multi_prj_pt_mul_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *scalars,
				 uint32_t scalar_len, const uint8_t *points_aff, uint8_t *out_aff, uint8_t *status);
int ecamd_multi_prj_pt_mul_batch_fmt(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *scalars,
				     uint32_t scalar_len, const uint8_t *points, int in_fmt, uint8_t *out, int out_fmt,
				     uint8_t *status);
int ecamd_multi_prj_pt_add_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *p1_aff, const uint8_t *p2_aff,
				uint8_t *out_aff, uint8_t *status);
int ecamd_multi_prj_pt_op_batch_fmt(ecamd_multi *m, const ecamd_mcurve *curve, int op, uint32_t n, const uint8_t *p1, const uint8_t *p2,
				    int in_fmt, uint8_t *out, int out_fmt, uint8_t *status);
int ecamd_multi_prj_pt_unprotected_mult_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *scalars,
					      uint32_t scalar_len, uint32_t scalar_stride, const uint8_t *points, int in_fmt, uint8_t *out,
					      int out_fmt, uint8_t *status);
int ecamd_multi_prj_pt_unique_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *points, int in_fmt,
				    uint8_t *out, int out_fmt, uint8_t *status);
int ecamd_multi_ecdsa_verify_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *pubkeys_aff,
				   const uint8_t *sigs, const uint8_t *digests, uint32_t digest_len, uint8_t *result);
int ecamd_multi_ecdsa_verify_batch_fmt(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *pubkeys, int pub_fmt,
				       const uint8_t *sigs, const uint8_t *digests, uint32_t digest_len, uint8_t *result);
int ecamd_multi_ecdsa_verify_msg_batch_fmt(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *pubkeys, int pub_fmt,
					   const uint8_t *sigs, int hash_type, const uint8_t *msg_slots, uint32_t msg_stride, uint8_t *result);
int ecamd_multi_eddsa_verify_msg_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
				       const uint8_t *hash_slots, uint32_t stride, uint8_t *result);
int ecamd_multi_eddsa_verify_msg_prj_batch(ecamd_multi *m, const ecamd_mcurve *c, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
					   const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, uint8_t *result);
int ecamd_multi_eddsa_verify_msg_prj_all_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
					       const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, int *all_valid);
int ecamd_multi_eddsa_verify_ph_prj_batch(ecamd_multi *m, const ecamd_mcurve *c, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
					  const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, const uint8_t *msg_slots, uint32_t msg_stride,
					  uint8_t *result);
int ecamd_multi_ecdsa_sign_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *privs,
				 const uint8_t *nonces, const uint8_t *digests, uint32_t digest_len, uint8_t *sigs,
				 uint8_t *status);
int ecamd_multi_ecdsa_sign_msg_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *privs, const uint8_t *nonce_raw,
				     int hash_type, const uint8_t *msg_slots, uint32_t msg_stride, uint8_t *sigs, uint8_t *status);
int ecamd_multi_key_pair_gen_raw_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *raw, uint8_t *priv_out,
				       uint8_t *pub_out_aff, uint8_t *status);
int ecamd_multi_ecccdh_derive_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *privs,
				    const uint8_t *peers_aff, uint8_t *secrets, uint8_t *status);
int ecamd_multi_xdh_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *k, const uint8_t *u,
			  uint8_t *out, uint8_t *status);
int ecamd_multi_eddsa_verify_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *pubkeys,
				   const uint8_t *sigs, const uint8_t *hram, uint32_t hram_len, uint8_t *result);
int ecamd_multi_eddsa_encode_point_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *points_prj,
					 uint8_t *enc, uint8_t *status);
/* ec_verify_batch's whole-batch bit, sharded (see ec_eddsa_verify_all_batch: Ed25519 shards of at least 2^17 items run the
 * multi-scalar multiplication on their device); first_rejected (may be NULL): lowest rejected index of the whole batch, n if none */
int ecamd_multi_eddsa_verify_all_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *pubkeys,
				       const uint8_t *sigs, const uint8_t *hram, uint32_t hram_len, int *all_valid,
				       uint32_t *first_rejected);
/* ec_schnorr_verify_all_batch, sharded: every device decides its shard with a combination of its own; valid iff every shard is */
int ecamd_multi_schnorr_verify_all_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *s, const uint8_t *ne,
					 const uint8_t *keys_aff, const uint8_t *r, int r_fmt, int *all_valid);
int ecamd_multi_schnorr_verify_msg_all_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *keys, int key_fmt,
					     const uint8_t *sigs, int r_fmt, int hash_type, const uint8_t *hash_slots, uint32_t stride,
					     uint32_t x_offset, int *all_valid);
int ecamd_multi_eddsa_sign_R_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *r_hash, uint8_t *R_enc,
				   uint8_t *status);
int ecamd_multi_eddsa_sign_S_batch(ecamd_multi *m, const ecamd_mcurve *curve, uint32_t n, const uint8_t *r_hash, const uint8_t *hram,
				   const uint8_t *a_scalars, uint8_t *S_out);
/* ecamd_ctx_set_secret_scalars / ecamd_ctx_wipe_scratch on every rank's context */
int ecamd_multi_set_secret_scalars(ecamd_multi *m, int on);
/* ecamd_ctx_set_host_ready_hook for every rank: fn sees item numbers of the WHOLE call's arrays (a rank's shard offset is added) and may be
 * entered from several ranks' threads at once */
int ecamd_multi_set_host_ready_hook(ecamd_multi *m, ecamd_host_ready_fn fn, void *arg);
int ecamd_multi_set_msm_seed(ecamd_multi *m, const uint8_t seed[32]);   /* rank r: seed with r xored into its first bytes */
int ecamd_multi_wipe_scratch(ecamd_multi *m);
/* The one collective, for callers that keep device-resident outputs on every GPU: an RCCL all-gather (over xGMI) of
 * equal-size shards.  d_send[r]: bytes_per_rank bytes on rank r's device; d_recv[r]: nranks * bytes_per_rank bytes
 * there.  librccl is loaded on first use; needs distinct devices.  The gathers run on private streams that first wait for
 * everything enqueued so far on each rank's context stream (ecamd_multi_ctx(m, r)'s, where the *_dev entry points put their
 * kernels by default), so device-resident producers need no host synchronisation in between; ecamd_multi_allgather_streams
 * takes the producers' streams (one hipStream_t per rank, NULL entries = the context's) for shards written elsewhere.
 * Returns when the gathered data is in place on every rank. */
int ecamd_multi_allgather(ecamd_multi *m, const void *const *d_send, void *const *d_recv, size_t bytes_per_rank);
int ecamd_multi_allgather_streams(ecamd_multi *m, const void *const *d_send, void *const *d_recv, size_t bytes_per_rank,
				  void *const *producer_streams);

/* Test hook of the Ed25519 multi-scalar multiplication: the combination with a caller-chosen 32-byte seed.  z_out (n x 16
 * little-endian z_i) and sum_out (36 words: X, Y, Z, T of the sum before the cofactor, nine radix-2^29 digits each of lazily
 * reduced residues mod 2^255 - 19) may be NULL.  n <= the context's max_chunk. */
int ecamd_debug_eddsa_msm(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
			  const uint8_t *hram, const uint8_t seed[32], int *accept, uint8_t *z_out, uint32_t *sum_out);

/* The same for the Schnorr-type multi-scalar multiplication (ec_schnorr_verify_all_batch).  sum_out: the lanes' sum before the generator's
 * term, ecamd_debug_schnorr_msm_words() words (X, Y, Z digits of the unit's representation, then an "is infinity" word). */
int ecamd_debug_schnorr_msm(ecamd_ctx *ctx, const ecamd_curve *curve, uint32_t n, const uint8_t *s, const uint8_t *ne, const uint8_t *keys_aff,
			    const uint8_t *r, int r_fmt, const uint8_t seed[32], int *accept, uint8_t *z_out, uint32_t *sum_out);
uint32_t ecamd_debug_schnorr_msm_words(const ecamd_curve *curve);

#ifdef __cplusplus
}
#endif
#endif /* LIBECC_AMD_H */
