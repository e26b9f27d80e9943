// libecc_amd/csrc/ecamd_host_internal.h -- what the host-side translation units of the C ABI (include/libecc_amd.h) share.
//
// The units:
//   ecamd_host.cpp         errors, host big integers, the context, curve handles, scratch sizing, host_pipeline and the heads of the entry
//                          points, scalar multiplication and point operations, ECDSA and its relatives, XDH
//   ecamd_host_eddsa.cpp   EdDSA on the WEI25519 and WEI448 handles: verification, the Ed25519 whole-batch evaluation (buckets and Straus) and
//                          Ed448's, which runs the Schnorr-type one, signing, one-call signing, the ragged-message forms (ec_eddsa_*_msgs_*)
//   ecamd_host_msm.cpp     the Schnorr-type whole-batch evaluation (ec_schnorr_verify_*all_*) and the seed of a whole-batch call's z_i
//   ecamd_host_sigfam.cpp  ECKCDSA / ECSDSA / ECOSDSA, BIGN / DBIGN, BIP0340 / ECFSDSA, message-level ECGDSA / ECRDSA / SM2, ec_hash_slots_*,
//                          ec_digest_slots_*, HMAC and deterministic ECDSA over the whole hash table (ec_hmac_slots_*, ec_*_ht_*),
//                          the ragged message array (ec_digest_msgs_*, ec_ecdsa_verify_msgs_*, ec_decdsa_sign_msgs_*)
//                          and the _ht names of the three commitment-hashing families (ec_sig_hashed_*_ht_*, ec_schnorr_*_ht_*, ec_bip0340_*_ht_*)
// A protocol family lives in exactly one unit.  This header declares only what more than one unit uses; what one unit needs stays
// `static` in its file.  The shared functions are in namespace ecamd_host with hidden visibility: none of them enters the library's
// dynamic symbol table.
#ifndef ECAMD_HOST_INTERNAL_H
#define ECAMD_HOST_INTERNAL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <strings.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <functional>
#include <mutex>
#include <sys/random.h>

#include "../../include/libecc_amd.h"
#include "ecamd_internal.h"

#pragma GCC visibility push(hidden)

// small host big integers (little-endian 32-bit words); only used to derive constants
typedef std::vector<uint32_t> Big;
struct SchnorrStreamStep;   // ecamd_host_msm.cpp: which part of the evaluation a call of schnorr_msm_dev_locked runs

namespace ecamd_host {
int fail(const std::string &m);   // files the thread's error string (ecamd_last_error) and returns -1
}
#define HIPCHK(expr) \
	do { \
		hipError_t e_ = (expr); \
		if (e_ != hipSuccess) { \
			return ecamd_host::fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
		} \
	} while (0)

#define SIG_ECDSA 1   /* libecc's ec_alg_type number of ECDSA: the `alg` of the verification paths when they serve ECDSA */

// ------------------------------------------------------------------------------------------
// objects behind the opaque handles
// ------------------------------------------------------------------------------------------
// The scratch slots of ecamd_ctx::stage[].  Every device core works in a FRAME: a set of named slots, sized by stage_need()
// when the core starts and dead when it returns.  Frames of different cores share indices on purpose (one context runs one
// call at a time, ctx->mu), so a buffer grown by one family serves the next.  This block is the one place that says which
// frames exist, who uses them, and which may be live at the same time; two names with one value in frames that can be
// live together are a bug.
//
//   frame (prefix)            slots         used by                                                live beside it
//   HW_  hand-staged host     0..3          pt_batch, ec_prj_pt_op_batch_fmt, ec_prj_pt_unprotected_mult_batch, ec_fp_op_batch   nothing
//   PF_  point formats        0..7          pt_fmt_batch                                           (smul_dev_locked: no slots)
//   YX_  square roots         0..3          y_from_x_common                                        nothing
//   MH_  EdDSA whole batch    0..3, 14      eddsa_msm_host_locked, eddsa448_msm_host_locked        EV_ 3..9, 12, 13 (Ed448 only: hence 14, not 3)
//   MS_  Schnorr whole batch  0..4          schnorr_msm_host_locked                                nothing (the evaluation works in ctx->msm)
//   XD_  X25519 / X448        2..5, 7, 8    xdh_dev_locked                                         nothing
//   CD_  ECCCDH               3..8          ecccdh_dev_locked                                      nothing
//   ST_  verification         3..15         two_mul_dev / two_mul_sum_dev and their callers: ecdsa_two_smul_dev, ecdsa_fused_g_dev,
//                                           hsig_ / bign_ / schnorr_item_verify_dev_locked         ST_SLOTS.., ST_TARGET, SI_, EF_, BW_
//   VP_  secp256r1 loop       3..5, 7       ecdsa_verify_dev_locked (ST_U, ST_V and VP_*); its redo pass is the ST_ frame, after it   ST_TARGET, EF_
//   RC_  recovery             10..14        ecdsa_recover_dev_locked, on top of ST_U .. ST_FLAGS (it has no [q]Y pass and no W' of its own)
//   SG_  signing              3..5, 7, 20   ecdsa_ / sig_ / hsig_ / bign_ / schnorr_item_sign_dev_locked, ec_ecdsa_sign_msg_batch,
//                                           decdsa_sign_ / decdsa_ht_ / dbign_sign_ / bip0340_dev_locked (SG_NONCES)   ST_FLAGS, ST_SLOTS, ST_DIGESTS, ST_BELT
//   EV_  EdDSA verification   3..15, 18, 19 eddsa_verify_dev_locked, eddsa448_verify_dev_locked, eddsa448_msm_dev_locked   ST_DIGESTS (h), EP_, EB_, MH_
//   SR_  EdDSA [r]B           3..5          eddsa_sign_R_dev_locked                                ES_ (it runs inside the one-call signing)
//   EN_  EdDSA point encoding 3, 4          ec_eddsa_encode_point_batch                            nothing
//   BL_  blinded scalars      12, 13        ec_prj_pt_mul_blind_batch                              (smul_dev_locked: no slots)
//   EF_  projective ECDSA keys 12, 14..16   ecdsa_verify_host_fmt: the imported keys; the regrouped items of keys at infinity   ST_ 3..11, VP_, ST_DIGESTS, ST_TARGET
//        slots and digests    16..18        ST_SLOTS, ST_DIGESTS, ST_BELT: the staged message slots and what is hashed from them, for every family
//   SI_  Schnorr item extras  18, 20..23    schnorr_item_verify_dev_locked; 20 / 21 also ec_schnorr_verify_msg_all_batch's key import   ST_, BW_
//   EP_  EdDSA projective     20..23        eddsa_verify_msg_prj_impl, per chunk                   EV_, EB_, ST_DIGESTS
//   BW_  Schnorr batch-wide   24..28        ec_schnorr_verify_msg_all_batch: filed chunk by chunk, read when the last chunk is in,
//                                           so they outlive every per-chunk frame of the call     SI_PRJ_*, ST_DIGESTS, ST_ (item-by-item fallback)
//   EB_  EdDSA batch-wide     24..27        eddsa_verify_msg_prj_impl, the same way                EP_, EV_, ST_DIGESTS
//        sig_target           29            ST_TARGET: the comparison target of ECGDSA / ECRDSA / SM2, beside ST_ and VP_
//   ES_  one-call EdDSA sign  30..40        eddsa_sign_msg_dev_locked, eddsa_pub_key_dev_locked    SR_
//   SM_  sig from messages    41, 42        sig_msg_verify_ / sig_msg_sign_dev_locked, which outlive the digest-level core they call   ST_, VP_, SG_, ST_SLOTS, ST_DIGESTS, ST_TARGET
//   DM_  ragged messages      43..45        msgs_host_call (the staged piece of the message array and its rebased offsets), ecdsa_verify_msgs_ /
//                                           decdsa_sign_msgs_ / eddsa_verify_msgs_dev_locked (DM_BAD), which outlive the core they call   ST_, VP_, SG_, EV_, ST_DIGESTS
//
// smul_dev_locked itself takes no slot (ctx->tbl, ctx->tbl_fast); host_pipeline stages in ctx->hbuf.
// ------------------------------------------------------------------------------------------
enum StageSlot {
	HW_IN0 = 0, HW_IN1 = 1, HW_OUT = 2, HW_STATUS = 3,
	PF_SCALARS = 0, PF_IN = 1, PF_AFF = 2, PF_PRE = 3, PF_RES = 4, PF_RST = 5, PF_OUT = 6, PF_OST = 7,
	YX_IN = 0, YX_Y1 = 1, YX_Y2 = 2, YX_ST = 3,
	MH_PUB = 0, MH_SIG = 1, MH_HRAM = 2, MH_VERDICTS = 3, MH_VERDICT448 = 14,
	MS_S = 0, MS_NE = 1, MS_KEYS = 2, MS_VERDICTS = 3, MS_R = 4,
	XD_SCALARS = 2, XD_POINTS = 3, XD_FLAGS = 4, XD_REC = 5, XD_OUT = 7, XD_STK = 8,
	CD_OUT = 3, CD_ST = 4, CD_HQ = 5, CD_STH = 6, CD_QP = 7, CD_STSUB = 8,
	// W' = [u]G + [v]Y: the multipliers, A = [u]G, B = [v]Y and their status bytes, the flag byte of the prep kernel, the status and the
	// point of the [q]Y pass, W' and its status, and the sinks of k_recover_fin's second sum A - B
	ST_U = 3, ST_V = 4, ST_A = 5, ST_B = 6, ST_STA = 7, ST_STB = 8, ST_FLAGS = 9, ST_SUB = 10, ST_QY = 11,
	ST_W = 12, ST_WSINK = 13, ST_STW = 14, ST_STWSINK = 15,
	VP_FLAGS = 5, VP_KEYS = 7,   // VP_KEYS: the zeroed points of rejected keys, then the key status
	RC_YST = 10, RC_X = 11, RC_Y1 = 12, RC_Y2 = 13, RC_R = 14,
	SG_KG = 3, SG_STKG = 4, SG_Y = 5, SG_STY = 7, SG_NONCES = 20,   // SG_Y, SG_STY: BIP0340's public key
	// 3: the key as a Weierstrass point, or v and |u| of the half-length scalars; 13: the status of [h]A, or the lattice kernel's meta bytes
	EV_A = 3, EV_R = 4, EV_FLAGSA = 5, EV_FLAGSR = 6, EV_FLAGSS = 7, EV_S = 8, EV_H = 9, EV_EDA = 10, EV_REC = 11,
	EV_HA = 12, EV_STHA = 13, EV_SG = 14, EV_STSG = 15, EV_TBL = 18, EV_EDR = 19,
	EV_NE = 12, EV_GATE = 13,    // eddsa448_msm_dev_locked: q - h, and the gate word with the piece's verdict behind it
	SR_R = 3, SR_RW = 4, SR_STR = 5,
	EN_AFF = 3, EN_PRE = 4,
	BL_SCALARS = 12, BL_BAD = 13,
	EF_AFF = 12, EF_INF_SIGS = 14, EF_INF_DATA = 15, EF_INF_RES = 16,
	ST_SLOTS = 16, ST_DIGESTS = 17, ST_BELT = 18,
	SI_KEY = 18, SI_PRJ_AFF = 20, SI_PRJ_ST = 21, SI_WPT = 22, SI_WST = 23,   // the key as the equation uses it; the projective import; ECFSDSA's W
	EP_AFF = 20, EP_PRE = 21, EP_KEY = 22, EP_KST = 23,
	BW_S = 24, BW_NE = 25, BW_KEYS = 26, BW_R = 27, BW_VERDICTS = 28,
	EB_KEYS = 24, EB_SIGS = 25, EB_HRAM = 26, EB_MARKS = 27,
	ST_TARGET = 29,
	ES_A = 30, ES_RHASH = 31, ES_AWIDE = 32, ES_HRAM = 33, ES_R = 34, ES_S = 35, ES_BAD = 36, ES_STR = 37, ES_STA = 38, ES_AENC = 39, ES_PH = 40,
	SM_BAD = 41, SM_Z = 42,   // the items a message-level ECGDSA / ECRDSA / SM2 call rejects itself; SM2's Z
	DM_MSGS = 43, DM_OFFS = 44, DM_BAD = 45,   // the items whose offsets are unusable
	ECAMD_NSTAGE
};
static_assert(ECAMD_NSTAGE == DM_BAD + 1, "ECAMD_NSTAGE counts the slots: the last frame ends the array");

struct ecamd_ctx {
	int device;
	hipStream_t stream;
	uint32_t max_chunk;
	// grow-only scratch
	uint32_t *tbl;      // complete-formula kernel: 16 x 3 x NW words per item, word-major
	size_t tbl_bytes;
	uint32_t *tbl_fast; // fast paths: per-item window tables (secp256r1: 512 B affine table + 1120 B staging per item)
	size_t tbl_fast_bytes;
	uint8_t *prep_scratch;     // k_ecdsa_prep_g: prefix products, n x NL words
	size_t prep_scratch_bytes;
	uint8_t *stage[ECAMD_NSTAGE];
	size_t stage_bytes[ECAMD_NSTAGE];
	// the scratch above is shared by every call: a call enqueued on another stream than the previous one first waits
	// for `busy`, recorded behind the previous call's last kernel (StreamScope)
	hipEvent_t busy;
	hipStream_t last_stream;
	bool inflight;
	// host-pointer entry points: chunks of host_chunk items, the copy of chunk c+1 overlaps the kernels of chunk c
	hipStream_t copy_stream;
	hipEvent_t in_ready[2];
	// ECDSA verification on secp256r1: k_ecdsa_prep (s^-1, u1, u2 mod q: two waves per SIMD, compute only) runs on this stream
	// beside the bandwidth-bound k_p256_table / k_p256_affine of the same chunk; the interleaved window loop -- the first reader
	// of u1, u2 and the flags -- waits for side_done ($ECAMD_NO_SIDE_STREAM: off).  66.0 -> 67.0 M verifications/s.
	hipStream_t side_stream;
	hipEvent_t side_fork, side_done, side_mid, side_aux;   // (side_mid / side_aux: the bucket evaluation's second and third joins)
	hipEvent_t side_hi, side_red;   // the bucket evaluation: the key-only windows are summed (on the caller's stream) / reduced (on the side stream)
	hipStream_t side2_stream;       // the bucket evaluation: the windows below 2^128 are filed here while the key-only windows are summed
	hipEvent_t side2_fork, side2_done;
	bool side2_ok;
	bool side_ok;
	uint32_t host_chunk;
	uint32_t host_first_min;   // smallest first chunk of a multi-chunk call (ECAMD_HOST_RAMP_MIN, default 2^16; host_pipeline)
	// producer hook of the host-pointer entry points (ecamd_ctx_set_host_ready_hook): called before a range of the caller's input arrays is read
	ecamd_host_ready_fn ready_fn = nullptr;
	void *ready_arg = nullptr;
	uint8_t *hbuf[2][6];       // double-buffered device staging of the caller's arrays (inputs and outputs)
	size_t hbuf_bytes[2][6];
	uint32_t comb_min_batch;   // fixed-base batches of at least this many items build / use the generator's comb table (0: never)
	bool secret_scalars;       // ecamd_ctx_set_secret_scalars: constant-address look-ups, no data-dependent kernel choice
	int eddsa_msm;             // ecamd_ctx_set_eddsa_msm: 0 never, 1 batches of at least msm_min items, 2 always
	uint32_t msm_min, msm_k;   // msm_k: items per lane of the Straus evaluation (0: chosen from the batch size)
	uint8_t *msm;              // scratch of the multi-scalar multiplication
	size_t msm_bytes;
	uint8_t msm_seed_bytes[32]; // ecamd_ctx_set_msm_seed: key of the next whole-batch combination's z_i (used once)
	bool msm_seed_valid;
	bool timing;               // record HIP events around the kernels of the scalar-mult pipeline
	hipEvent_t ev[ECAMD_NTIMED + 1];
	bool ev_valid;
	hipEvent_t ev_dom[2];      // around the dominant kernel of the last protocol call (verify loop, ladder, Edwards window loop)
	bool ev_dom_valid;
	std::mutex mu;
};

struct ecamd_curve {
	ecamd_ctx *ctx;
	int nw;     // 32-bit words per element
	int slot;   // __constant__ slot: field of definition
	int qslot;  // __constant__ slot: generator order q as a modulus (-1: protocol ops unavailable)
	int curve_type;  // libecc's ec_curve_type of a built-in curve (structured keys carry it), 0 for user curves
	int qnw;    // words of the mod-q kernels: nw, or more when q is longer than p (secp224k1: |q| = 225 > 224)
	int clen;   // BYTECEIL(pbits)
	int qlen;   // BYTECEIL(qbits)
	int pbits, qbits;
	uint32_t jmax;  // floor((p - 1) / q) capped at 64: how many multiples of q a verification's r + j q < p can take (curve_finish)
	Big p, a, b, order, gx, gy, q;
	uint8_t *d_gen;  // generator, affine X||Y big-endian, in HBM; followed by q (qlen bytes) and the cofactor byte
	uint32_t cofactor; // order / q when that is 1..255, else 0
	// per-curve constants of the Ed25519 / X25519 / X448 entry points, computed on first use (ctx->mu held)
	int ed_state;    // 0 not yet, 1 ready, -1 this handle is not the Ed25519 model (ed_err says why)
	const char *ed_err;
	EcamdEdDecodeArgs ed_tmpl;
	uint32_t ed_cof_dbl;
	int ed448_state;     // Ed448 on the WEI448 handle: 0 not yet, 1 ready, -1 not that curve
	const char *ed448_err;
	EcamdEd448DecodeArgs ed448_tmpl;
	uint8_t ed448_c4[56]; // 4^-1 mod q, big-endian (eddsa_import_pub_key multiplies the key by it)
	uint32_t ed_2d[9];   // 2 d mod p, plain radix-2^29 digits (Edwards arithmetic of the 2^255 - 19 unit)
	uint32_t ed_Bx[9], ed_By[9];  // the Ed25519 base point, the same digits
	int xdh_state;
	const char *xdh_err;
	EcamdXdhPrepArgs xdh_tmpl;
	uint32_t xdh_A3[17];
	uint8_t xdh_cof;
	int sqrt_state;  // Tonelli-Shanks constants of fp_sqrt for this field: 0 not yet, 1 ready (ctx->mu held)
	EcamdYfromXArgs sqrt_tmpl;
	bool is_p256;    // exactly secp256r1: hand-specialised radix-2^29 Jacobian kernel
	int gslot;       // constant slot of the generic radix-2^29 Jacobian kernel (-1: none)
	int gpslot;      // secp256r1 handles only (their scalar multiplication has its own kernels): slot of the dense 256-bit radix-2^29 unit holding
			 // the curve, for k_prj_import_g (-1: none, k_prj_import<8> serves)
	int gqslot;      // constant slot of the dense radix-2^29 unit of the ORDER's size holding q as its modulus (k_ecdsa_prep_g; -1: none)
	int gflavour;    // 0 dense reduction, 1 secp521r1 (p = 2^521 - 1), 2 p = 2^255 - 19, 3 secp384r1's prime, 4 secp256k1's prime, 5 p = 2^448 - 2^224 - 1,
	                 // 6 secp224r1's prime, 7 secp192r1's prime (3, 6, 7: signed sparse Montgomery reduction)
	uint32_t *d_comb4;  // the 4-bit comb of the generator for SECRET scalars: secp256r1 65 x 8 entries of 40 words (k_p256_comb4m, built with the
			    // handle), radix-2^29 units (8 NW + 1) x 8 comb entries (k_comb_g<.., SCAN4>, built on first use); NULL: none
	bool comb4_off;     // ... its construction was tried
	uint32_t *d_gtab; // secp256r1: affine window table [1..8]G, radix-2^29 Montgomery digits, 8 x 40 words
	uint32_t *d_comb; // fast paths: 16-bit comb table of G, built on the first large fixed-base batch (NULL before / disabled)
	bool comb_off;    // construction failed or is in progress: do not try (again)
	uint32_t *d_edcomb; // WEI25519 on the 2^255 - 19 unit: 16-bit comb table of the Ed25519 base point ON THE EDWARDS CURVE
	                    // (k_ed_tail_c25519), built on the first verification batch of comb_min_batch items; NULL before / disabled
	bool edcomb_off;
	uint32_t qdig[9]; // secp256r1: digits of the group order
};

namespace ecamd_host {

// the host big integers
int big_bitlen(const Big &a);
void big_to_be(uint8_t *dst, int len, const Big &a);
void big_trim(Big &a);
Big big_from_be(const uint8_t *b, size_t len);
int big_cmp(const Big &a, const Big &b);
Big big_add(const Big &a, const Big &b);
Big big_sub(const Big &a, const Big &b);  // a >= b
Big big_mul(const Big &a, const Big &b);
Big big_mod(const Big &a, const Big &m);
Big big_pow2(int e);
Big big_mulmod(const Big &a, const Big &b, const Big &m);
Big big_powmod(const Big &a, const Big &e, const Big &m);
void big_store(uint32_t *dst, int nw, const Big &a);
void big_digits29(uint32_t *dst, int nl, const Big &a, int w = 29);   // w-bit digits, nl of them
Big big_sqrt_m1(const Big &p);  // 2^((p-1)/4) mod p, a square root of -1 when p = 5 mod 8

// Every call works in the context's shared scratch (window tables, stage[] buffers).  A call enqueued on another
// stream than the previous one therefore first makes its stream wait for the previous call's last kernel, and
// leaves an event behind its own last kernel (ctx->mu held for the lifetime of the scope).
// (the stream of the innermost scope on this thread -- what ensure() orders the wipe of a growing scratch buffer behind -- is a
// thread-local of ecamd_host.cpp, where the constructor and the destructor are defined)
struct StreamScope {
	ecamd_ctx *c;
	hipStream_t s, outer;
	bool outer_active;
	StreamScope(ecamd_ctx *ctx, hipStream_t stream);
	~StreamScope();
};

// Scalars that are public by construction (u1, u2 of a verification, h and S of EdDSA, the group order and cofactor of a
// subgroup check) keep the digit-indexed look-ups and the comb table even when the context is in secret-scalar mode
// (ecamd_ctx_set_secret_scalars is about private keys, nonces and blinded scalars).  ctx->mu held.
struct PublicScalars {
	ecamd_ctx *c;
	bool saved;
	explicit PublicScalars(ecamd_ctx *ctx) : c(ctx), saved(ctx->secret_scalars) { c->secret_scalars = false; }
	~PublicScalars() { c->secret_scalars = saved; }
};

// grow-only device scratch: *buf holds at least `need` bytes afterwards; a buffer that has to grow is wiped before it is freed
int ensure(uint8_t **buf, size_t *have, size_t need);

// Size slots of a frame by name (the StageSlot block above ecamd_ctx): ensured in the order given; 0 bytes asks for nothing.
struct StageNeed {
	StageSlot slot;
	size_t bytes;
};
int stage_need(ecamd_ctx *ctx, std::initializer_list<StageNeed> needs);
int stage_need(ecamd_ctx *ctx, StageSlot slot, size_t bytes);

// The one way a device core bounds its scratch: pieces of at most ctx->max_chunk items, in order on the stream.  body(off, m) enqueues
// the items [off, off + m); the first non-zero result ends the walk and is returned.  A core that sizes its frame once does so before
// the walk, for chunk_items() items.  (Three whole-batch loops number their pieces for the z_i and so walk by hand:
// eddsa_verify_msg_prj_impl and ec_schnorr_verify_msg_all_batch, which also skip the walk after a streamed batch, and
// eddsa_verify_all_dev_locked.)
static inline uint32_t chunk_items(const ecamd_ctx *ctx, uint32_t n) { return n < ctx->max_chunk ? n : ctx->max_chunk; }
template <class Body>
static int for_chunks(const ecamd_ctx *ctx, uint32_t n, Body body)
{
	for (uint32_t off = 0; off < n; off += ctx->max_chunk) {
		const uint32_t m = (n - off) < ctx->max_chunk ? (n - off) : ctx->max_chunk;
		if (const int rc = body(off, m)) {
			return rc;
		}
	}
	return 0;
}

// the caller's arrays of a host-pointer entry point (host_pipeline, ecamd_host.cpp)
struct HostArr {
	const uint8_t *in;   // input array (or NULL)
	uint8_t *out;        // output array (or NULL)
	size_t stride;       // bytes per item
};

// what host_pipeline hands its core for one chunk: the item count, the device copies of the caller's arrays (index = position in `arrs`;
// NULL where the array is not an input / output), the stream, and `between` (see below)
using DevIn = std::vector<const uint8_t *>;
using DevOut = std::vector<uint8_t *>;
using Between = std::function<int()>;
using HostCore = std::function<int(uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &between)>;

// ------------------------------------------------------------------------------------------
// The head of an entry point, after its own argument checks and the n == 0 return.  Device pointers: the lock, the device, the
// caller's stream or the context's, the StreamScope, then body(s).  Host pointers: the lock, the device, host_pipeline.
// Entry points that take the lock earlier (a setup step under it), drop it in between or open no scope keep their own head.
// ------------------------------------------------------------------------------------------
template <class Body>
static int dev_call(ecamd_ctx *ctx, void *hip_stream, Body body)
{
	std::lock_guard<std::mutex> lk(ctx->mu);
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
	StreamScope scope(ctx, s);
	return body(s);
}
int host_call(ecamd_ctx *ctx, int pbits, uint32_t n, const std::vector<HostArr> &arrs, const HostCore &core);
// the pipeline itself, for the heads that already hold ctx->mu and have set the device (even_chunk: see its definition)
int host_pipeline(ecamd_ctx *ctx, int pbits, uint32_t n, const std::vector<HostArr> &arrs, const HostCore &core, uint32_t even_chunk = 0);

// ---- the cores of ecamd_host.cpp that the other families build on (ctx->mu held; only enqueue) ----
hipError_t launch_prj_import(const ecamd_curve *cv, const EcamdPrjInArgs &I, hipStream_t s);
// sstride = slen normally; 0 broadcasts one scalar to every item (subgroup / cofactor passes)
int smul_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_scalars, uint32_t slen,
		    const uint8_t *d_points, uint8_t *d_out, uint8_t *d_status, hipStream_t s,
		    uint32_t sstride = 0xffffffffu, bool redo_only = false, const uint8_t *d_scalars2 = nullptr);
// W' = [u]G + [v]Y for a verification (ST_ frame), and the digest-level cores the message-level forms call
int verify_sum_need(ecamd_ctx *ctx, const ecamd_curve *cv, size_t chunk);
int verify_sum_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t m, const uint8_t *d_Y, hipStream_t s);
int ecdsa_verify_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_pub,
			    const uint8_t *d_sig, const uint8_t *d_dig, uint32_t hlen, uint8_t *d_res, hipStream_t s,
			    const Between *between = nullptr, int alg = SIG_ECDSA);
// ECDSA signing with given nonces (SG_ frame: [k]G as the context's secret-scalar mode says, then r and s)
int ecdsa_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_privs, const uint8_t *d_nonces,
			  const uint8_t *d_digests, uint32_t hlen, uint8_t *d_sigs, uint8_t *d_status, hipStream_t s);
int sig_alg_ok(const char *fn, int alg);
// the generator's 16-bit comb table, built on the first fixed-base batch of comb_min_batch items; the digests of staged message slots into ST_DIGESTS
void maybe_build_comb(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n);
int ecdsa_hash_stage(ecamd_ctx *ctx, int hash_type, uint32_t m, const uint8_t *d_slots, uint32_t stride, uint32_t dlen, hipStream_t s);

// ---- the whole-batch evaluation of ecamd_host_msm.cpp that Ed448's whole-batch form runs too, and the seed of the z_i (ctx->mu held) ----
int msm_seed(ecamd_ctx *ctx, uint8_t seed[32]);
void msm_seed_discard(ecamd_ctx *ctx);   // (takes ctx->mu itself)
static inline size_t msm_align(size_t x) { return (x + 255) & ~(size_t)255; }
bool schnorr_msm_unit(const ecamd_curve *cv, int *pbits, int *flavour, int *slot);
int schnorr_msm_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_s, const uint8_t *d_ne, const uint8_t *d_keys,
			   const uint8_t *d_r, int r_fmt, const uint8_t seed[32], uint32_t piece, uint8_t *d_verdict, uint8_t *d_z_dump,
			   uint32_t *d_sum_dump, hipStream_t s, uint32_t cof_dbl = 0, const SchnorrStreamStep *step = nullptr);
int schnorr_msm_host_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *sv, const uint8_t *ne, const uint8_t *keys,
			    const uint8_t *r, int r_fmt, const uint8_t *fixed_seed, int *accept, uint8_t *z_out, uint32_t *sum_out);

// ---- the ragged message array (ecamd_host_sigfam.cpp), shared with EdDSA's ragged calls (ecamd_host_eddsa.cpp) ----
// a per-item array of a host form: `stride` octets from item to item, `len` octets used per item (the last item's stride is not read)
struct MsgsArr {
	const uint8_t *in;
	uint8_t *out;
	size_t stride, len;
};
using MsgsCore = std::function<int(uint32_t m, const uint8_t *d_msgs, uint64_t msgs_len, const uint64_t *d_offsets, const DevIn &ip, const DevOut &op, hipStream_t s)>;
// The host form of a ragged call: takes ctx->mu, stages pieces of at most max_chunk items or MSGS_CHUNK_BYTES octets with offsets rebased
// to the piece (DM_MSGS / DM_OFFS, the per-item arrays through ctx->hbuf[0]) and runs core on each; one piece at a time.
int msgs_host_call(const char *fn, ecamd_ctx *ctx, uint32_t n, const uint8_t *msgs, const uint64_t *offsets, const std::vector<MsgsArr> &arrs,
		   const MsgsCore &core);
// the alignment of a _dev form's d_msgs (4) and d_offsets (8), and d_msgs != NULL with a positive length
int msgs_dev_ptr_ok(const char *fn, const void *d_msgs, uint64_t msgs_len, const void *d_offsets);
int sig_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *d_privs, const uint8_t *d_nonces,
			const uint8_t *d_digests, uint32_t hlen, uint8_t *d_sigs, uint8_t *d_status, hipStream_t s);

}  // namespace ecamd_host

#pragma GCC visibility pop
#endif
