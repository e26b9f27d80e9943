// libecc_amd/csrc/ecamd_host_msm.cpp -- host side of the C ABI declared in include/libecc_amd.h: the Schnorr-type whole-batch verification as
// one multi-scalar multiplication (BIP0340, ECFSDSA; Ed448's whole-batch form runs the same evaluation), and the seed of its z_i
// (ecamd_host_internal.h says what the host units share and how they are laid out).
#include "ecamd_host_internal.h"

using namespace ecamd_host;

// key of the z_i of the batch equation: the caller's 32 bytes when ecamd_ctx_set_msm_seed left some (used once), else getrandom
int ecamd_host::msm_seed(ecamd_ctx *ctx, uint8_t seed[32])
{
	if (ctx->msm_seed_valid) {
		memcpy(seed, ctx->msm_seed_bytes, 32);
		memset(ctx->msm_seed_bytes, 0, 32);
		ctx->msm_seed_valid = false;
		return 0;
	}
	size_t got = 0;
	while (got < 32) {
		const ssize_t r = getrandom(seed + got, 32 - got, 0);
		if (r <= 0) {
			return fail("ec_eddsa_verify_all_batch: getrandom failed (the z_i of the batch equation must be unpredictable)");
		}
		got += (size_t)r;
	}
	return 0;
}
// the seed of ecamd_ctx_set_msm_seed keys ONE whole-batch call: whichever path that call took (Ed448, a batch below msm_min,
// mode 0, an error), it is gone afterwards
void ecamd_host::msm_seed_discard(ecamd_ctx *ctx)
{
	if (ctx) {
		std::lock_guard<std::mutex> lk(ctx->mu);
		if (ctx->msm_seed_valid) {
			memset(ctx->msm_seed_bytes, 0, sizeof(ctx->msm_seed_bytes));
			ctx->msm_seed_valid = false;
		}
	}
}
// the bucket evaluation FILED CHUNK BY CHUNK (ec_schnorr_verify_msg_all_batch): which part of schnorr_msm_dev_locked a call runs
struct SchnorrStreamStep {
	int mode;                // 1: scratch sized, flag word and counters cleared; 2: the items [first, first + count) imported, their scalars
	                         // formed, filed; 3: c and [c]G, the ranking, the buckets summed, reduced and compared
	uint32_t first, count;
};

// ------------------------------------------------------------------------------------------
// Schnorr-type whole-batch verification on a short-Weierstrass curve as one multi-scalar multiplication (EcamdMsmArgs in
// ecamd_internal.h; BIP0340's and ECFSDSA's batch equation, sig/bip0340.c:808-1025, sig/ecfsdsa.c:657-837): per piece of at most
// max_chunk items   k_msm_scal (z_i, z_i (q - e_i), z_i s_i mod q)  ->  k_msm_vsum (c = sum z_i s_i)  ->  [c]G by the handle's
// fixed-base path  ->  k_msm_table_g (2n window tables)  ->  k_msm_loop_g (Straus, K items per lane)  ->  k_msm_sum_g / final.
// ------------------------------------------------------------------------------------------
bool ecamd_host::schnorr_msm_unit(const ecamd_curve *cv, int *pbits, int *flavour, int *slot)
{
	if (cv->gslot >= 0) {
		*pbits = cv->pbits;
		*flavour = cv->gflavour;
		*slot = cv->gslot;
		return true;
	}
	if (cv->is_p256 && cv->gpslot >= 0) {   // secp256r1: the dense 256-bit unit that serves its projective import
		*pbits = 256;
		*flavour = 0;
		*slot = cv->gpslot;
		return true;
	}
	return false;
}

static uint32_t schnorr_msm_pick_k(uint32_t n)
{
	if (const char *e = getenv("ECAMD_SCHNORR_MSM_K")) {
		const uint32_t k = (uint32_t)strtoul(e, nullptr, 10);
		if (k >= 1 && k <= 64) {
			return k;
		}
	}
	// measured on secp256k1 (profiles/r5h_schnorr_msm.md): the Straus loop wants about 2^18 lanes (four waves per SIMD: its additions are
	// dependent chains) before sharing doublings pays -- 2^20 items: K = 4 (19.3 ms) beats 8 (23.1) and 2 (20.6); 2^18 items: K = 1
	uint32_t k = n >> 18;
	if (k < 1) {
		k = 1;
	}
	return k > 8 ? 8 : k;
}

// Straus (round 5) or buckets (round 6) for a piece of n items.  Buckets: windows of 16 bits -- z_i has 128 = 8 x 16 of them, and the
// orders of the usual curves a multiple of 16 -- from 2^17 items on (below, the fixed costs of the sort and of the reduction over 2^16
// buckets per window outweigh the additions they save: profiles/r6h_schnorr_bucket.md), and only when the order's TOP window still has
// at least 12 bits: a top window of t bits files n points into 2^t buckets, each added up by one lane (secp521r1: 9 bits, secp224k1:
// 1 bit -- those keep the Straus loop).  $ECAMD_SCHNORR_MSM_ALGO=straus|bucket overrides the size rule (tests, measurements).
static bool schnorr_msm_use_buckets(const ecamd_curve *cv, uint32_t n)
{
	const uint32_t top_bits = (uint32_t)cv->qbits - 16u * (((uint32_t)cv->qbits - 1u) / 16u);
	if (top_bits < 12u) {
		return false;
	}
	if (const char *e = getenv("ECAMD_SCHNORR_MSM_ALGO")) {
		if (!strcmp(e, "straus")) {
			return false;
		}
		if (!strcmp(e, "bucket")) {
			return true;
		}
	}
	return n >= (1u << 17);
}
static uint32_t schnorr_bkt_window(uint32_t) { return 16u; }
// the streamed form (SchnorrStreamStep) files into fixed-capacity buckets and ends on the side stream's joins
static bool schnorr_msm_streams(const ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n)
{
	return n <= ctx->max_chunk && schnorr_msm_use_buckets(cv, n) && ctx->side_ok && getenv("ECAMD_NO_BKT_BESIDE") == nullptr &&
	       getenv("ECAMD_BKT_EXACT_SORT") == nullptr && getenv("ECAMD_NO_SCHNORR_STREAM") == nullptr;
}

int ecamd_host::schnorr_msm_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_s, const uint8_t *d_ne, const uint8_t *d_keys,
				  const uint8_t *d_r, int r_fmt, const uint8_t seed[32], uint32_t piece, uint8_t *d_verdict, uint8_t *d_z_dump,
				  uint32_t *d_sum_dump, hipStream_t s, uint32_t cof_dbl, const SchnorrStreamStep *step)
{
	const int mode = step ? step->mode : 0;
	// cof_dbl > 0 (eddsa448_msm_dev_locked only): the final test is [2^cof_dbl](sum + [c]G) = infinity, EdDSA's cofactored equation
	int pbits = 0, flav = 0, gslot = -1;
	if (!schnorr_msm_unit(cv, &pbits, &flav, &gslot) || cv->qslot < 0) {
		return fail("internal: Schnorr multi-scalar multiplication without a radix-2^29 unit");
	}
	const bool buckets = schnorr_msm_use_buckets(cv, n);
	const uint32_t K = schnorr_msm_pick_k(n);
	const uint32_t L = (n + K - 1) / K;
	const size_t itemw = ecamd_g29_table_words(pbits, flav), recw = ecamd_g29_msm_rec_words(pbits, flav);
	const size_t cl = (size_t)cv->clen, ql = (size_t)cv->qlen, qnw = (size_t)cv->qnw;
	// bucket evaluation: window bits, windows of the full-length scalars / of the 128-bit z_i, counters, reduction scratch
	const uint32_t bc = schnorr_bkt_window(n), bnwin = (uint32_t)((8 * ql + bc - 1) / bc), bnwinZ = (128u + bc - 1) / bc;
	const size_t bcounters = (size_t)bnwin << bc, bpw = ecamd_g29_bkt_point_words(pbits, flav);
	const size_t bfold = ecamd_bkt_fold();
	const size_t bred_words = 2 * (2 * (size_t)bnwin * ((((size_t)1 << bc) + bfold - 1) / bfold) * recw + ((size_t)bnwin + 2) * recw);
	size_t off = 0;
	auto carve = [&](size_t bytes) {
		const size_t o = off;
		off += msm_align(bytes);
		return o;
	};
	const size_t o_tbl = carve(buckets ? (size_t)2 * n * bpw * 4 : (size_t)2 * n * itemw * 4);
	const size_t o_rec = carve(buckets ? bcounters * recw * 4 : (size_t)L * recw * 4);
	const size_t o_tmp = carve(buckets ? bred_words * 4 : ((size_t)L / 16 + 2) * recw * 4);
	// fixed-capacity filing unless $ECAMD_BKT_EXACT_SORT: 32 + 2 lambda slots per bucket, lambda = 2n / 2^16 the mean of the fullest windows
	const uint32_t bcap = getenv("ECAMD_BKT_EXACT_SORT") ? 0u : 32u + 2u * (uint32_t)(((size_t)2 * n + 65535) >> 16);
	// ... and the order's TOP window: z_i (q - e_i) < q, so its digits take (q >> 16 top_win) + 1 values only and the n keys crowd into that many
	// buckets (brainpoolP256r1: 43 516 of 65 536; an order just above a power of 2^16: a few) -- a capacity of its own
	const uint32_t btop = ((uint32_t)cv->qbits - 1u) / 16u;
	uint32_t btopvals = 1;
	{
		const uint32_t bit = 16u * btop;   // the digit of q itself in that window, + 1
		const size_t wi = bit / 32u;
		const uint32_t word = wi < cv->q.size() ? cv->q[wi] : 0u;
		btopvals = ((word >> (bit % 32u)) & 0xffffu) + 1u;
	}
	const uint32_t bcap_top = bcap ? 32u + 2u * (uint32_t)(((size_t)n + btopvals - 1) / btopvals) : 0u;
	const size_t o_cnt = carve(buckets ? 4 * bcounters * 4 : 0);
	const size_t o_ord = carve(buckets ? (bcap ? ((size_t)btop << 16) * bcap * 4 + ((size_t)(bnwin - btop) << 16) * bcap_top * 4 : (size_t)bnwin * 2 * n * 4) : 0);
	const size_t o_w = carve((size_t)n * ql), o_z = carve((size_t)n * 16), o_v = carve((size_t)n * qnw * 4);
	const size_t o_v1 = carve(((size_t)n / 64 + 2) * qnw * 4), o_v2 = carve(((size_t)n / 4096 + 2) * qnw * 4);
	const size_t o_c = carve(ql), o_gen = carve(2 * cl), o_gst = carve(4), o_word = carve(4);
	if (ensure(&ctx->msm, &ctx->msm_bytes, off)) {
		return -1;
	}
	uint8_t *M = ctx->msm;
	if (mode <= 1) {
		HIPCHK(hipMemsetAsync(M + o_word, 0, 4, s));
	}
	if (mode == 1) {
		HIPCHK(hipMemsetAsync(M + o_cnt, 0, bcounters * 4, s));   // (the filing's counters)
		return 0;
	}
	if (mode == 2) {
		// one staging chunk of the streamed form, everything on the caller's stream: the keys' and the commitments' import, the scalars, the filing
		EcamdMsmArgs P;
		memset(&P, 0, sizeof(P));
		P.ptsY = d_keys;
		P.ptsR = d_r;
		P.flagword = (uint32_t *)(M + o_word);
		P.pts = (uint32_t *)(M + o_tbl);
		P.n = n;
		P.clen = (uint32_t)cl;
		P.r_fmt = (uint32_t)r_fmt;
		P.cof_dbl = cof_dbl;
		P.pt_first = step->first;
		P.pt_count = step->count;
		HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 10, P, nullptr, nullptr, nullptr, nullptr, nullptr, s));
		P.pt_first = n + step->first;
		HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 10, P, nullptr, nullptr, nullptr, nullptr, nullptr, s));
	}
	bool points_beside = mode == 3;   // (the streamed form asked schnorr_msm_streams first: buckets, a side stream)
	if (mode == 0 && buckets && ctx->side_ok && getenv("ECAMD_NO_BKT_BESIDE") == nullptr) {
		// the import of the 2n points (on-curve checks, BIP0340's square roots: VALU work that reads only the caller's arrays) runs on the side
		// stream beside the scalar kernels and the counting sort (atomics and scattered stores); the bucket additions wait for both
		EcamdMsmArgs P;
		memset(&P, 0, sizeof(P));
		P.ptsY = d_keys;
		P.ptsR = d_r;
		P.flagword = (uint32_t *)(M + o_word);
		P.pts = (uint32_t *)(M + o_tbl);
		P.n = n;
		P.clen = (uint32_t)cl;
		P.r_fmt = (uint32_t)r_fmt;
		P.cof_dbl = cof_dbl;
		HIPCHK(hipEventRecord(ctx->side_fork, s));
		HIPCHK(hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0));
		// the keys first (an on-curve check each): the windows above z_i's 128 bits hold keys only and can be added up while the
		// commitments are still being lifted (a square root each)
		P.pt_first = 0;
		P.pt_count = n;
		HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 10, P, nullptr, nullptr, nullptr, nullptr, nullptr, ctx->side_stream));
		HIPCHK(hipEventRecord(ctx->side_mid, ctx->side_stream));
		P.pt_first = n;
		HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 10, P, nullptr, nullptr, nullptr, nullptr, nullptr, ctx->side_stream));
		HIPCHK(hipEventRecord(ctx->side_done, ctx->side_stream));
		points_beside = true;
	}
	EcamdMsmScalArgs C;
	memset(&C, 0, sizeof(C));
	C.s = d_s;
	C.ne = d_ne;
	C.scW = M + o_w;
	C.scZ = M + o_z;
	C.v = (uint32_t *)(M + o_v);
	C.flagword = (uint32_t *)(M + o_word);
	C.z_dump = d_z_dump;
	memcpy(C.seed, seed, 32);
	C.nonce[0] = piece;
	C.nonce[1] = 0x5343484eu;   // "SCHN": another stream than the Ed25519 combination's under the same seed
	C.n = n;
	C.qlen = (uint32_t)ql;
	C.qslot = cv->qslot;
	if (mode == 2) {
		C.first = step->first;
		C.count = step->count;
	}
	if (mode != 3) {
		HIPCHK(ecamd_launch_msm_scal(cv->qnw, C, s));
	}
	if (mode == 2) {
		uint32_t *cnt = (uint32_t *)(M + o_cnt);
		EcamdBktSortArgs B;
		memset(&B, 0, sizeof(B));
		B.scW = M + o_w;
		B.scZ = M + o_z;
		B.hist = cnt;
		B.cap = bcap;
		B.cap_top = bcap_top;
		B.top_win = btop;
		B.flag = (uint32_t *)(M + o_word);
		B.order = (uint32_t *)(M + o_ord);
		B.n = n;
		B.wlen = (uint32_t)ql;
		B.zlen = 16;
		B.c = bc;
		B.nwin = bnwin;
		B.nwinZ = bnwinZ < bnwin ? bnwinZ : bnwin;
		B.part = 1;
		B.item_first = step->first;
		B.item_count = step->count;
		HIPCHK(ecamd_launch_bkt_sort(B, s));
		return 0;
	}
	// c = sum z_i s_i and [c]G: four tiny reduction launches and a one-item fixed-base multiplication, a latency-bound chain of 0.7 ms that
	// only the final comparison needs -- on the side stream behind the points when there is one, beside the counting sort
	hipStream_t vs = s;
	if (points_beside) {
		HIPCHK(hipEventRecord(ctx->side_fork, s));
		HIPCHK(hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0));
		vs = ctx->side_stream;
	}
	{
		// c = sum v_i mod q: levels of fan-in 64, the last one writes the big-endian bytes
		EcamdMsmVsumArgs V;
		memset(&V, 0, sizeof(V));
		V.qlen = (uint32_t)ql;
		V.qslot = cv->qslot;
		const uint32_t *src = (const uint32_t *)(M + o_v);
		uint32_t *bufs[2] = {(uint32_t *)(M + o_v1), (uint32_t *)(M + o_v2)};
		uint32_t count = n;
		int b = 0;
		do {
			const uint32_t outc = (count + 63) / 64;
			V.in = src;
			V.out = bufs[b];
			V.count = count;
			V.c_be = outc == 1 ? M + o_c : nullptr;
			HIPCHK(ecamd_launch_msm_vsum(cv->qnw, V, vs));
			src = bufs[b];
			b ^= 1;
			count = outc;
		} while (count > 1);
	}
	// [c]G from the handle's own fixed-base path, one item, device pointers (the comb table is built for a batch of this size: without
	// it the single item would walk the whole window loop alone, a millisecond of latency)
	maybe_build_comb(ctx, const_cast<ecamd_curve *>(cv), n);
	if (smul_dev_locked(ctx, cv, 1, M + o_c, (uint32_t)ql, nullptr, M + o_gen, M + o_gst, vs, 0xffffffffu, false, nullptr)) {
		return -1;
	}
	if (points_beside) {
		HIPCHK(hipEventRecord(ctx->side_aux, ctx->side_stream));
	}
	EcamdMsmArgs A;
	memset(&A, 0, sizeof(A));
	A.ptsY = d_keys;
	A.ptsR = d_r;
	A.scW = M + o_w;
	A.scZ = M + o_z;
	A.tbl = (uint32_t *)(M + o_tbl);
	A.rec = (uint32_t *)(M + o_rec);
	A.flagword = (uint32_t *)(M + o_word);
	A.n = n;
	A.K = K;
	A.L = L;
	A.clen = (uint32_t)cl;
	A.wlen = (uint32_t)ql;
	A.zlen = 16;
	A.r_fmt = (uint32_t)r_fmt;
	A.cof_dbl = cof_dbl;
	if (buckets) {
		A.pts = (uint32_t *)(M + o_tbl);
		A.bsum = (uint32_t *)(M + o_rec);
		A.red = (uint32_t *)(M + o_tmp);
		A.red_words = bred_words;
		A.c = bc;
		A.nwin = bnwin;
		uint32_t *cnt = (uint32_t *)(M + o_cnt);
		A.bcount = cnt;
		A.bstart = cnt + bcounters;
		A.order = (const uint32_t *)(M + o_ord);
		EcamdBktSortArgs B;
		memset(&B, 0, sizeof(B));
		B.scW = M + o_w;
		B.scZ = M + o_z;
		B.hist = cnt;
		B.start = cnt + bcounters;
		B.cursor = cnt + 2 * bcounters;
		B.perm = getenv("ECAMD_NO_BKT_RANK") ? nullptr : cnt + 3 * bcounters;
		A.perm = B.perm;
		B.cap = A.cap = bcap;
		B.cap_top = A.cap_top = bcap_top;
		B.top_win = A.top_win = btop;
		B.flag = (uint32_t *)(M + o_word);
		B.order = (uint32_t *)(M + o_ord);
		B.n = n;
		B.wlen = (uint32_t)ql;
		B.zlen = 16;
		B.c = bc;
		B.nwin = bnwin;
		B.nwinZ = bnwinZ < bnwin ? bnwinZ : bnwin;
		// $ECAMD_BKT_FILE_SPLIT (off by default): the key-only windows filed first, on the caller's stream, and summed while the windows below
		// 2^128 are filed on a stream of their own.  Measured (profiles/r6_f4_kernels.md): secp256k1 2^20 items 6.91 -> 7.35 ms, Ed448 25.8 -> 25.7 --
		// the filing's atomics and scattered stores slow the gathers of the accumulation they run beside by more than the wait they save
		const bool file_split = mode == 0 && points_beside && B.nwinZ < bnwin && bcap != 0u && ctx->side2_ok && getenv("ECAMD_BKT_FILE_SPLIT") != nullptr;
		if (file_split) {
			HIPCHK(hipMemsetAsync(B.hist, 0, bcounters * 4, s));
			B.win_first = B.nwinZ;
			B.win_count = bnwin - B.nwinZ;
			HIPCHK(ecamd_launch_bkt_sort(B, s));
			HIPCHK(hipEventRecord(ctx->side2_fork, s));
			HIPCHK(hipStreamWaitEvent(ctx->side2_stream, ctx->side2_fork, 0));
			B.win_first = 0;
			B.win_count = B.nwinZ;
			HIPCHK(ecamd_launch_bkt_sort(B, ctx->side2_stream));
			HIPCHK(hipEventRecord(ctx->side2_done, ctx->side2_stream));
		} else {
			B.part = mode == 3 ? 2u : 0u;   // (the streamed form has filed everything: the ranking alone)
			HIPCHK(ecamd_launch_bkt_sort(B, s));
		}
		uint32_t *d_total = (uint32_t *)(M + o_tmp) + bred_words - recw;
		if (!points_beside) {
			HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 10, A, nullptr, nullptr, nullptr, nullptr, nullptr, s));
		}
		if (ctx->timing) {   // the dominant kernel: k_bkt_accum_g, both launches (ecamd_ctx_dominant_kernel_ms)
			HIPCHK(hipEventRecord(ctx->ev_dom[0], s));
		}
		bool reduced = false;
		if (points_beside && B.nwinZ < bnwin) {
			// the windows that hold keys only, as soon as the keys are in; then the rest once the commitments are
			if (mode == 0) {
				HIPCHK(hipStreamWaitEvent(s, ctx->side_mid, 0));
			}
			A.win_first = B.nwinZ;
			A.win_count = bnwin - B.nwinZ;
			HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 11, A, nullptr, nullptr, nullptr, nullptr, nullptr, s));
			const bool red_beside = getenv("ECAMD_NO_BKT_RED_BESIDE") == nullptr;
			if (red_beside) {
				// ... and their reduction on the side stream (idle by now: the commitments and [c]G are short) while the other windows are
				// still being summed: the doubling chain of window w is 16 w long -- one lane per window, latency-bound -- and these are the
				// long ones; the windows below 2^128 then end in chains of at most 112 doublings
				HIPCHK(hipEventRecord(ctx->side_hi, s));
				HIPCHK(hipStreamWaitEvent(ctx->side_stream, ctx->side_hi, 0));
				HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 12, A, nullptr, nullptr, nullptr, nullptr, nullptr, ctx->side_stream));
				HIPCHK(hipEventRecord(ctx->side_red, ctx->side_stream));
			}
			if (mode == 0) {
				HIPCHK(hipStreamWaitEvent(s, ctx->side_done, 0));
			}
			if (file_split) {
				HIPCHK(hipStreamWaitEvent(s, ctx->side2_done, 0));
			}
			A.win_first = 0;
			A.win_count = B.nwinZ;
			HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 11, A, nullptr, nullptr, nullptr, nullptr, nullptr, s));
			if (red_beside) {
				if (ctx->timing) {
					HIPCHK(hipEventRecord(ctx->ev_dom[1], s));
					ctx->ev_dom_valid = true;
				}
				HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 12, A, nullptr, nullptr, nullptr, nullptr, nullptr, s));
				HIPCHK(hipStreamWaitEvent(s, ctx->side_red, 0));
				A.win_count = 0;
				HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 14, A, nullptr, nullptr, nullptr, nullptr, nullptr, s));
				reduced = true;
			}
			A.win_count = 0;
		} else {
			if (points_beside && mode == 0) {
				HIPCHK(hipStreamWaitEvent(s, ctx->side_done, 0));
			}
			HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 11, A, nullptr, nullptr, nullptr, nullptr, nullptr, s));
		}
		if (!reduced) {
			if (ctx->timing) {
				HIPCHK(hipEventRecord(ctx->ev_dom[1], s));
				ctx->ev_dom_valid = true;
			}
			HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 12, A, nullptr, nullptr, nullptr, nullptr, nullptr, s));
		}
		if (points_beside) {
			HIPCHK(hipStreamWaitEvent(s, ctx->side_aux, 0));   // [c]G
		}
		HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, 13, A, d_total, M + o_gen, M + o_gst, d_verdict, d_sum_dump, s));
		return 0;
	}
	for (int phase = 0; phase < 3; phase++) {
		const bool timed = ctx->timing && phase == 1;   // the dominant kernel: k_msm_loop_g (ecamd_ctx_dominant_kernel_ms)
		if (timed) {
			HIPCHK(hipEventRecord(ctx->ev_dom[0], s));
		}
		HIPCHK(ecamd_launch_msm_g29(pbits, gslot, flav, phase, A, (uint32_t *)(M + o_tmp), M + o_gen, M + o_gst, d_verdict, d_sum_dump, s));
		if (timed) {
			HIPCHK(hipEventRecord(ctx->ev_dom[1], s));
			ctx->ev_dom_valid = true;
		}
	}
	return 0;
}

static int schnorr_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *a, const void *b, const void *c,
			   const void *d, int r_fmt, const void *out)
{
	if (!ctx || !cv || cv->ctx != ctx || !out || n == 0 || !a || !b || !c || !d || (r_fmt != 0 && r_fmt != 1)) {
		return fail(std::string(fn) + ": bad argument (the reference rejects num = 0 too)");
	}
	return 0;
}

// 1: the multi-scalar form can serve this handle (a radix-2^29 unit; q usable as a modulus of at least 160 bits; for r_fmt 1, p = 3 mod 4)
static bool schnorr_msm_available(const ecamd_curve *cv, int r_fmt)
{
	int pb, fl, sl;
	if (!schnorr_msm_unit(cv, &pb, &fl, &sl) || cv->qslot < 0 || cv->qbits < 160 || (uint32_t)cv->qlen < 16u) {
		return false;
	}
	// Prime-order groups only.  On a curve with a cofactor a commitment R + D, D of small order, is rejected by the item
	// form but passes the random combination whenever z_i D = O -- with probability 1 / ord(D), up to 1/2 -- so the batch form would accept
	// what a loop of ec_verify rejects (the reference's batch has that weakness; this one must not).  Such curves take the item form.
	if (cv->cofactor != 1) {
		return false;
	}
	if (r_fmt == 1 && (cv->p[0] & 3u) != 3u) {
		return false;
	}
	return true;
}

int ecamd_host::schnorr_msm_host_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *sv, const uint8_t *ne, const uint8_t *keys,
				   const uint8_t *r, int r_fmt, const uint8_t *fixed_seed, int *accept, uint8_t *z_out, uint32_t *sum_out)
{
	uint8_t seed[32];
	if (fixed_seed) {
		memcpy(seed, fixed_seed, 32);
	} else if (msm_seed(ctx, seed)) {
		return -1;
	}
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	PublicScalars pub_scope(ctx);   // everything a verification multiplies by is public
	const size_t cl = (size_t)cv->clen, ql = (size_t)cv->qlen, rl = r_fmt ? cl : 2 * cl;
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	const uint32_t pieces = (n + chunk - 1) / chunk;
	int pb, fl, sl;
	(void)schnorr_msm_unit(cv, &pb, &fl, &sl);
	const size_t recw = ecamd_g29_msm_rec_words(pb, fl);
	if (stage_need(ctx, MS_S, (size_t)chunk * ql) || stage_need(ctx, MS_NE, (size_t)chunk * ql) ||
	    stage_need(ctx, MS_KEYS, (size_t)chunk * 2 * cl) || stage_need(ctx, MS_R, (size_t)chunk * rl) ||
	    stage_need(ctx, MS_VERDICTS, (size_t)pieces + (z_out ? (size_t)chunk * 16 : 0) + 512 + recw * 4)) {
		return -1;
	}
	uint8_t *d_verdicts = ctx->stage[MS_VERDICTS];
	HIPCHK(hipMemsetAsync(d_verdicts, 1, pieces, s));
	uint32_t *d_sum = (uint32_t *)(ctx->stage[MS_VERDICTS] + ((pieces + 255) & ~(size_t)255));
	uint8_t *d_z = z_out ? (uint8_t *)(d_sum + recw) : nullptr;
	for (uint32_t off = 0, pc = 0; off < n; off += chunk, pc++) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		HIPCHK(hipMemcpyAsync(ctx->stage[MS_S], sv + (size_t)off * ql, (size_t)m * ql, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(ctx->stage[MS_NE], ne + (size_t)off * ql, (size_t)m * ql, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(ctx->stage[MS_KEYS], keys + (size_t)off * 2 * cl, (size_t)m * 2 * cl, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(ctx->stage[MS_R], r + (size_t)off * rl, (size_t)m * rl, hipMemcpyHostToDevice, s));
		if (schnorr_msm_dev_locked(ctx, cv, m, ctx->stage[MS_S], ctx->stage[MS_NE], ctx->stage[MS_KEYS], ctx->stage[MS_R], r_fmt, seed, pc, d_verdicts + pc, d_z,
					   sum_out ? d_sum : nullptr, s)) {
			(void)hipStreamSynchronize(s);
			return -1;
		}
		if (z_out) {
			HIPCHK(hipMemcpyAsync(z_out + (size_t)off * 16, d_z, (size_t)m * 16, hipMemcpyDeviceToHost, s));
		}
	}
	std::vector<uint8_t> v(pieces, 1);
	HIPCHK(hipMemcpyAsync(v.data(), d_verdicts, pieces, hipMemcpyDeviceToHost, s));
	if (sum_out) {
		HIPCHK(hipMemcpyAsync(sum_out, d_sum, recw * 4, hipMemcpyDeviceToHost, s));
	}
	HIPCHK(hipStreamSynchronize(s));
	memset(seed, 0, sizeof(seed));
	*accept = 1;
	for (uint32_t pc = 0; pc < pieces; pc++) {
		if (v[pc] != 0) {
			*accept = 0;
		}
	}
	return 0;
}

extern "C" int ec_schnorr_verify_all_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *s, const uint8_t *ne,
					   const uint8_t *keys_aff, const uint8_t *r, int r_fmt, int *all_valid)
{
	if (schnorr_args_ok("ec_schnorr_verify_all_batch", ctx, cv, n, s, ne, keys_aff, r, r_fmt, all_valid)) {
		return -1;
	}
	*all_valid = 0;
	int ret = 0;
	{
		std::lock_guard<std::mutex> lk(ctx->mu);
		HIPCHK(hipSetDevice(ctx->device));
		if (schnorr_msm_available(cv, r_fmt)) {
			ret = schnorr_msm_host_locked(ctx, cv, n, s, ne, keys_aff, r, r_fmt, nullptr, all_valid, nullptr, nullptr);
		}   // else: not decided here, the caller verifies item by item
	}
	// the seed of ecamd_ctx_set_msm_seed keys THIS call only: whichever way it ended ("not available", an error before the seed was
	// read), nothing stays pending for an unrelated whole-batch call
	msm_seed_discard(ctx);
	return ret;
}

// The combination alone, device pointers, one piece (n <= the context's max_chunk): d_verdict[0] = 0 when the batch equation holds and no
// exceptional event was met, 1 otherwise ("not decided here").  Only enqueues on the stream.
extern "C" int ec_schnorr_verify_all_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *d_s, const void *d_ne,
						   const void *d_keys_aff, const void *d_r, int r_fmt, void *d_verdict, void *hip_stream)
{
	if (schnorr_args_ok("ec_schnorr_verify_all_batch_dev", ctx, cv, n, d_s, d_ne, d_keys_aff, d_r, r_fmt, d_verdict)) {
		return -1;
	}
	int ret = -1;
	{
		std::lock_guard<std::mutex> lk(ctx->mu);
		HIPCHK(hipSetDevice(ctx->device));
		if (n > ctx->max_chunk || !schnorr_msm_available(cv, r_fmt)) {
			ret = fail("ec_schnorr_verify_all_batch_dev: needs a prime-order curve with a radix-2^29 unit (ec_schnorr_verify_all_available) and n <= max_chunk");
		} else {
			uint8_t seed[32];
			if (!msm_seed(ctx, seed)) {
				hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
				StreamScope scope(ctx, s);
				PublicScalars pub_scope(ctx);
				if (hipMemsetAsync(d_verdict, 1, 1, s) == hipSuccess) {
					ret = schnorr_msm_dev_locked(ctx, cv, n, (const uint8_t *)d_s, (const uint8_t *)d_ne, (const uint8_t *)d_keys_aff,
								     (const uint8_t *)d_r, r_fmt, seed, 0, (uint8_t *)d_verdict, nullptr, nullptr, s);
				}
				memset(seed, 0, sizeof(seed));
			}
		}
	}
	msm_seed_discard(ctx);
	return ret;
}

// BIP0340 / ECFSDSA whole-batch verification FROM keys, signatures and hash inputs (round 6): what libsign_amd.so's ec_verify_batch needs
// so that nothing but marshalling stays on the host.  Per chunk of the double-buffered staging: the keys are imported and normalised on
// the device (k_prj_import_g; affine keys go as they are), k_schnorr_prep writes the key's x into the blank of the item's hash input
// (BIP0340: e = H(H(tag) || H(tag) || r || Y.x || m), sig/bip0340.c:437-494 -- the caller supplies everything but Y.x) and files the key as
// the equation uses it (the even-y representative), s and the commitment in batch-wide arrays; the hash inputs are hashed
// (k_sha2_slots) and k_schnorr_ne leaves q - e.  When the last chunk is in, the batch is ONE multi-scalar multiplication per max_chunk
// items (schnorr_msm_dev_locked): the copies of the 200 MB a 2^20-item batch brings hide behind the front-end kernels, and the
// Straus loop runs at its full-batch rate.  *all_valid = 0: not decided here (see ec_schnorr_verify_all_batch).
extern "C" int ec_schnorr_verify_msg_all_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *keys, int key_fmt,
						   const uint8_t *sigs, int r_fmt, int hash_type, const uint8_t *hash_slots, uint32_t stride,
						   uint32_t x_offset, int *all_valid)
{
	if (schnorr_args_ok("ec_schnorr_verify_msg_all_batch", ctx, cv, n, keys, sigs, hash_slots, hash_slots, r_fmt, all_valid)) {
		return -1;
	}
	*all_valid = 0;
	const int hl = ecamd_sha2_digest_len(hash_type);
	const size_t cl = (size_t)cv->clen, ql = (size_t)cv->qlen, rl = r_fmt ? cl : 2 * cl, sl = rl + ql;
	if ((key_fmt != ECAMD_PT_AFFINE && key_fmt != ECAMD_PT_PROJECTIVE) || hl == 0 || stride < 4 || (stride & 3u) || stride > 4096 ||
	    (x_offset != 0xffffffffu && (uint64_t)x_offset + 4 + cl > stride) || cl > 72) {
		return fail("ec_schnorr_verify_msg_all_batch: bad argument (key_fmt ECAMD_PT_AFFINE / _PROJECTIVE; hash_type 1 .. 4 (SHA-224 / 256 / 384 / 512); stride a "
			    "multiple of 4 in 4 .. 4096; the blank for the key's x, if any, inside the slot)");
	}
	int ret = 0;
	{
		std::lock_guard<std::mutex> lk(ctx->mu);
		HIPCHK(hipSetDevice(ctx->device));
		if (schnorr_msm_available(cv, r_fmt)) {
			ret = -1;
			uint8_t seed[32];
			const size_t kw = (key_fmt == ECAMD_PT_PROJECTIVE ? 3 : 2) * cl;
			// batch-wide arrays: 24 s, 25 q - e, 26 keys, 27 commitments, 28 the front end's flag word and the verdicts
			const uint32_t pieces = (n + ctx->max_chunk - 1) / ctx->max_chunk;
			if (!msm_seed(ctx, seed) && !stage_need(ctx, BW_S, (size_t)n * ql) &&
			    !stage_need(ctx, BW_NE, (size_t)n * ql) && !stage_need(ctx, BW_KEYS, (size_t)n * 2 * cl) &&
			    !stage_need(ctx, BW_R, (size_t)n * rl) && !stage_need(ctx, BW_VERDICTS, 256 + (size_t)pieces)) {
				uint8_t **S = ctx->stage;
				uint32_t *d_flag = (uint32_t *)S[BW_VERDICTS];
				uint8_t *d_verdicts = S[BW_VERDICTS] + 256;
				uint32_t done = 0;
				PublicScalars pub_scope(ctx);   // everything a verification multiplies by is public
				EcamdSchnorrPrepArgs P;
				memset(&P, 0, sizeof(P));
				big_to_be(P.p_be, (int)cl, cv->p);
				EcamdSchnorrNeArgs N;
				memset(&N, 0, sizeof(N));
				for (int w = 0; w < 18; w++) {
					N.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
				}
				bool first = true;
				const std::vector<HostArr> arrs = {{keys, nullptr, kw}, {sigs, nullptr, sl}, {hash_slots, nullptr, stride}};
				// One piece, by buckets: the combination's per-item stages (the 2n points' import, the scalars, the filing) on every chunk as it
				// lands, in even chunks of 2^17 items -- what waits for the last chunk is the ranking, the additions and the reduction
				// ($ECAMD_NO_SCHNORR_STREAM: the whole combination after the last chunk, as for batches of several pieces)
				const bool streamed = schnorr_msm_streams(ctx, cv, n);
				SchnorrStreamStep step = {1, 0, 0};
				int begun = 0;
				if (streamed) {
					StreamScope scope(ctx, ctx->stream);
					begun = schnorr_msm_dev_locked(ctx, cv, n, S[BW_S], S[BW_NE], S[BW_KEYS], S[BW_R], r_fmt, seed, 0, d_verdicts, nullptr, nullptr, ctx->stream, 0, &step);
				}
				int rc = begun ? -1 : host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &,
										     hipStream_t s, const Between &) {
					if (first) {
						HIPCHK(hipMemsetAsync(d_flag, 0, 4, s));
						HIPCHK(hipMemsetAsync(d_verdicts, 1, pieces, s));
						first = false;
					}
					const uint8_t *d_aff = ip[0], *d_kst = nullptr;
					if (key_fmt == ECAMD_PT_PROJECTIVE) {
						if (stage_need(ctx, SI_PRJ_AFF, (size_t)m * 2 * cl) || stage_need(ctx, SI_PRJ_ST, m)) {
							return -1;
						}
						EcamdPrjInArgs I;
						I.in = ip[0];
						I.aff = S[SI_PRJ_AFF];
						I.pre = S[SI_PRJ_ST];
						I.n = m;
						I.clen = (uint32_t)cl;
						I.for_mul = 0;
						I.slot = cv->slot;
						HIPCHK(launch_prj_import(cv, I, s));
						d_aff = S[SI_PRJ_AFF];
						d_kst = S[SI_PRJ_ST];
					}
					P.keys_aff = d_aff;
					P.kst = d_kst;
					P.sigs = ip[1];
					P.slots = const_cast<uint8_t *>(ip[2]);   // the staged copy of the caller's slots
					P.keys_out = S[BW_KEYS] + (size_t)done * 2 * cl;
					P.s_out = S[BW_S] + (size_t)done * ql;
					P.r_out = S[BW_R] + (size_t)done * rl;
					P.flag = d_flag;
					P.n = m;
					P.clen = (uint32_t)cl;
					P.qlen = (uint32_t)ql;
					P.rlen = (uint32_t)rl;
					P.stride = stride;
					P.x_off = x_offset;
					P.even_y = r_fmt ? 1u : 0u;
					HIPCHK(ecamd_launch_schnorr_prep(P, s));
					if (ecdsa_hash_stage(ctx, hash_type, m, ip[2], stride, (uint32_t)hl, s)) {
						return -1;
					}
					N.dig = S[ST_DIGESTS];
					N.ne = S[BW_NE] + (size_t)done * ql;
					N.n = m;
					N.hlen = (uint32_t)hl;
					N.qlen = (uint32_t)ql;
					HIPCHK(ecamd_launch_schnorr_ne(cv->qnw, N, s));
					if (streamed) {
						step.mode = 2;
						step.first = done;
						step.count = m;
						if (schnorr_msm_dev_locked(ctx, cv, n, S[BW_S], S[BW_NE], S[BW_KEYS], S[BW_R], r_fmt, seed, 0, d_verdicts, nullptr, nullptr, s, 0, &step)) {
							return -1;
						}
					}
					done += m;
					return 0;
				}, streamed ? (1u << 17) : 0u);
				if (!rc) {
					hipStream_t s = ctx->stream;
					StreamScope scope(ctx, s);
					uint32_t pc = 0;
					if (streamed) {
						step.mode = 3;
						rc = schnorr_msm_dev_locked(ctx, cv, n, S[BW_S], S[BW_NE], S[BW_KEYS], S[BW_R], r_fmt, seed, 0, d_verdicts, nullptr, nullptr, s, 0, &step);
					}
					// (a loop of its own, not for_chunks: pc numbers the pieces for their z_i and verdicts, and a streamed batch skips the walk)
					for (uint32_t off = 0; off < n && !rc && !streamed; off += ctx->max_chunk, pc++) {
						const uint32_t m = (n - off) < ctx->max_chunk ? (n - off) : ctx->max_chunk;
						rc = schnorr_msm_dev_locked(ctx, cv, m, S[BW_S] + (size_t)off * ql, S[BW_NE] + (size_t)off * ql, S[BW_KEYS] + (size_t)off * 2 * cl,
									    S[BW_R] + (size_t)off * rl, r_fmt, seed, pc, d_verdicts + pc, nullptr, nullptr, s);
					}
					std::vector<uint8_t> v(pieces, 1);
					uint32_t flag = 1;
					if (!rc && hipMemcpyAsync(v.data(), d_verdicts, pieces, hipMemcpyDeviceToHost, s) == hipSuccess &&
					    hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess) {
						int ok = flag == 0;
						for (uint32_t k = 0; k < pieces; k++) {
							ok = ok && v[k] == 0;
						}
						*all_valid = ok;
						ret = 0;
					} else {
						(void)hipStreamSynchronize(s);
						if (!rc) {
							ret = fail("ec_schnorr_verify_msg_all_batch: reading the verdict back failed");
						}
					}
				}
			}
			memset(seed, 0, sizeof(seed));
		}   // else: not decided here
	}
	msm_seed_discard(ctx);
	return ret;
}

extern "C" uint32_t ecamd_debug_schnorr_msm_words(const ecamd_curve *cv)
{
	int pb, fl, sl;
	return (cv && schnorr_msm_unit(cv, &pb, &fl, &sl)) ? ecamd_g29_msm_rec_words(pb, fl) : 0u;
}

extern "C" int ec_schnorr_verify_all_available(const ecamd_curve *cv, int r_fmt) { return (cv && schnorr_msm_available(cv, r_fmt)) ? 1 : 0; }

// test hook: the combination with a caller-chosen seed; z_out (n x 16 little-endian) and sum_out (the lanes' Jacobian sum: X, Y, Z digits
// of the unit and an "is infinity" word, ecamd_debug_schnorr_msm_words() words) may be NULL
extern "C" int ecamd_debug_schnorr_msm(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *s, const uint8_t *ne, const uint8_t *keys_aff,
				       const uint8_t *r, int r_fmt, const uint8_t seed[32], int *accept, uint8_t *z_out, uint32_t *sum_out)
{
	if (schnorr_args_ok("ecamd_debug_schnorr_msm", ctx, cv, n, s, ne, keys_aff, r, r_fmt, accept) || !seed) {
		return -1;
	}
	std::lock_guard<std::mutex> lk(ctx->mu);
	HIPCHK(hipSetDevice(ctx->device));
	if (n > ctx->max_chunk || !schnorr_msm_available(cv, r_fmt)) {
		return fail("ecamd_debug_schnorr_msm: needs a radix-2^29 unit for the curve and 0 < n <= max_chunk");
	}
	return schnorr_msm_host_locked(ctx, cv, n, s, ne, keys_aff, r, r_fmt, seed, accept, z_out, sum_out);
}
