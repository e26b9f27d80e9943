// libecc_amd/csrc/ecamd_host_eddsa.cpp -- host side of the C ABI declared in include/libecc_amd.h: EdDSA on the WEI25519 and WEI448 handles
// (verification, the Ed25519 whole-batch evaluation, signing, one-call signing, the ragged-message forms)
// (ecamd_host_internal.h says what the host units share and how they are laid out).
#include "ecamd_host_internal.h"
#include "ecamd_eddsa_sign.h"

using namespace ecamd_host;

// ------------------------------------------------------------------------------------------
// Ed25519 verification: eddsa_import_pub_key (sig/eddsa.c:862) + _eddsa_verify_init (:1846) +
// _eddsa_verify_finalize (:2130) with the hash H(dom || R || A || M) supplied by the caller.
// ------------------------------------------------------------------------------------------
static Big big_inv_p(const Big &a, const Big &p) { return big_powmod(a, big_sub(p, Big(1, 2)), p); }
static Big big_negmod(const Big &a, const Big &p) { return big_mod(big_sub(p, big_mod(a, p)), p); }

// square root for p = 5 mod 8; returns false when n is a non-residue
static bool big_sqrt_5mod8(const Big &n, const Big &p, Big *out)
{
	Big e = big_add(p, Big(1, 3));
	Big q(e.size(), 0);
	for (size_t i = 0; i < e.size(); i++) {
		q[i] = (e[i] >> 3) | ((i + 1 < e.size()) ? (e[i + 1] << 29) : 0u);
	}
	big_trim(q);
	Big c = big_powmod(n, q, p);
	if (big_cmp(big_mulmod(c, c, p), big_mod(n, p)) != 0) {
		c = big_mulmod(c, big_sqrt_m1(p), p);
	}
	*out = c;
	return big_cmp(big_mulmod(c, c, p), big_mod(n, p)) == 0;
}

// constants of the Ed25519 path for this handle; ctx->mu held
static void ed_setup(ecamd_curve *cv)
{
	cv->ed_state = -1;
	if (!(cv->pbits == 255 && cv->clen == 32 && cv->nw == 8 && cv->qslot >= 0 &&
	      big_cmp(cv->p, big_sub(big_pow2(255), Big(1, 19))) == 0)) {
		cv->ed_err = "ec_eddsa_verify_batch: only Ed25519 (the WEI25519 curve handle) is supported";
		return;
	}
	const Big &p = cv->p;
	const Big one(1, 1), two(1, 2), three(1, 3);
	const Big A(1, 486662);
	const Big A3 = big_mulmod(A, big_inv_p(three, p), p);
	// edwards25519: a = -1, d = -121665/121666; alpha_edwards^2 = -(A + 2) (B = 1 Montgomery model)
	const Big a_ed = big_sub(p, one);
	const Big d_ed = big_negmod(big_mulmod(Big(1, 121665), big_inv_p(Big(1, 121666), p), p), p);
	Big alpha;
	if (!big_sqrt_5mod8(big_negmod(big_add(A, two), p), p, &alpha)) {
		cv->ed_err = "ec_eddsa_verify_batch: internal: alpha";
		return;
	}
	{
		// the handle must be the Weierstrass model whose generator is the image of the Ed25519 base
		// point (y = 4/5, x even); this also fixes the sign of alpha_edwards
		const Big yb = big_mulmod(Big(1, 4), big_inv_p(Big(1, 5), p), p);
		const Big y2 = big_mulmod(yb, yb, p);
		const Big num = big_mod(big_add(one, big_sub(p, y2)), p);
		const Big den = big_mod(big_add(a_ed, big_sub(p, big_mulmod(d_ed, y2, p))), p);
		Big xb;
		if (!big_sqrt_5mod8(big_mulmod(num, big_inv_p(den, p), p), p, &xb)) {
			cv->ed_err = "ec_eddsa_verify_batch: internal: base point";
			return;
		}
		if (xb[0] & 1u) {
			xb = big_sub(p, xb);
		}
		const Big um = big_mulmod(big_mod(big_add(one, yb), p), big_inv_p(big_mod(big_add(one, big_sub(p, yb)), p), p), p);
		const Big X = big_mod(big_add(um, A3), p);
		Big vm = big_mulmod(big_mulmod(alpha, um, p), big_inv_p(xb, p), p);
		if (big_cmp(vm, cv->gy) != 0) {
			alpha = big_sub(p, alpha);
			vm = big_sub(p, vm);
		}
		if (big_cmp(X, cv->gx) != 0 || big_cmp(vm, cv->gy) != 0) {
			cv->ed_err = "ec_eddsa_verify_batch: the curve generator is not the image of the Ed25519 base point";
			return;
		}
		big_digits29(cv->ed_Bx, 9, xb);
		big_digits29(cv->ed_By, 9, yb);
	}
	cv->ed_cof_dbl = 0xffffffffu;
	{
		Big t = cv->q;
		for (uint32_t c = 0; c <= 4; c++) {
			if (big_cmp(t, cv->order) == 0) {
				cv->ed_cof_dbl = c;
				break;
			}
			t = big_add(t, t);
		}
	}
	if (cv->ed_cof_dbl == 0xffffffffu) {
		cv->ed_err = "ec_eddsa_verify_batch: unexpected cofactor";
		return;
	}
	const int nw = cv->nw;
	const Big R = big_mod(big_pow2(32 * nw), p);
	EcamdEdDecodeArgs &D = cv->ed_tmpl;
	memset(&D, 0, sizeof(D));
	D.len = 32;
	D.slot = cv->slot;
	big_store(D.a, nw, big_mulmod(a_ed, R, p));
	big_store(D.d, nw, big_mulmod(d_ed, R, p));
	big_store(D.sm1, nw, big_mulmod(big_sqrt_m1(p), R, p));
	big_store(D.alpha, nw, big_mulmod(alpha, R, p));
	big_store(D.A3, nw, big_mulmod(A3, R, p));
	big_digits29(D.g_d, 9, d_ed);
	big_digits29(D.g_sm1, 9, big_sqrt_m1(p));
	big_digits29(D.g_alpha, 9, alpha);
	big_digits29(D.g_A3, 9, A3);
	big_digits29(cv->ed_2d, 9, big_mod(big_add(d_ed, d_ed), p));
	cv->ed_state = 1;
}

// Round 4: the 16-bit comb table of the Ed25519 base point on the Edwards curve, T[j][m-1] = [m 2^(16 j)]B (m = 1..32768, j < 16)
// and [2^256]B, as precomputed entries (y - x, y + x, 2d x y), 128 bytes each (67 MB of the 288 GB).  The multiples come from this
// engine's own scalar multiplication on the Weierstrass model -- the batch maybe_build_comb uses -- and k_edcomb_build_c25519 maps
// them to the Edwards curve.  With it k_ed_tail_c25519 finishes a verification without leaving the Edwards curve.  ctx->mu held.
static void maybe_build_edcomb(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n)
{
	if (cv->d_edcomb || cv->edcomb_off || ctx->comb_min_batch == 0 || n < ctx->comb_min_batch || cv->gflavour != 2 || cv->gslot < 0) {
		return;
	}
	cv->edcomb_off = true;   // stays set if anything fails
	if (hipDeviceSynchronize() != hipSuccess) {   // the build borrows the context's scratch (see maybe_build_comb)
		return;
	}
	const uint32_t slen = 32, nwin = 16, ne = ECAMD_EDC_ENTRIES;
	std::vector<uint8_t> hs((size_t)ne * slen, 0);
	for (uint32_t j = 0; j < nwin; j++) {
		for (uint32_t m = 1; m <= 32768; m++) {
			uint8_t *e = &hs[((size_t)j * 32768 + (m - 1)) * slen];
			e[slen - 1 - 2 * j] = (uint8_t)(m & 0xff);
			e[slen - 2 - 2 * j] = (uint8_t)(m >> 8);
		}
	}
	big_to_be(&hs[(size_t)nwin * 32768 * slen], (int)slen, big_mod(big_pow2(256), cv->q));
	uint8_t *dsc = nullptr, *dpt = nullptr, *dst = nullptr;
	uint32_t *table = nullptr;
	std::vector<uint8_t> st(ne);
	hipStream_t s = ctx->stream;
	bool ok = hipMalloc((void **)&dsc, hs.size()) == hipSuccess && hipMalloc((void **)&dpt, (size_t)ne * 64) == hipSuccess &&
		  hipMalloc((void **)&dst, ne) == hipSuccess && hipMalloc((void **)&table, (size_t)ne * ECAMD_EDC_ENT_WORDS * 4) == hipSuccess &&
		  hipMemcpy(dsc, hs.data(), hs.size(), hipMemcpyHostToDevice) == hipSuccess;
	{
		const uint32_t user_chunk = ctx->max_chunk;
		ctx->max_chunk = user_chunk < (1u << 20) ? (1u << 20) : user_chunk;
		ok = ok && smul_dev_locked(ctx, cv, ne, dsc, slen, nullptr, dpt, dst, s) == 0;
		ctx->max_chunk = user_chunk;
	}
	if (ok) {
		EcamdEdTailConsts C;
		memcpy(C.g_2d, cv->ed_2d, sizeof(C.g_2d));
		memcpy(C.g_alpha, cv->ed_tmpl.g_alpha, sizeof(C.g_alpha));
		memcpy(C.g_A3, cv->ed_tmpl.g_A3, sizeof(C.g_A3));
		ok = ecamd_launch_edcomb_build_c25519(dpt, ne, table, C, cv->gslot, s) == hipSuccess &&
		     hipMemcpyAsync(st.data(), dst, ne, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
	}
	for (uint32_t i = 0; ok && i < ne; i++) {
		ok = (st[i] == 0);
	}
	(void)hipFree(dsc);
	(void)hipFree(dpt);
	(void)hipFree(dst);
	if (!ok) {
		(void)hipFree(table);
		(void)hipGetLastError();
		return;   // the Weierstrass tail keeps serving
	}
	cv->d_edcomb = table;
	cv->edcomb_off = false;
}

// device pointers in and out; only enqueues on s
static int eddsa_verify_dev_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig,
				   const uint8_t *d_hram, uint32_t hram_len, uint8_t *d_res, hipStream_t s)
{
	if (n > ctx->max_chunk) {  // bound the scratch: pieces of max_chunk items, in order on the stream
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return eddsa_verify_dev_locked(ctx, cv, m, d_pub + (size_t)off * 32, d_sig + (size_t)off * 64,
						       d_hram + (size_t)off * hram_len, hram_len, d_res + off, s);
		});
	}
	const size_t len = 32, plen = 64;
	const uint32_t cof_dbl = cv->ed_cof_dbl;
	if (stage_need(ctx, {{EV_A, n * plen}, {EV_R, n * plen}, {EV_FLAGSA, n}, {EV_FLAGSR, n}, {EV_FLAGSS, n}, {EV_S, n * len}, {EV_H, n * len},
			     {EV_HA, n * plen}, {EV_STHA, n}, {EV_SG, n * plen}, {EV_STSG, n}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	const int nw = cv->nw;
	EcamdEdDecodeArgs D = cv->ed_tmpl;
	D.n = n;
	D.encA = d_pub;
	D.strideA = (uint32_t)len;
	D.encR = d_sig;
	D.strideR = (uint32_t)plen;
	D.pointsA = S[EV_A];
	D.pointsR = S[EV_R];
	D.flagsA = S[EV_FLAGSA];
	D.flagsR = S[EV_FLAGSR];
	D.cof_dbl = cof_dbl;
	const bool unit25519 = cv->gflavour == 2 && cv->gslot >= 0;
	const bool edwards_hA = unit25519 && getenv("ECAMD_NO_EDWARDS_SMUL") == nullptr;
	D.edA = nullptr;
	if (edwards_hA) {
		// A on the Edwards curve, extended result records, window tables
		if (stage_need(ctx, EV_EDA, (size_t)n * 20 * 4) ||
		    stage_need(ctx, EV_REC, (size_t)n * ECAMD_EDR_REC_WORDS * 4) ||
		    stage_need(ctx, EV_TBL, (size_t)n * ECAMD_EDT_ITEM_WORDS * 4)) {
			return -1;
		}
		D.edA = (uint32_t *)S[EV_EDA];
	}
	// Edwards path: R's map to the Weierstrass model rides on the shared inversion of k_ed_hA_fin instead of costing the
	// decode kernel an inversion per item (EV_EDR: R on the Edwards curve)
	const bool late_map = edwards_hA && getenv("ECAMD_NO_ED_LATE_MAP") == nullptr;
	// round 4: the whole tail on the Edwards curve ([S]B from the Edwards comb table; no map, no inversion, no Weierstrass pass)
	bool ed_tail = false;
	if (late_map && getenv("ECAMD_NO_ED_TAIL") == nullptr) {
		maybe_build_edcomb(ctx, cv, n);
		ed_tail = cv->d_edcomb != nullptr;
	}
	// round 4, second step: half-length scalars (k_ed_lat) and one window loop over the tables of A and R (k_ed_smul2_c25519)
	const bool lattice = ed_tail && len == 32 && getenv("ECAMD_NO_ED_LATTICE") == nullptr;
	if (lattice && stage_need(ctx, EV_TBL, (size_t)n * 2 * ECAMD_EDT_ITEM_WORDS * 4)) {
		return -1;
	}
	// k_ed_lat (S < q, h mod q, the truncated Euclid: integer work with data-dependent trip counts, 0.43 VALU busy) beside the decode
	// kernel (two square-root chains, MAD bound) on the side stream: both read only the caller's arrays.  $ECAMD_NO_ED_LAT_BESIDE: in line.
	bool lat_beside = false;
	EcamdEdLatArgs L;   // EV_A (n x 64, free on this path): v and |u|, 12 words per item; EV_H: s' = u S mod q; EV_STHA: meta
	memset(&L, 0, sizeof(L));
	if (lattice) {
		L.sigs = d_sig;
		L.hram = d_hram;
		L.S_be = S[EV_S];
		L.sp_be = S[EV_H];
		L.uv = (uint32_t *)S[EV_A];
		L.meta = S[EV_STHA];
		L.flags = S[EV_FLAGSS];
		L.n = n;
		L.hlen = hram_len;
		L.qslot = cv->qslot;
		if (ctx->side_ok && getenv("ECAMD_NO_ED_LAT_BESIDE") == nullptr) {
			HIPCHK(hipEventRecord(ctx->side_fork, s));
			HIPCHK(hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0));
			HIPCHK(ecamd_launch_ed_lat(L, ctx->side_stream));
			HIPCHK(hipEventRecord(ctx->side_done, ctx->side_stream));
			lat_beside = true;
		}
	}
	if (late_map) {
		if (stage_need(ctx, EV_EDR, (size_t)n * 20 * 4)) {
			return -1;
		}
		D.edR = (uint32_t *)ctx->stage[EV_EDR];
		HIPCHK(ecamd_launch_ed_decode_ed_c25519(D, cv->gslot, s));
	} else if (unit25519) {
		HIPCHK(ecamd_launch_ed_decode_c25519(D, cv->gslot, s));  // the same decoding on the radix-2^29 field
	} else {
		HIPCHK(ecamd_launch_ed_decode(nw, D, s));
	}
	if (lattice) {
		if (lat_beside) {
			HIPCHK(hipStreamWaitEvent(s, ctx->side_done, 0));
		} else {
			HIPCHK(ecamd_launch_ed_lat(L, s));
		}
		EcamdEdSmul2Args E;
		memset(&E, 0, sizeof(E));
		E.edA = (const uint32_t *)S[EV_EDA];
		E.edR = (const uint32_t *)ctx->stage[EV_EDR];
		E.flagsA = S[EV_FLAGSA];
		E.flagsR = S[EV_FLAGSR];
		E.flagsS = S[EV_FLAGSS];
		E.uv = (const uint32_t *)S[EV_A];
		E.meta = S[EV_STHA];
		E.tbl = (uint32_t *)ctx->stage[EV_TBL];
		E.rec = (uint32_t *)S[EV_REC];
		E.n = n;
		memcpy(E.g_2d, cv->ed_2d, sizeof(E.g_2d));
		HIPCHK(ecamd_launch_ed_smul2_c25519(E, cv->gslot, s, ctx->timing ? ctx->ev_dom : nullptr));
		ctx->ev_dom_valid = ctx->ev_dom_valid || ctx->timing;
		EcamdEdTailArgs T;
		memset(&T, 0, sizeof(T));
		T.rec = (const uint32_t *)S[EV_REC];
		T.edR = (const uint32_t *)ctx->stage[EV_EDR];
		T.flagsA = S[EV_FLAGSA];
		T.flagsR = S[EV_FLAGSR];
		T.flagsS = S[EV_FLAGSS];
		T.S_be = S[EV_S];
		T.sp_be = S[EV_H];
		T.meta = S[EV_STHA];
		T.comb = cv->d_edcomb;
		T.result = d_res;
		T.n = n;
		T.cof_dbl = cof_dbl;
		memcpy(T.C.g_2d, cv->ed_2d, sizeof(T.C.g_2d));
		HIPCHK(ecamd_launch_ed_tail2_c25519(T, cv->gslot, s));
		return 0;
	}
	EcamdEdScalArgs C;
	memset(&C, 0, sizeof(C));
	C.sigs = d_sig;
	C.hram = d_hram;
	C.S_be = S[EV_S];
	C.h_be = S[EV_H];
	C.flags = S[EV_FLAGSS];
	C.n = n;
	C.len = (uint32_t)len;
	C.hlen = hram_len;
	C.qslot = cv->qslot;
	HIPCHK(ecamd_launch_ed_scal(nw, C, s));
	// [h]A, [S]G  ([8]A != infinity was checked by the decode kernel)
	if (edwards_hA) {
		// [h]A on the Edwards curve itself (complete extended-coordinate formulas), mapped to the Weierstrass model
		EcamdEdSmulArgs E;
		memset(&E, 0, sizeof(E));
		E.edA = (const uint32_t *)S[EV_EDA];
		E.scalars = S[EV_H];
		E.flags = S[EV_FLAGSA];
		E.tbl = (uint32_t *)S[EV_TBL];
		E.rec = (uint32_t *)S[EV_REC];
		E.out = S[EV_HA];
		E.status = S[EV_STHA];
		E.n = n;
		memcpy(E.g_2d, cv->ed_2d, sizeof(E.g_2d));
		memcpy(E.g_alpha, cv->ed_tmpl.g_alpha, sizeof(E.g_alpha));
		memcpy(E.g_A3, cv->ed_tmpl.g_A3, sizeof(E.g_A3));
		if (late_map) {
			E.edR = (const uint32_t *)ctx->stage[EV_EDR];
			E.flagsR = S[EV_FLAGSR];
			E.outR = S[EV_R];
		}
		if (ed_tail) {
			E.out = nullptr;   // no k_ed_hA_fin: [h]A stays in E.rec
		}
		HIPCHK(ecamd_launch_ed_smul_c25519(E, cv->gslot, s, ctx->timing ? ctx->ev_dom : nullptr));
		ctx->ev_dom_valid = ctx->ev_dom_valid || ctx->timing;
	}
	if (ed_tail) {
		EcamdEdTailArgs T;
		memset(&T, 0, sizeof(T));
		T.rec = (const uint32_t *)S[EV_REC];
		T.edR = (const uint32_t *)ctx->stage[EV_EDR];
		T.flagsA = S[EV_FLAGSA];
		T.flagsR = S[EV_FLAGSR];
		T.flagsS = S[EV_FLAGSS];
		T.S_be = S[EV_S];
		T.comb = cv->d_edcomb;
		T.result = d_res;
		T.n = n;
		T.cof_dbl = cof_dbl;
		memcpy(T.C.g_2d, cv->ed_2d, sizeof(T.C.g_2d));
		HIPCHK(ecamd_launch_ed_tail_c25519(T, cv->gslot, s));
		return 0;
	}
	{
		PublicScalars pub_scope(ctx);   // h and S of a signature are public
		if ((!edwards_hA && smul_dev_locked(ctx, cv, n, S[EV_H], (uint32_t)len, S[EV_A], S[EV_HA], S[EV_STHA], s)) ||
		    smul_dev_locked(ctx, cv, n, S[EV_S], (uint32_t)len, nullptr, S[EV_SG], S[EV_STSG], s)) {
			return -1;
		}
	}
	EcamdEdFinArgs F;
	memset(&F, 0, sizeof(F));
	F.SG = S[EV_SG];
	F.stSG = S[EV_STSG];
	F.hA = S[EV_HA];
	F.sthA = S[EV_STHA];
	F.R = S[EV_R];
	F.flagsA = S[EV_FLAGSA];
	F.flagsR = S[EV_FLAGSR];
	F.flagsS = S[EV_FLAGSS];
	F.result = d_res;
	F.n = n;
	F.clen = (uint32_t)len;
	F.cof_dbl = cof_dbl;
	F.slot = cv->slot;
	if (cv->gflavour == 2 && cv->gslot >= 0 && getenv("ECAMD_NO_ED_FIN_G") == nullptr) {
		HIPCHK(ecamd_launch_ed_fin_g29(2, cv->gslot, F, s));   // the same tail on the 2^255 - 19 unit (k_ed_fin_g)
	} else {
		HIPCHK(ecamd_launch_ed_fin(nw, F, s));
	}
	return 0;
}

// ---- Ed448 (EDDSA448 branches of sig/eddsa.c) on the WEI448 handle ----
static Big big_div4(const Big &x)
{
	Big q(x.size(), 0);
	for (size_t i = 0; i < x.size(); i++) {
		q[i] = (x[i] >> 2) | ((i + 1 < x.size()) ? (x[i + 1] << 30) : 0u);
	}
	big_trim(q);
	return q;
}

static void ed448_setup(ecamd_curve *cv)
{
	cv->ed448_state = -1;
	const Big p448 = big_sub(big_sub(big_pow2(448), big_pow2(224)), Big(1, 1));
	if (!(cv->pbits == 448 && cv->clen == 56 && cv->nw == 14 && cv->qslot >= 0 && cv->qnw == 14 && cv->qlen == 56 &&
	      big_cmp(cv->p, p448) == 0)) {
		cv->ed448_err = "ec_eddsa_verify_batch: Ed448 needs the WEI448 curve handle";
		return;
	}
	const Big &p = cv->p;
	const Big one(1, 1), two(1, 2), three(1, 3);
	const Big A(1, 156326);
	const Big A3 = big_mulmod(A, big_inv_p(three, p), p);
	const Big d448 = big_sub(p, Big(1, 39081));
	const Big e4 = big_div4(big_add(p, one));                    // (p + 1) / 4: square roots for p = 3 mod 4
	Big alpha = big_powmod(Big(1, 156324), e4, p);               // alpha^2 = A - 2
	if (big_cmp(big_mulmod(alpha, alpha, p), Big(1, 156324)) != 0) {
		cv->ed448_err = "ec_eddsa_verify_batch: internal: alpha";
		return;
	}
	const Big diso = big_mulmod(Big(1, 156328), big_inv_p(Big(1, 156324), p), p);
	{
		// the Ed448 base point (RFC 8032) must map to the generator of the handle; this fixes the sign of alpha
		static const uint8_t yb_le[56] = {
			0x14, 0xfa, 0x30, 0xf2, 0x5b, 0x79, 0x08, 0x98, 0xad, 0xc8, 0xd7, 0x4e, 0x2c, 0x13, 0xbd, 0xfd, 0xc4, 0x39, 0x7c,
			0xe6, 0x1c, 0xff, 0xd3, 0x3a, 0xd7, 0xc2, 0xa0, 0x05, 0x1e, 0x9c, 0x78, 0x87, 0x40, 0x98, 0xa3, 0x6c, 0x73, 0x73,
			0xea, 0x4b, 0x62, 0xc7, 0xc9, 0x56, 0x37, 0x20, 0x76, 0x88, 0x24, 0xbc, 0xb6, 0x6e, 0x71, 0x46, 0x3f, 0x69};
		uint8_t yb_be[56];
		for (int i = 0; i < 56; i++) {
			yb_be[i] = yb_le[55 - i];
		}
		const Big y = big_from_be(yb_be, 56);
		const Big yy = big_mulmod(y, y, p);
		auto sub = [&](const Big &a, const Big &b) { return big_mod(big_add(a, big_sub(p, big_mod(b, p))), p); };
		const Big t = big_mulmod(sub(one, yy), big_inv_p(sub(one, big_mulmod(d448, yy, p)), p), p);
		Big x = big_powmod(t, e4, p);
		if (big_cmp(big_mulmod(x, x, p), t) != 0) {
			cv->ed448_err = "ec_eddsa_verify_batch: internal: base point";
			return;
		}
		if (x[0] & 1u) {
			x = big_sub(p, x);                                   // the encoding's sign bit is 0
		}
		const Big xx = big_mulmod(x, x, p);
		const Big X = big_mulmod(big_mulmod(alpha, big_mulmod(x, y, p), p), big_inv_p(sub(sub(two, xx), yy), p), p);
		const Big Y = big_mulmod(big_mod(big_add(xx, yy), p), big_inv_p(sub(yy, xx), p), p);
		const Big u = big_mulmod(big_mod(big_add(one, Y), p), big_inv_p(sub(one, Y), p), p);
		Big v = big_mulmod(big_mulmod(alpha, u, p), big_inv_p(X, p), p);
		const Big Xw = sub(A3, u);
		Big Yw = sub(Big(1, 0), v);
		if (big_cmp(Yw, cv->gy) != 0) {
			alpha = big_sub(p, alpha);
			Yw = sub(Big(1, 0), Yw);
		}
		if (big_cmp(Xw, cv->gx) != 0 || big_cmp(Yw, cv->gy) != 0) {
			cv->ed448_err = "ec_eddsa_verify_batch: the curve generator is not the image of the Ed448 base point";
			return;
		}
	}
	{
		Big t = big_add(cv->q, cv->q);
		t = big_add(t, t);
		if (big_cmp(t, cv->order) != 0) {
			cv->ed448_err = "ec_eddsa_verify_batch: unexpected cofactor";
			return;
		}
	}
	Big c4;
	for (uint32_t j = 1; j <= 3; j++) {
		Big jq = big_add(big_mul(cv->q, Big(1, j)), one);
		if ((jq[0] & 3u) == 0) {
			c4 = big_div4(jq);
			break;
		}
	}
	big_to_be(cv->ed448_c4, 56, c4);
	const int nw = cv->nw;
	const Big R = big_mod(big_pow2(32 * nw), p);
	EcamdEd448DecodeArgs &D = cv->ed448_tmpl;
	memset(&D, 0, sizeof(D));
	D.slot = cv->slot;
	big_store(D.d448, nw, big_mulmod(d448, R, p));
	big_store(D.diso, nw, big_mulmod(diso, R, p));
	big_store(D.alpha, nw, big_mulmod(alpha, R, p));
	big_store(D.A3, nw, big_mulmod(A3, R, p));
	big_digits29(D.g_d448, 16, d448, 28);     // the Goldilocks unit's 28-bit limbs
	big_digits29(D.g_diso, 16, diso, 28);
	big_digits29(D.g_alpha, 16, alpha, 28);
	big_digits29(D.g_A3, 16, A3, 28);
	cv->ed448_state = 1;
}

// device pointers in and out; pubs n x 57, sigs n x 114, hram n x 114
static int eddsa448_verify_dev_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig,
				      const uint8_t *d_hram, uint8_t *d_res, hipStream_t s)
{
	if (n > ctx->max_chunk) {  // bound the scratch: pieces of max_chunk items, in order on the stream
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return eddsa448_verify_dev_locked(ctx, cv, m, d_pub + (size_t)off * 57, d_sig + (size_t)off * 114,
							  d_hram + (size_t)off * 114, d_res + off, s);
		});
	}
	const size_t len = 56, plen = 112;
	// EV_H holds k = 4h 4^-1 mod 4q, EV_HA / EV_STHA [k]A and its status
	if (stage_need(ctx, {{EV_A, n * plen}, {EV_R, n * plen}, {EV_FLAGSA, n}, {EV_FLAGSR, n}, {EV_FLAGSS, n}, {EV_S, n * len}, {EV_H, n * len},
			     {EV_HA, n * plen}, {EV_STHA, n}, {EV_SG, n * plen}, {EV_STSG, n}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	EcamdEd448DecodeArgs D = cv->ed448_tmpl;
	D.n = n;
	D.encA = d_pub;
	D.strideA = 57;
	D.encR = d_sig;
	D.strideR = 114;
	D.pointsA = S[EV_A];
	D.pointsR = S[EV_R];
	D.flagsA = S[EV_FLAGSA];
	D.flagsR = S[EV_FLAGSR];
	if (cv->gflavour == 5 && cv->gslot >= 0 && getenv("ECAMD_NO_G448_DECODE") == nullptr) {
		HIPCHK(ecamd_launch_ed448_decode_g(D, cv->gslot, s));   // the same decoding on the Goldilocks radix-2^29 field
	} else {
		HIPCHK(ecamd_launch_ed448_decode(D, s));
	}
	EcamdEdScalArgs C;
	memset(&C, 0, sizeof(C));
	C.sigs = d_sig;
	C.hram = d_hram;
	C.S_be = S[EV_S];
	C.h_be = S[EV_H];
	C.flags = S[EV_FLAGSS];
	C.n = n;
	C.len = 57;
	C.hlen = 114;
	C.qslot = cv->qslot;
	C.c4_mod4 = cv->ed448_c4[55] & 3u;
	HIPCHK(ecamd_launch_ed448_scal(C, s));
	// the reference's [4h mod q]([4^-1 mod q]A) as one multiplication of A (k_ed448_scal), and [S]G
	{
		PublicScalars pub_scope(ctx);   // h and S of a signature are public
		if (smul_dev_locked(ctx, cv, n, S[EV_H], (uint32_t)len, S[EV_A], S[EV_HA], S[EV_STHA], s) ||
		    smul_dev_locked(ctx, cv, n, S[EV_S], (uint32_t)len, nullptr, S[EV_SG], S[EV_STSG], s)) {
			return -1;
		}
	}
	EcamdEdFinArgs F;
	memset(&F, 0, sizeof(F));
	F.SG = S[EV_SG];
	F.stSG = S[EV_STSG];
	F.hA = S[EV_HA];
	F.sthA = S[EV_STHA];
	F.R = S[EV_R];
	F.flagsA = S[EV_FLAGSA];
	F.flagsR = S[EV_FLAGSR];
	F.flagsS = S[EV_FLAGSS];
	F.result = d_res;
	F.n = n;
	F.clen = (uint32_t)len;
	F.cof_dbl = 2;
	F.Akey = S[EV_A];      // [4]A = infinity <=> the stored key [4^-1 mod q]A has small order
	F.stA = nullptr;
	F.slot = cv->slot;
	if (cv->gflavour == 5 && cv->gslot >= 0 && getenv("ECAMD_NO_ED_FIN_G") == nullptr) {
		HIPCHK(ecamd_launch_ed_fin_g29(5, cv->gslot, F, s));   // the same tail on the Goldilocks unit (k_ed_fin_g)
	} else {
		HIPCHK(ecamd_launch_ed_fin(cv->nw, F, s));
	}
	return 0;
}

// ------------------------------------------------------------------------------------------
// Round 6: Ed448 whole-batch verification (SURVEY.md 8 row f4 for EDDSA448 / EDDSA448PH; _eddsa_verify_batch, sig/eddsa.c:2580-2860, serves both
// EdDSA curves).  The reference's combination  sum [cof z_i]R_i + sum [z_i 4 h_i][cof]A'_i + [-sum z_i S_i][cof]G = infinity  on the Weierstrass
// model is, on the prime-order components, the Schnorr-type equation  [sum z_i S_i]G + sum [z_i (q - h_i)]A_i - sum [z_i]R_i  of
// schnorr_msm_dev_locked with its final test cofactored: the decoding of eddsa448_verify_dev_locked (A_i, R_i as affine points of WEI448), S_i
// and (q - h_i) mod q from k_ed448_scal, the reference's per-item rejections as one gate word (k_ed_msm_gate), then the multi-scalar
// multiplication on the Goldilocks unit -- by buckets from 2^17 items on, the Straus loop below -- ending in [4](sum + [c]G) = infinity.
// Soundness as for the item form: [4] kills every torsion component, so scalars taken mod q and the decoded (not the stored [4^-1]A) key are
// exact; a batch with an item that fails its cofactored equation passes with probability ~2^-128.  d_verdict[0] is SET to 1 for "not
// decided here" and never cleared (the pieces of one call share it).  Only enqueues.
// ------------------------------------------------------------------------------------------
static bool eddsa448_msm_available(const ecamd_curve *cv)
{
	int pb, fl, sl;
	return cv->pbits == 448 && cv->ed448_state == 1 && cv->nw == 14 && cv->cofactor == 4 && cv->qslot >= 0 && cv->qbits >= 160 &&
	       schnorr_msm_unit(cv, &pb, &fl, &sl);
}

static int eddsa448_msm_dev_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig, const uint8_t *d_hram,
				   const uint8_t seed[32], uint32_t piece, uint8_t *d_verdict, hipStream_t s)
{
	if (n == 0 || n > ctx->max_chunk) {
		return fail("internal: eddsa448_msm_dev_locked serves one piece of at most max_chunk items");
	}
	const size_t len = 56, plen = 112;
	// (EV_H: k, unused here)
	if (stage_need(ctx, {{EV_A, n * plen}, {EV_R, n * plen}, {EV_FLAGSA, n}, {EV_FLAGSR, n}, {EV_FLAGSS, n}, {EV_S, n * len}, {EV_H, n * len},
			     {EV_NE, n * len}, {EV_GATE, 256}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	EcamdEd448DecodeArgs D = cv->ed448_tmpl;
	D.n = n;
	D.encA = d_pub;
	D.strideA = 57;
	D.encR = d_sig;
	D.strideR = 114;
	D.pointsA = S[EV_A];
	D.pointsR = S[EV_R];
	D.flagsA = S[EV_FLAGSA];
	D.flagsR = S[EV_FLAGSR];
	if (cv->gflavour == 5 && cv->gslot >= 0 && getenv("ECAMD_NO_G448_DECODE") == nullptr) {
		HIPCHK(ecamd_launch_ed448_decode_g(D, cv->gslot, s));
	} else {
		HIPCHK(ecamd_launch_ed448_decode(D, s));
	}
	EcamdEdScalArgs C;
	memset(&C, 0, sizeof(C));
	C.sigs = d_sig;
	C.hram = d_hram;
	C.S_be = S[EV_S];
	C.h_be = S[EV_H];
	C.ne_be = S[EV_NE];
	C.flags = S[EV_FLAGSS];
	C.n = n;
	C.len = 57;
	C.hlen = 114;
	C.qslot = cv->qslot;
	C.c4_mod4 = cv->ed448_c4[55] & 3u;
	HIPCHK(ecamd_launch_ed448_scal(C, s));
	uint32_t *d_gate = (uint32_t *)S[EV_GATE];
	uint8_t *d_piece = S[EV_GATE] + 16;
	HIPCHK(hipMemsetAsync(S[EV_GATE], 0, 16, s));
	HIPCHK(hipMemsetAsync(d_piece, 1, 1, s));
	// (the keys of small order, [4]A = infinity: seen by the combination's own import of the keys on the fast unit -- cof_dbl of EcamdMsmArgs)
	HIPCHK(ecamd_launch_ed_msm_gate(cv->nw, S[EV_A], S[EV_FLAGSA], S[EV_FLAGSR], S[EV_FLAGSS], n, (uint32_t)len, 0, cv->slot, d_gate, s));
	{
		PublicScalars pub_scope(ctx);   // everything a verification multiplies by is public
		if (schnorr_msm_dev_locked(ctx, cv, n, S[EV_S], S[EV_NE], S[EV_A], S[EV_R], 0, seed, piece, d_piece, nullptr, nullptr, s, 2)) {
			return -1;
		}
	}
	HIPCHK(ecamd_launch_verdict_or(d_verdict, d_piece, d_gate, s));
	return 0;
}

// host arrays -> one verdict: pieces of max_chunk items, each with its own combination.  *accept = 1 when every piece accepts.
static int eddsa448_msm_host_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs, const uint8_t *hram,
				    int *accept)
{
	uint8_t seed[32];
	if (msm_seed(ctx, seed)) {
		return -1;
	}
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	if (stage_need(ctx, MH_PUB, (size_t)chunk * 57) || stage_need(ctx, MH_SIG, (size_t)chunk * 114) ||
	    stage_need(ctx, MH_HRAM, (size_t)chunk * 114) || stage_need(ctx, MH_VERDICT448, 256)) {
		return -1;
	}
	uint8_t *d_verdict = ctx->stage[MH_VERDICT448];
	HIPCHK(hipMemsetAsync(d_verdict, 0, 1, s));
	for (uint32_t off = 0, pc = 0; off < n; off += chunk, pc++) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		HIPCHK(hipMemcpyAsync(ctx->stage[MH_PUB], pubkeys + (size_t)off * 57, (size_t)m * 57, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(ctx->stage[MH_SIG], sigs + (size_t)off * 114, (size_t)m * 114, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(ctx->stage[MH_HRAM], hram + (size_t)off * 114, (size_t)m * 114, hipMemcpyHostToDevice, s));
		if (eddsa448_msm_dev_locked(ctx, cv, m, ctx->stage[MH_PUB], ctx->stage[MH_SIG], ctx->stage[MH_HRAM], seed, pc, d_verdict, s)) {
			(void)hipStreamSynchronize(s);
			return -1;
		}
	}
	uint8_t v = 1;
	HIPCHK(hipMemcpyAsync(&v, d_verdict, 1, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	memset(seed, 0, sizeof(seed));
	*accept = v == 0;
	return 0;
}

static int eddsa_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const void *a, const void *b,
			 const void *c, const void *d, uint32_t hram_len)
{
	if (!ctx || !cv_in || cv_in->ctx != ctx || (n && (!a || !b || !c || !d))) {
		return fail(std::string(fn) + ": bad argument");
	}
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	if (cv->pbits == 448) {
		if (cv->ed448_state == 0) {
			ed448_setup(cv);
		}
		if (cv->ed448_state < 0) {
			return fail(cv->ed448_err);
		}
		if (hram_len != 114) {
			return fail(std::string(fn) + ": Ed448 hashes with SHAKE256 (114 bytes): hram_len must be 114");
		}
		return 0;
	}
	if (cv->ed_state == 0) {
		ed_setup(cv);
	}
	if (cv->ed_state < 0) {
		return fail(cv->ed_err);
	}
	if (hram_len != 64) {
		return fail(std::string(fn) + ": Ed25519 hashes with SHA-512: hram_len must be 64");
	}
	return 0;
}

extern "C" int ec_eddsa_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const void *d_pubkeys,
					 const void *d_sigs, const void *d_hram, uint32_t hram_len, void *d_result,
					 void *hip_stream)
{
	if (!ctx) {
		return fail("ec_eddsa_verify_batch_dev: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	if (eddsa_args_ok("ec_eddsa_verify_batch_dev", ctx, cv_in, n, d_pubkeys, d_sigs, d_hram, d_result, hram_len)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
	StreamScope scope(ctx, s);
	if (cv_in->pbits == 448) {
		return eddsa448_verify_dev_locked(ctx, const_cast<ecamd_curve *>(cv_in), n, (const uint8_t *)d_pubkeys,
						  (const uint8_t *)d_sigs, (const uint8_t *)d_hram, (uint8_t *)d_result, s);
	}
	return eddsa_verify_dev_locked(ctx, const_cast<ecamd_curve *>(cv_in), n, (const uint8_t *)d_pubkeys,
				       (const uint8_t *)d_sigs, (const uint8_t *)d_hram, hram_len, (uint8_t *)d_result, s);
}

extern "C" int ec_eddsa_verify_batch(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const uint8_t *pubkeys,
				     const uint8_t *sigs, const uint8_t *hram, uint32_t hram_len, uint8_t *result)
{
	if (!ctx) {
		return fail("ec_eddsa_verify_batch: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	if (eddsa_args_ok("ec_eddsa_verify_batch", ctx, cv_in, n, pubkeys, sigs, hram, result, hram_len)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	const bool e448 = cv->pbits == 448;
	const std::vector<HostArr> arrs = {{pubkeys, nullptr, e448 ? 57u : 32u}, {sigs, nullptr, e448 ? 114u : 64u},
					   {hram, nullptr, hram_len}, {nullptr, result, 1}};
	return host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return e448 ? eddsa448_verify_dev_locked(ctx, cv, m, ip[0], ip[1], ip[2], op[3], s)
			    : eddsa_verify_dev_locked(ctx, cv, m, ip[0], ip[1], ip[2], hram_len, op[3], s);
	});
}

// Ed25519 verification with the hash INPUTS instead of the hashes: slot i (stride bytes: u32 length, then the bytes) holds
// dom2 || R || A || PH(M) as the verifier would feed them to SHA-512 (sig/eddsa.c:1995-2045, :2180-2200); hram is computed on the device.
extern "C" int ec_eddsa_verify_msg_batch(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
					 const uint8_t *hash_slots, uint32_t stride, uint8_t *result)
{
	if (!ctx || stride < 4 || (stride & 3u) || stride > 4096) {
		return fail("ec_eddsa_verify_msg_batch: bad argument (stride: a multiple of 4 in 4 .. 4096)");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	if (eddsa_args_ok("ec_eddsa_verify_msg_batch", ctx, cv_in, n, pubkeys, sigs, hash_slots, result, 64)) {
		return -1;
	}
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	if (cv->pbits != 255) {
		return fail("ec_eddsa_verify_msg_batch: Ed25519 (the WEI25519 handle) only: Ed448 hashes with SHAKE256");
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	const std::vector<HostArr> arrs = {{pubkeys, nullptr, 32u}, {sigs, nullptr, 64u}, {hash_slots, nullptr, stride}, {nullptr, result, 1}};
	return host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		if (ecdsa_hash_stage(ctx, 4, m, ip[2], stride, 64, s)) {
			return -1;
		}
		return eddsa_verify_dev_locked(ctx, cv, m, ip[0], ip[1], ctx->stage[ST_DIGESTS], 64, op[3], s);
	});
}

static int eddsa_sign_setup(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const void *a, const void *b,
			    const void *c, EcamdEdSignArgs *T)
{
	if (!ctx || !cv_in || cv_in->ctx != ctx || (n && (!a || !b || !c))) {
		return fail(std::string(fn) + ": bad argument");
	}
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	memset(T, 0, sizeof(*T));
	if (cv->pbits == 448) {
		if (cv->ed448_state == 0) {
			ed448_setup(cv);
		}
		if (cv->ed448_state < 0) {
			return fail(std::string(fn) + ": Ed448 signing needs the WEI448 curve handle");
		}
		memcpy(T->alpha, cv->ed448_tmpl.alpha, sizeof(T->alpha));
		memcpy(T->A3, cv->ed448_tmpl.A3, sizeof(T->A3));
		big_store(T->c4, 17, big_from_be(cv->ed448_c4, 56));
		T->is448 = 1;
	} else {
		if (cv->ed_state == 0) {
			ed_setup(cv);
		}
		if (cv->ed_state < 0) {
			return fail(std::string(fn) + ": EdDSA signing needs the WEI25519 or the WEI448 curve handle");
		}
		memcpy(T->alpha, cv->ed_tmpl.alpha, sizeof(T->alpha));
		memcpy(T->A3, cv->ed_tmpl.A3, sizeof(T->A3));
	}
	T->slot = cv->slot;
	T->qslot = cv->qslot;
	return 0;
}
// The same from the PROJECTIVE key an ec_pub_key holds (X || Y || Z on WEI25519): what a verifier that starts from libecc structures
// needs -- the reference hashes the key's Ed25519 ENCODING (eddsa_export_pub_key, sig/eddsa.c:795: Weierstrass -> Edwards -> octets), which
// ec_eddsa_encode_point_batch computes; here that encoding goes straight into the item's hash input on the device (bytes a_offset ..
// a_offset + 32 of the slot's message, which the caller leaves blank; the caller's array itself is not written), so one call replaces encode / copy back / build the inputs /
// verify.  A key that does not import (coordinates >= p, not on the curve) or is the point at infinity rejects its item.
// the encode step of EcamdEdSignArgs (Rw, stR -> out, status): on the 2^255 - 19 unit when the handle has it (k_ed_enc_c25519; round 6), else the
// saturated-word kernel ($ECAMD_NO_ED_ENC_G: always the latter)
static hipError_t launch_ed_sign_enc(const ecamd_curve *cv, const EcamdEdSignArgs &A, hipStream_t s)
{
	if (!A.is448 && cv->pbits == 255 && cv->ed_state == 1 && cv->gflavour == 2 && cv->gslot >= 0 && getenv("ECAMD_NO_ED_ENC_G") == nullptr) {
		EcamdEdTailConsts C;
		memcpy(C.g_2d, cv->ed_2d, sizeof(C.g_2d));
		memcpy(C.g_alpha, cv->ed_tmpl.g_alpha, sizeof(C.g_alpha));
		memcpy(C.g_A3, cv->ed_tmpl.g_A3, sizeof(C.g_A3));
		return ecamd_launch_ed_enc_c25519(A.Rw, A.stR, A.out, A.status, A.n, C, cv->gslot, s);
	}
	return ecamd_launch_ed_sign_enc(A, s);
}
struct EdBktRun {
	EcamdEdMsmArgs A;
	EcamdEdBktArgs B;
	EcamdEdMsmScalArgs C;
	EcamdEdMsmLaneArgs N;
	uint32_t *flagword;
	uint32_t n;
};
// ------------------------------------------------------------------------------------------
// Ed25519 whole-batch verification as one multi-scalar multiplication (the equation of _eddsa_verify_batch_no_memory,
// sig/eddsa.c:2278-2545, on the Edwards curve; kernels k_edmsm_* of ecamd_g29_kernel.hip / ecamd_kernels.hip).
// verdict byte: 0 = the combination vanishes and no item was rejected beforehand, 1 otherwise.  Only enqueues.
// ------------------------------------------------------------------------------------------
static bool eddsa_msm_available(const ecamd_curve *cv)
{
	return cv->pbits == 255 && cv->ed_state == 1 && cv->gflavour == 2 && cv->gslot >= 0;
}

static uint32_t eddsa_msm_pick_k(const ecamd_ctx *ctx, uint32_t n)
{
	if (ctx->msm_k) {
		return ctx->msm_k;
	}
	// one wave per SIMD needs 65536 lanes; two or more hide the table look-ups better
	uint32_t k = n >> 16;   // measured: 2^17 -> 2, 2^18 -> 4, 2^19 and up -> 8 (profiles/r2l_eddsa_msm.json)
	if (k < 1) {
		k = 1;
	}
	return k > 8 ? 8 : k;
}

// Round 6: the Ed25519 combination by buckets (k_edbkt_*; the Schnorr-type form: schnorr_msm_dev_locked) from 2^18 items on --
// $ECAMD_ED_MSM_ALGO=straus|bucket overrides the size rule.  The base point's term [q - sum z_i S_i]B enters as one copy of B per 64
// items with that group's share of the scalar: no global sum, no separate multiplication.
// scratch and kernel arguments of one combination over n items (ctx->msm; the flag word cleared)
static int eddsa_bkt_setup(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig, const uint8_t *d_hram,
			   const uint8_t seed[32], uint32_t piece, uint8_t *d_z_dump, EdBktRun &R, hipStream_t s)
{
	const uint32_t LB = (n + 63) / 64;
	const size_t counters = (size_t)16 << 16, recw = ECAMD_EDM_REC_WORDS;
	const uint32_t cap = 32u + 2u * (uint32_t)(((size_t)2 * n + LB + 65535) >> 16);
	// window 15: z_i h_i mod q < q = 2^252 + ..., so its digits take 4 097 values only and the n + LB scalars of that window crowd into as many buckets
	const uint32_t cap_top = 32u + 2u * (uint32_t)(((size_t)n + LB + 4096) / 4097);
	const size_t red_words = 2 * (2 * (size_t)16 * (65536 / ecamd_bkt_fold()) * recw + 18 * recw);   // (k_edbkt_reduce: two halves, T and U of the first level)
	size_t off = 0;
	auto carve = [&](size_t bytes) {
		const size_t o = off;
		off += msm_align(bytes);
		return o;
	};
	const size_t o_pts = carve(((size_t)2 * n + LB) * ECAMD_EDB_PT_STRIDE * 4);
	const size_t o_cA = carve((size_t)n * 32), o_zR = carve((size_t)n * 20), o_zs = carve((size_t)n * 32);
	const size_t o_rawC = carve((size_t)n * 32), o_rawZ = carve((size_t)n * 16), o_rawB = carve((size_t)LB * 32), o_sB = carve((size_t)LB * 32);
	const size_t o_flags = carve(n), o_flagsS = carve(n);
	const size_t o_cnt = carve(2 * counters * 4), o_ord = carve(((size_t)15 << 16) * cap * 4 + ((size_t)1 << 16) * cap_top * 4);
	const size_t o_bsum = carve(counters * recw * 4), o_red = carve(red_words * 4);
	const size_t o_word = carve(4);
	if (ensure(&ctx->msm, &ctx->msm_bytes, off)) {
		return -1;
	}
	uint8_t *M = ctx->msm;
	HIPCHK(hipMemsetAsync(M + o_word, 0, 4, s));
	R.n = n;
	R.flagword = (uint32_t *)(M + o_word);
	EcamdEdMsmArgs &A = R.A;
	memset(&A, 0, sizeof(A));
	A.encA = d_pub;
	A.strideA = 32;
	A.encR = d_sig;
	A.strideR = 64;
	A.flags = M + o_flags;
	A.n = n;
	A.cof_dbl = cv->ed_cof_dbl;
	memcpy(A.g_d, cv->ed_tmpl.g_d, sizeof(A.g_d));
	memcpy(A.g_sm1, cv->ed_tmpl.g_sm1, sizeof(A.g_sm1));
	memcpy(A.g_2d, cv->ed_2d, sizeof(A.g_2d));
	memcpy(A.g_Bx, cv->ed_Bx, sizeof(A.g_Bx));
	memcpy(A.g_By, cv->ed_By, sizeof(A.g_By));
	EcamdEdBktArgs &B = R.B;
	memset(&B, 0, sizeof(B));
	B.rawC = (const uint32_t *)(M + o_rawC);
	B.rawB = (const uint32_t *)(M + o_rawB);
	B.rawZ = (const uint32_t *)(M + o_rawZ);
	B.pts = (uint32_t *)(M + o_pts);
	B.count = (uint32_t *)(M + o_cnt);
	B.perm = B.count + counters;
	B.order = (uint32_t *)(M + o_ord);
	B.bsum = (uint32_t *)(M + o_bsum);
	B.red = (uint32_t *)(M + o_red);
	B.red_words = red_words;
	B.flagword = R.flagword;
	B.n = n;
	B.LB = LB;
	B.cap = cap;
	B.cap_top = cap_top;
	EcamdEdMsmScalArgs &C = R.C;
	memset(&C, 0, sizeof(C));
	C.sigs = d_sig;
	C.hram = d_hram;
	C.cA = (uint32_t *)(M + o_cA);
	C.zR = (uint32_t *)(M + o_zR);
	C.zs = (uint32_t *)(M + o_zs);
	C.rawC = (uint32_t *)(M + o_rawC);
	C.rawZ = (uint32_t *)(M + o_rawZ);
	C.flagsS = M + o_flagsS;
	C.z_dump = d_z_dump;
	memcpy(C.seed, seed, 32);
	C.nonce[0] = piece;
	C.n = n;
	C.qslot = cv->qslot;
	EcamdEdMsmLaneArgs &N = R.N;
	memset(&N, 0, sizeof(N));
	N.zs = (const uint32_t *)(M + o_zs);
	N.flags = M + o_flags;
	N.flagsS = M + o_flagsS;
	N.sB = (uint32_t *)(M + o_sB);
	N.rawB = (uint32_t *)(M + o_rawB);
	N.flagword = R.flagword;
	N.n = n;
	N.K = 64;
	N.L = LB;
	N.qslot = cv->qslot;
	return 0;
}
// the buckets summed, reduced and compared (everything is filed)
static int eddsa_bkt_tail(ecamd_ctx *ctx, ecamd_curve *cv, EdBktRun &R, uint8_t *d_verdict, uint32_t *d_sum_dump, hipStream_t s)
{
	if (ctx->timing) {
		HIPCHK(hipEventRecord(ctx->ev_dom[0], s));   // the dominant kernel: k_edbkt_accum, both launches (ecamd_ctx_dominant_kernel_ms)
	}
	if (ctx->side_ok && getenv("ECAMD_NO_EDBKT_SPLIT") == nullptr) {
		// the key-only windows (8 .. 15: z_i has 128 bits) first; their reduction and their doubling chains -- 16 w doublings in one lane, the long
		// ones -- on the side stream (idle by now) while the windows that hold the commitments too are summed (the Schnorr-type form does the same)
		HIPCHK(ecamd_launch_edbkt(R.A, R.B, 10, nullptr, nullptr, nullptr, cv->gslot, s));
		HIPCHK(hipEventRecord(ctx->side_hi, s));
		HIPCHK(hipStreamWaitEvent(ctx->side_stream, ctx->side_hi, 0));
		HIPCHK(ecamd_launch_edbkt(R.A, R.B, 12, nullptr, nullptr, nullptr, cv->gslot, ctx->side_stream));
		HIPCHK(hipEventRecord(ctx->side_red, ctx->side_stream));
		HIPCHK(ecamd_launch_edbkt(R.A, R.B, 11, nullptr, nullptr, nullptr, cv->gslot, s));
		if (ctx->timing) {
			HIPCHK(hipEventRecord(ctx->ev_dom[1], s));
			ctx->ev_dom_valid = true;
		}
		HIPCHK(ecamd_launch_edbkt(R.A, R.B, 13, nullptr, nullptr, nullptr, cv->gslot, s));
		HIPCHK(hipStreamWaitEvent(s, ctx->side_red, 0));
		HIPCHK(ecamd_launch_edbkt(R.A, R.B, 14, R.flagword, d_verdict, d_sum_dump, cv->gslot, s));
		return 0;
	}
	HIPCHK(ecamd_launch_edbkt(R.A, R.B, 1, nullptr, nullptr, nullptr, cv->gslot, s));
	if (ctx->timing) {
		HIPCHK(hipEventRecord(ctx->ev_dom[1], s));
		ctx->ev_dom_valid = true;
	}
	HIPCHK(ecamd_launch_edbkt(R.A, R.B, 2, R.flagword, d_verdict, d_sum_dump, cv->gslot, s));
	return 0;
}

static int eddsa_bkt_dev_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig, const uint8_t *d_hram,
				const uint8_t seed[32], uint32_t piece, uint8_t *d_verdict, uint8_t *d_z_dump, uint32_t *d_sum_dump, hipStream_t s)
{
	EdBktRun R;
	if (eddsa_bkt_setup(ctx, cv, n, d_pub, d_sig, d_hram, seed, piece, d_z_dump, R, s)) {
		return -1;
	}
	// the decoding (two square roots per item: VALU work on the caller's arrays alone) on the side stream, beside the scalars and the filing
	const bool beside = ctx->side_ok && getenv("ECAMD_NO_BKT_BESIDE") == nullptr;
	hipStream_t ps = s;
	if (beside) {
		HIPCHK(hipEventRecord(ctx->side_fork, s));
		HIPCHK(hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0));
		ps = ctx->side_stream;
	}
	HIPCHK(ecamd_launch_edbkt(R.A, R.B, 0, nullptr, nullptr, nullptr, cv->gslot, ps));
	if (beside) {
		HIPCHK(hipEventRecord(ctx->side_done, ctx->side_stream));
	}
	HIPCHK(ecamd_launch_edmsm_scal(R.C, s));
	if (beside) {
		HIPCHK(hipStreamWaitEvent(s, ctx->side_done, 0));   // (the lane kernel reads the decoding's flags)
	}
	HIPCHK(ecamd_launch_edmsm_lane(R.N, s));
	HIPCHK(ecamd_launch_edbkt_file(R.B, s));
	return eddsa_bkt_tail(ctx, cv, R, d_verdict, d_sum_dump, s);
}

// The same combination FILED CHUNK BY CHUNK (round 6, ec_eddsa_verify_msg_prj_all_batch): a batch that arrives through the host pipeline is
// copy-bound while it arrives -- 285 MB per 2^20 items at PCIe rate, the device nearly idle -- and the combination used to start when the last
// chunk was in (7 ms).  Its per-item stages (the two decodings, the scalars, the filing: 4.4 of the 7 ms) now run on each chunk as it lands;
// what is left for the end is the base point's copies, the ranking, the additions and the reduction.  z_i is keyed by the item's index in the
// batch, so the verdict is that of eddsa_bkt_dev_locked with the same seed.
static int eddsa_bkt_stream_begin(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig, const uint8_t *d_hram,
				  const uint8_t seed[32], EdBktRun &R, hipStream_t s)
{
	if (eddsa_bkt_setup(ctx, cv, n, d_pub, d_sig, d_hram, seed, 0, nullptr, R, s)) {
		return -1;
	}
	HIPCHK(hipMemsetAsync(R.B.count, 0, ((size_t)16 << 16) * 4, s));
	return 0;
}
static int eddsa_bkt_stream_chunk(ecamd_curve *cv, EdBktRun &R, uint32_t first, uint32_t count, hipStream_t s)
{
	if (count == 0) {
		return 0;
	}
	R.A.first = R.C.first = R.B.first = first;
	R.A.count = R.C.count = R.B.count_items = count;
	R.B.part = 1;
	HIPCHK(ecamd_launch_edbkt(R.A, R.B, 0, nullptr, nullptr, nullptr, cv->gslot, s));
	HIPCHK(ecamd_launch_edmsm_scal(R.C, s));
	HIPCHK(ecamd_launch_edbkt_file(R.B, s));
	return 0;
}
static int eddsa_bkt_stream_end(ecamd_ctx *ctx, ecamd_curve *cv, EdBktRun &R, uint8_t *d_verdict, hipStream_t s)
{
	R.A.first = R.A.count = R.C.first = R.C.count = 0;
	HIPCHK(ecamd_launch_edmsm_lane(R.N, s));
	R.B.part = 2;
	HIPCHK(ecamd_launch_edbkt_file(R.B, s));
	return eddsa_bkt_tail(ctx, cv, R, d_verdict, nullptr, s);
}

// buckets or the Straus loop for a piece of n items ($ECAMD_ED_MSM_ALGO=straus|bucket overrides the size rule)
static bool eddsa_msm_use_buckets(uint32_t n)
{
	const char *e = getenv("ECAMD_ED_MSM_ALGO");
	const bool force_b = e && !strcmp(e, "bucket"), force_s = e && !strcmp(e, "straus");
	return force_b || (!force_s && n >= (1u << 18));   // measured: 2^17 items 2.18 ms by buckets, 2.06 by Straus; 2^18: 2.80 / 3.22; 2^20: 6.85 / 10.8
}

static int eddsa_msm_dev_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig,
				const uint8_t *d_hram, const uint8_t seed[32], uint32_t piece, uint8_t *d_verdict, uint8_t *d_z_dump,
				uint32_t *d_sum_dump, hipStream_t s)
{
	if (eddsa_msm_use_buckets(n)) {
		return eddsa_bkt_dev_locked(ctx, cv, n, d_pub, d_sig, d_hram, seed, piece, d_verdict, d_z_dump, d_sum_dump, s);
	}
	const uint32_t K = eddsa_msm_pick_k(ctx, n);
	const uint32_t L = (n + K - 1) / K;
	size_t off = 0;
	auto carve = [&](size_t bytes) {
		const size_t o = off;
		off += msm_align(bytes);
		return o;
	};
	const size_t o_tbl = carve((size_t)n * 2 * ECAMD_EDT_ITEM_WORDS * 4);
	const size_t o_cA = carve((size_t)n * 32), o_zR = carve((size_t)n * 20), o_zs = carve((size_t)n * 32);
	const size_t o_flags = carve(n), o_flagsS = carve(n);
	const size_t o_sB = carve((size_t)L * 32), o_rec = carve((size_t)L * ECAMD_EDM_REC_WORDS * 4);
	const size_t o_tmp = carve(((size_t)L / 16 + 1) * ECAMD_EDM_REC_WORDS * 4);
	const size_t o_tblB = carve((size_t)ECAMD_EDT_ITEM_WORDS * 4), o_word = carve(4);
	if (ensure(&ctx->msm, &ctx->msm_bytes, off)) {
		return -1;
	}
	uint8_t *M = ctx->msm;
	HIPCHK(hipMemsetAsync(M + o_word, 0, 4, s));
	EcamdEdMsmArgs A;
	memset(&A, 0, sizeof(A));
	A.encA = d_pub;
	A.strideA = 32;
	A.encR = d_sig;
	A.strideR = 64;
	A.tbl = (uint32_t *)(M + o_tbl);
	A.flags = M + o_flags;
	A.cA = (const uint32_t *)(M + o_cA);
	A.zR = (const uint32_t *)(M + o_zR);
	A.sB = (const uint32_t *)(M + o_sB);
	A.tblB = (const uint32_t *)(M + o_tblB);
	A.rec = (uint32_t *)(M + o_rec);
	A.n = n;
	A.K = K;
	A.L = L;
	A.cof_dbl = cv->ed_cof_dbl;
	memcpy(A.g_d, cv->ed_tmpl.g_d, sizeof(A.g_d));
	memcpy(A.g_sm1, cv->ed_tmpl.g_sm1, sizeof(A.g_sm1));
	memcpy(A.g_2d, cv->ed_2d, sizeof(A.g_2d));
	memcpy(A.g_Bx, cv->ed_Bx, sizeof(A.g_Bx));
	memcpy(A.g_By, cv->ed_By, sizeof(A.g_By));
	HIPCHK(ecamd_launch_edmsm_btable(A, (uint32_t *)(M + o_tblB), cv->gslot, s));
	HIPCHK(ecamd_launch_edmsm_prep(A, cv->gslot, s));
	EcamdEdMsmScalArgs C;
	memset(&C, 0, sizeof(C));
	C.sigs = d_sig;
	C.hram = d_hram;
	C.cA = (uint32_t *)(M + o_cA);
	C.zR = (uint32_t *)(M + o_zR);
	C.zs = (uint32_t *)(M + o_zs);
	C.flagsS = M + o_flagsS;
	C.z_dump = d_z_dump;
	memcpy(C.seed, seed, 32);
	C.nonce[0] = piece;
	C.n = n;
	C.qslot = cv->qslot;
	HIPCHK(ecamd_launch_edmsm_scal(C, s));
	EcamdEdMsmLaneArgs N;
	memset(&N, 0, sizeof(N));
	N.zs = (const uint32_t *)(M + o_zs);
	N.flags = M + o_flags;
	N.flagsS = M + o_flagsS;
	N.sB = (uint32_t *)(M + o_sB);
	N.flagword = (uint32_t *)(M + o_word);
	N.n = n;
	N.K = K;
	N.L = L;
	N.qslot = cv->qslot;
	HIPCHK(ecamd_launch_edmsm_lane(N, s));
	if (ctx->timing) {
		HIPCHK(hipEventRecord(ctx->ev_dom[0], s));   // the dominant kernel: k_edmsm_loop (ecamd_ctx_dominant_kernel_ms)
	}
	HIPCHK(ecamd_launch_edmsm_loop(A, cv->gslot, s));
	if (ctx->timing) {
		HIPCHK(hipEventRecord(ctx->ev_dom[1], s));
		ctx->ev_dom_valid = true;
	}
	HIPCHK(ecamd_launch_edmsm_reduce(A, (uint32_t *)(M + o_tmp), (const uint32_t *)(M + o_word), d_verdict, d_sum_dump, cv->gslot, s));
	return 0;
}

// host arrays -> one verdict: pieces of max_chunk items, each with its own combination.  *accept = 1 when every piece accepts.
static int eddsa_msm_host_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
				 const uint8_t *hram, const uint8_t *fixed_seed, int *accept, uint8_t *z_out, uint32_t *sum_out)
{
	uint8_t seed[32];
	if (fixed_seed) {
		memcpy(seed, fixed_seed, 32);
	} else if (msm_seed(ctx, seed)) {
		return -1;
	}
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	const uint32_t pieces = (n + chunk - 1) / chunk;
	if (stage_need(ctx, MH_PUB, (size_t)chunk * 32) || stage_need(ctx, MH_SIG, (size_t)chunk * 64) ||
	    stage_need(ctx, MH_HRAM, (size_t)chunk * 64) ||
	    stage_need(ctx, MH_VERDICTS, (size_t)pieces + (z_out ? (size_t)chunk * 16 : 0) + 256 + ECAMD_EDM_REC_WORDS * 4)) {
		return -1;
	}
	uint8_t *d_verdicts = ctx->stage[MH_VERDICTS];
	HIPCHK(hipMemsetAsync(d_verdicts, 0, pieces, s));
	uint32_t *d_sum = (uint32_t *)(ctx->stage[MH_VERDICTS] + ((pieces + 255) & ~(size_t)255));
	uint8_t *d_z = z_out ? (uint8_t *)(d_sum + ECAMD_EDM_REC_WORDS) : nullptr;
	for (uint32_t off = 0, pc = 0; off < n; off += chunk, pc++) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		HIPCHK(hipMemcpyAsync(ctx->stage[MH_PUB], pubkeys + (size_t)off * 32, (size_t)m * 32, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(ctx->stage[MH_SIG], sigs + (size_t)off * 64, (size_t)m * 64, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(ctx->stage[MH_HRAM], hram + (size_t)off * 64, (size_t)m * 64, hipMemcpyHostToDevice, s));
		if (eddsa_msm_dev_locked(ctx, cv, m, ctx->stage[MH_PUB], ctx->stage[MH_SIG], ctx->stage[MH_HRAM], seed, pc, d_verdicts + pc, d_z,
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
		HIPCHK(hipMemcpyAsync(sum_out, d_sum, ECAMD_EDM_REC_WORDS * 4, hipMemcpyDeviceToHost, s));
	}
	HIPCHK(hipStreamSynchronize(s));
	*accept = 1;
	for (uint32_t pc = 0; pc < pieces; pc++) {
		if (v[pc] != 0) {
			*accept = 0;
		}
	}
	return 0;
}

// all_valid != NULL (round 6, Ed25519 only): ONE accept bit instead of per-item results -- the front end of every chunk (import, encoding, hashes)
// files the encoded keys, the signatures and the hashes in batch-wide arrays (EB_KEYS, EB_SIGS, EB_HRAM; EB_MARKS: per-item "the key has no encoding"), and when
// the last chunk is in the batch equation is evaluated once per max_chunk items (eddsa_msm_dev_locked: by buckets from 2^18 items on).
// *all_valid = 0: not decided here (ec_eddsa_verify_all_batch's contract without its item-by-item pass: the caller has one).
static int eddsa_verify_msg_prj_impl(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
				     const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, const uint8_t *msg_slots, uint32_t msg_stride,
				     uint8_t *result, int *all_valid = nullptr)
{
	const std::string f(fn);
	if (!ctx || !cv_in) {
		return fail(f + ": bad argument");
	}
	// Ed25519 (WEI25519 handle): 32-octet keys, SHA-512; Ed448 (WEI448 handle): 57-octet keys, SHAKE256 with 114 octets (pre-hash: 64)
	const bool e448 = cv_in->pbits == 448;
	const uint32_t kl = e448 ? 57u : 32u, sl = 2 * kl, hl = sl;
	const int hash_type = e448 ? 5 : 4;
	const uint32_t blank = msg_slots ? kl + 64u : kl;   // A, or A || PH(M)
	if (stride < 4 || (stride & 3u) || stride > 4096 || (uint64_t)a_offset + 4 + blank > stride) {
		return fail(f + ": bad argument (stride: a multiple of 4 in 4 .. 4096; the blank for A [and PH(M)] must lie inside the slot)");
	}
	if (msg_slots && (msg_stride < 4 || (msg_stride & 3u) || msg_stride > 4096)) {
		return fail(f + ": bad argument (msg_stride: a multiple of 4 in 4 .. 4096)");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	EcamdEdSignArgs T;
	uint8_t dummy = 0;
	if (eddsa_sign_setup(fn, ctx, cv_in, n, keys_prj, sigs, hash_slots, &T) ||
	    eddsa_args_ok(fn, ctx, cv_in, n, keys_prj, sigs, hash_slots, all_valid ? &dummy : result, hl)) {
		return -1;
	}
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	const size_t cl = (size_t)cv->clen;
	uint8_t seed[32] = {0};
	uint32_t done = 0;
	if (all_valid) {
		*all_valid = 0;
		if (e448 ? !eddsa448_msm_available(cv) : !eddsa_msm_available(cv)) {
			return 0;   // not decided here
		}
		if (msm_seed(ctx, seed) || stage_need(ctx, EB_KEYS, (size_t)n * kl) || stage_need(ctx, EB_SIGS, (size_t)n * sl) ||
		    stage_need(ctx, EB_HRAM, (size_t)n * hl) || stage_need(ctx, EB_MARKS, (size_t)n + 256)) {
			return -1;
		}
	}
	std::vector<HostArr> arrs = {{keys_prj, nullptr, 3 * cl}, {sigs, nullptr, sl}, {hash_slots, nullptr, stride}, {nullptr, all_valid ? nullptr : result, 1}};
	if (msg_slots) {
		arrs.push_back({msg_slots, nullptr, msg_stride});
	}
	// Ed25519, one piece, by buckets: the combination's per-item stages on every chunk as it lands (eddsa_bkt_stream_*; $ECAMD_NO_ED_STREAM: the
	// whole combination after the last chunk, as for Ed448 and for batches of several pieces)
	EdBktRun run;
	const bool streamed = all_valid && !e448 && n <= ctx->max_chunk && eddsa_msm_use_buckets(n) && getenv("ECAMD_NO_ED_STREAM") == nullptr;
	if (streamed) {
		StreamScope scope(ctx, ctx->stream);
		if (eddsa_bkt_stream_begin(ctx, cv, n, ctx->stage[EB_KEYS], ctx->stage[EB_SIGS], ctx->stage[EB_HRAM], seed, run, ctx->stream)) {
			return -1;
		}
	}
	const int prc = host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		// EP_: the affine keys and their import status, the encodings and theirs (the verification core owns the EV_ frame)
		if (stage_need(ctx, EP_AFF, (size_t)m * 2 * cl) || stage_need(ctx, EP_PRE, m) ||
		    stage_need(ctx, EP_KEY, (size_t)m * kl) || stage_need(ctx, EP_KST, m)) {
			return -1;
		}
		uint8_t *slots = const_cast<uint8_t *>(ip[2]);   // the staged copy of the caller's slots
		if (msg_slots) {
			// PH(M): SHA-512(M), or the first 64 octets of SHAKE256(M), of every message, written behind the blank for A
			// (eddsa_compute_pre_hash, sig/eddsa.c:1049-1080, :1650-1657)
			if (ecdsa_hash_stage(ctx, hash_type, m, ip[4], msg_stride, 64, s)) {
				return -1;
			}
			HIPCHK(ecamd_launch_slot_patch(slots, stride, a_offset + kl, ctx->stage[ST_DIGESTS], 64, nullptr, m, s));
		}
		EcamdPrjInArgs I;
		I.in = ip[0];
		I.aff = ctx->stage[EP_AFF];
		I.pre = ctx->stage[EP_PRE];
		I.n = m;
		I.clen = (uint32_t)cl;
		I.for_mul = 0;
		I.slot = cv->slot;
		HIPCHK(launch_prj_import(cv, I, s));
		EcamdEdSignArgs A = T;
		A.n = m;
		A.Rw = ctx->stage[EP_AFF];
		A.stR = ctx->stage[EP_PRE];
		// (the whole-batch form files the encodings and their "no encoding" marks in batch-wide arrays: Ed25519's 32-octet encodings are written
		// there directly; Ed448's 57-octet ones keep their aligned staging and a copy)
		const bool direct = all_valid && !e448;
		A.out = direct ? ctx->stage[EB_KEYS] + (size_t)done * kl : ctx->stage[EP_KEY];
		A.status = direct ? ctx->stage[EB_MARKS] + (size_t)done : ctx->stage[EP_KST];
		HIPCHK(launch_ed_sign_enc(cv, A, s));
		HIPCHK(ecamd_launch_slot_patch(slots, stride, a_offset, A.out, kl, A.status, m, s));
		if (all_valid) {
			// the whole-batch form: file this chunk's encoded keys, signatures, hashes and "no encoding" marks; the equation comes at the end
			if (ecdsa_hash_stage(ctx, hash_type, m, slots, stride, hl, s)) {
				return -1;
			}
			if (!direct) {
				HIPCHK(hipMemcpyAsync(ctx->stage[EB_KEYS] + (size_t)done * kl, ctx->stage[EP_KEY], (size_t)m * kl, hipMemcpyDeviceToDevice, s));
				HIPCHK(hipMemcpyAsync(ctx->stage[EB_MARKS] + (size_t)done, ctx->stage[EP_KST], m, hipMemcpyDeviceToDevice, s));
			}
			HIPCHK(hipMemcpyAsync(ctx->stage[EB_SIGS] + (size_t)done * sl, ip[1], (size_t)m * sl, hipMemcpyDeviceToDevice, s));
			HIPCHK(hipMemcpyAsync(ctx->stage[EB_HRAM] + (size_t)done * hl, ctx->stage[ST_DIGESTS], (size_t)m * hl, hipMemcpyDeviceToDevice, s));
			if (streamed && eddsa_bkt_stream_chunk(cv, run, done, m, s)) {
				return -1;
			}
			done += m;
			return 0;
		}
		if (ecdsa_hash_stage(ctx, hash_type, m, slots, stride, hl, s) ||
		    (e448 ? eddsa448_verify_dev_locked(ctx, cv, m, ctx->stage[EP_KEY], ip[1], ctx->stage[ST_DIGESTS], op[3], s)
			  : eddsa_verify_dev_locked(ctx, cv, m, ctx->stage[EP_KEY], ip[1], ctx->stage[ST_DIGESTS], 64, op[3], s))) {
			return -1;
		}
		HIPCHK(ecamd_launch_reject_where(op[3], ctx->stage[EP_KST], m, s));
		return 0;
	}, streamed ? (1u << 17) : 0u);
	if (prc || !all_valid) {
		return prc;
	}
	// the batch equation over the filed arrays, a piece of max_chunk items at a time; the verdict byte rests behind the marks
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	uint8_t *d_verdict = ctx->stage[EB_MARKS] + n;
	HIPCHK(hipMemsetAsync(d_verdict, 0, 1, s));
	uint32_t pc = 0;
	if (streamed && eddsa_bkt_stream_end(ctx, cv, run, d_verdict, s)) {
		(void)hipStreamSynchronize(s);
		return -1;
	}
	// (a loop of its own, not for_chunks: pc numbers the pieces for their z_i, and a streamed batch skips the walk)
	for (uint32_t off = 0; off < n && !streamed; off += ctx->max_chunk, pc++) {
		const uint32_t m = (n - off) < ctx->max_chunk ? (n - off) : ctx->max_chunk;
		if (e448 ? eddsa448_msm_dev_locked(ctx, cv, m, ctx->stage[EB_KEYS] + (size_t)off * kl, ctx->stage[EB_SIGS] + (size_t)off * sl, ctx->stage[EB_HRAM] + (size_t)off * hl,
						   seed, pc, d_verdict, s)
			 : eddsa_msm_dev_locked(ctx, cv, m, ctx->stage[EB_KEYS] + (size_t)off * 32, ctx->stage[EB_SIGS] + (size_t)off * 64, ctx->stage[EB_HRAM] + (size_t)off * 64, seed, pc,
						d_verdict, nullptr, nullptr, s)) {
			(void)hipStreamSynchronize(s);
			return -1;
		}
	}
	std::vector<uint8_t> marks((size_t)n + 1, 1);
	HIPCHK(hipMemcpyAsync(marks.data(), ctx->stage[EB_MARKS], (size_t)n + 1, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	memset(seed, 0, sizeof(seed));
	int ok = marks[n] == 0;
	for (uint32_t i = 0; i < n && ok; i++) {
		ok = marks[i] == 0;   // a key without an encoding (not on the curve, at infinity): the reference rejects the item
	}
	*all_valid = ok;
	return 0;
}

// ec_verify_batch's one bit for plain Ed25519 FROM the projective keys, signatures and hash inputs of ec_eddsa_verify_msg_prj_batch (round 6):
// the same front end per staging chunk, then the batch equation over the whole batch as one multi-scalar multiplication per max_chunk
// items.  *all_valid = 0: not decided here -- a bad signature, a key that does not import or has no encoding, or a handle without the
// form (Ed448): the caller verifies item by item.
extern "C" int ec_eddsa_verify_msg_prj_all_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
						 const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, int *all_valid)
{
	if (!all_valid || n == 0) {
		return fail("ec_eddsa_verify_msg_prj_all_batch: bad argument (the reference rejects num = 0 too)");
	}
	const int r = eddsa_verify_msg_prj_impl("ec_eddsa_verify_msg_prj_all_batch", ctx, cv, n, keys_prj, sigs, hash_slots, stride, a_offset, nullptr, 0, nullptr,
						all_valid);
	msm_seed_discard(ctx);
	return r;
}

extern "C" int ec_eddsa_verify_msg_prj_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
					     const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, uint8_t *result)
{
	return eddsa_verify_msg_prj_impl("ec_eddsa_verify_msg_prj_batch", ctx, cv, n, keys_prj, sigs, hash_slots, stride, a_offset, nullptr, 0, result);
}

// The pre-hashed variant (EDDSA25519PH): the hash input is dom2(1, ctx) || R || A || PH(M) with PH(M) = SHA-512(M); the caller leaves 96
// blank octets at a_offset (A, then PH(M)) and hands the messages over in slots of their own, hashed on the device as well.
extern "C" int ec_eddsa_verify_ph_prj_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *keys_prj, const uint8_t *sigs,
					    const uint8_t *hash_slots, uint32_t stride, uint32_t a_offset, const uint8_t *msg_slots, uint32_t msg_stride,
					    uint8_t *result)
{
	if (n && !msg_slots) {
		return fail("ec_eddsa_verify_ph_prj_batch: bad argument");
	}
	static const uint8_t none = 0;
	return eddsa_verify_msg_prj_impl("ec_eddsa_verify_ph_prj_batch", ctx, cv, n, keys_prj, sigs, hash_slots, stride, a_offset, msg_slots ? msg_slots : &none,
					 msg_stride, result);
}

// the combination behind the checks of ec_eddsa_verify_all_batch_dev (ctx->mu held, a StreamScope open): d_verdict[0] = 0 / 1
static int eddsa_verify_all_dev_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const void *d_pubkeys, const void *d_sigs, const void *d_hram,
				       const uint8_t seed[32], void *d_verdict, hipStream_t s)
{
	const bool e448 = cv->pbits == 448;
	HIPCHK(hipMemsetAsync(d_verdict, 0, 1, s));
	uint32_t pc = 0;
	// (a loop of its own, not for_chunks: pc numbers the pieces for their z_i)
	for (uint32_t off = 0; off < n; off += ctx->max_chunk, pc++) {
		const uint32_t m = (n - off) < ctx->max_chunk ? (n - off) : ctx->max_chunk;
		if (e448) {
			if (eddsa448_msm_dev_locked(ctx, cv, m, (const uint8_t *)d_pubkeys + (size_t)off * 57, (const uint8_t *)d_sigs + (size_t)off * 114,
						    (const uint8_t *)d_hram + (size_t)off * 114, seed, pc, (uint8_t *)d_verdict, s)) {
				return -1;
			}
			continue;
		}
		if (eddsa_msm_dev_locked(ctx, cv, m, (const uint8_t *)d_pubkeys + (size_t)off * 32, (const uint8_t *)d_sigs + (size_t)off * 64,
					 (const uint8_t *)d_hram + (size_t)off * 64, seed, pc, (uint8_t *)d_verdict, nullptr, nullptr, s)) {
			return -1;
		}
	}
	return 0;
}

static int eddsa_verify_all_batch_dev_impl(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const void *d_pubkeys,
					     const void *d_sigs, const void *d_hram, uint32_t hram_len, void *d_verdict,
					     void *hip_stream)
{
	if (!ctx) {
		return fail("ec_eddsa_verify_all_batch_dev: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	if (eddsa_args_ok("ec_eddsa_verify_all_batch_dev", ctx, cv_in, n, d_pubkeys, d_sigs, d_hram, d_verdict, hram_len)) {
		return -1;
	}
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	const bool e448 = cv->pbits == 448;
	if (n == 0 || (e448 ? !eddsa448_msm_available(cv) : !eddsa_msm_available(cv))) {
		return fail("ec_eddsa_verify_all_batch_dev: needs n > 0 and Ed25519 (the WEI25519 handle on the 2^255 - 19 unit) or Ed448 (WEI448 on the Goldilocks unit)");
	}
	uint8_t seed[32];
	if (msm_seed(ctx, seed)) {
		return -1;
	}
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
	StreamScope scope(ctx, s);
	return eddsa_verify_all_dev_locked(ctx, cv, n, d_pubkeys, d_sigs, d_hram, seed, d_verdict, s);
}
extern "C" int ec_eddsa_verify_all_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const void *d_pubkeys,
					     const void *d_sigs, const void *d_hram, uint32_t hram_len, void *d_verdict,
					     void *hip_stream)
{
	const int r = eddsa_verify_all_batch_dev_impl(ctx, cv_in, n, d_pubkeys, d_sigs, d_hram, hram_len, d_verdict, hip_stream);
	msm_seed_discard(ctx);
	return r;
}

// test hook: the combination with a caller-chosen seed; z_out (n x 16 little-endian z_i) and sum_out (36 words: X, Y, Z, T of
// the sum before the cofactor, radix-2^29 digits of lazily reduced residues) may be NULL.  n <= the context's max_chunk.
extern "C" int ecamd_debug_eddsa_msm(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const uint8_t *pubkeys,
				     const uint8_t *sigs, const uint8_t *hram, const uint8_t seed[32], int *accept, uint8_t *z_out,
				     uint32_t *sum_out)
{
	if (!ctx || !accept || !seed) {
		return fail("ecamd_debug_eddsa_msm: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	uint8_t dummy = 0;
	if (eddsa_args_ok("ecamd_debug_eddsa_msm", ctx, cv_in, n, pubkeys, sigs, hram, &dummy, 64)) {
		return -1;
	}
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	if (n == 0 || n > ctx->max_chunk || !eddsa_msm_available(cv)) {
		return fail("ecamd_debug_eddsa_msm: needs Ed25519 on the 2^255 - 19 unit and 0 < n <= max_chunk");
	}
	HIPCHK(hipSetDevice(ctx->device));
	return eddsa_msm_host_locked(ctx, cv, n, pubkeys, sigs, hram, seed, accept, z_out, sum_out);
}

// Whole-batch predicate of ec_verify_batch (sig/sig_algs.c:675, eddsa_verify_batch sig/eddsa.c:2904): libecc accepts the
// batch when one random linear combination of the cofactored equations vanishes, which holds when every signature verifies
// and fails otherwise except with probability ~2^-128 over its random z_i.  Here every item is verified (the batch is the
// parallel dimension already), so the bit is the exact conjunction and the first rejected index comes for free.
static int eddsa_verify_all_batch_impl(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys,
				       const uint8_t *sigs, const uint8_t *hram, uint32_t hram_len, int *all_valid,
				       uint32_t *first_rejected)
{
	if (!all_valid || n == 0) {
		return fail("ec_eddsa_verify_all_batch: bad argument (the reference rejects num = 0 too)");
	}
	*all_valid = 0;
	if (first_rejected) {
		*first_rejected = n;
	}
	// large Ed25519 batches: the reference's own batch equation as one multi-scalar multiplication first; only a batch it
	// rejects is verified item by item (for the first rejected index, and because a rejection of the combination proves
	// that some item fails while the item-by-item results say which)
	if (ctx && cv && cv->ctx == ctx && pubkeys && sigs && hram && hram_len == 64 && cv->pbits == 255) {
		std::lock_guard<std::mutex> lk(ctx->mu);
		ecamd_curve *cw = const_cast<ecamd_curve *>(cv);
		if (ctx->eddsa_msm != 0 && (ctx->eddsa_msm == 2 || n >= ctx->msm_min)) {
			if (cw->ed_state == 0) {
				ed_setup(cw);
			}
			if (eddsa_msm_available(cw)) {
				HIPCHK(hipSetDevice(ctx->device));
				int accept = 0;
				if (eddsa_msm_host_locked(ctx, cw, n, pubkeys, sigs, hram, nullptr, &accept, nullptr, nullptr)) {
					return -1;
				}
				if (accept) {
					*all_valid = 1;
					return 0;
				}
			}
		}
	}
	// Ed448 (round 6): the same, on the Weierstrass model with the cofactored final test (eddsa448_msm_dev_locked)
	if (ctx && cv && cv->ctx == ctx && pubkeys && sigs && hram && hram_len == 114 && cv->pbits == 448) {
		std::lock_guard<std::mutex> lk(ctx->mu);
		ecamd_curve *cw = const_cast<ecamd_curve *>(cv);
		if (ctx->eddsa_msm != 0 && (ctx->eddsa_msm == 2 || n >= ctx->msm_min)) {
			if (cw->ed448_state == 0) {
				ed448_setup(cw);
			}
			if (eddsa448_msm_available(cw)) {
				HIPCHK(hipSetDevice(ctx->device));
				int accept = 0;
				if (eddsa448_msm_host_locked(ctx, cw, n, pubkeys, sigs, hram, &accept)) {
					return -1;
				}
				if (accept) {
					*all_valid = 1;
					return 0;
				}
			}
		}
	}
	std::vector<uint8_t> res(n, 1);
	if (ec_eddsa_verify_batch(ctx, cv, n, pubkeys, sigs, hram, hram_len, res.data())) {
		return -1;
	}
	uint32_t i = 0;
	while (i < n && res[i] == 0) {   // any non-zero byte is a rejection
		i++;
	}
	*all_valid = (i == n) ? 1 : 0;
	if (first_rejected) {
		*first_rejected = i;
	}
	return 0;
}
extern "C" int ec_eddsa_verify_all_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys,
					 const uint8_t *sigs, const uint8_t *hram, uint32_t hram_len, int *all_valid,
					 uint32_t *first_rejected)
{
	const int r = eddsa_verify_all_batch_impl(ctx, cv, n, pubkeys, sigs, hram, hram_len, all_valid, first_rejected);
	msm_seed_discard(ctx);
	return r;
}

// ------------------------------------------------------------------------------------------
// Ed25519 signing: the two device-side steps of _eddsa_sign (sig/eddsa.c:1554-1870) around the caller's hashes
// ------------------------------------------------------------------------------------------

// SR_: r big-endian, [r]G and its status
static int eddsa_sign_R_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, const EcamdEdSignArgs &T, uint32_t n,
				   const uint8_t *d_rhash, uint8_t *d_Renc, uint8_t *d_status, hipStream_t s)
{
	if (n > ctx->max_chunk) {  // bound the scratch: pieces of max_chunk items, in order on the stream
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return eddsa_sign_R_dev_locked(ctx, cv, T, m, d_rhash + (size_t)off * (T.is448 ? 114 : 64), d_Renc + (size_t)off * (T.is448 ? 57 : 32),
						       d_status + off, s);
		});
	}
	const uint32_t cl = (uint32_t)cv->clen;   // 32 / 56
	if (stage_need(ctx, SR_R, (size_t)n * cl) || stage_need(ctx, SR_RW, (size_t)n * 2 * cl) ||
	    stage_need(ctx, SR_STR, n)) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	EcamdEdSignArgs A = T;
	A.n = n;
	A.r_hash = d_rhash;
	A.r_be = S[SR_R];
	HIPCHK(ecamd_launch_ed_sign_r(A, s));
	if (smul_dev_locked(ctx, cv, n, S[SR_R], cl, nullptr, S[SR_RW], S[SR_STR], s)) {   // prj_pt_mul(r, G) (:1776; Ed448: r / 4, :1746)
		return -1;
	}
	A.Rw = S[SR_RW];
	A.stR = S[SR_STR];
	A.out = d_Renc;
	A.status = d_status;
	HIPCHK(launch_ed_sign_enc(cv, A, s));
	return 0;
}

extern "C" int ec_eddsa_sign_R_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *r_hash, uint8_t *R_enc,
				     uint8_t *status)
{
	if (!ctx) {
		return fail("ec_eddsa_sign_R_batch: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	EcamdEdSignArgs T;
	if (eddsa_sign_setup("ec_eddsa_sign_R_batch", ctx, cv, n, r_hash, R_enc, status, &T)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	const std::vector<HostArr> arrs = {{r_hash, nullptr, (size_t)(T.is448 ? 114 : 64)}, {nullptr, R_enc, (size_t)(T.is448 ? 57 : 32)}, {nullptr, status, 1}};
	return host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return eddsa_sign_R_dev_locked(ctx, cv, T, m, ip[0], op[1], op[2], s);
	});
}

// eddsa_export_pub_key in batch (sig/eddsa.c:795-860): the projective Weierstrass point an ec_pub_key holds ->
// prj_pt_shortw_to_aff_pt_edwards -> eddsa_encode_point, i.e. the octets the verifier hashes as "A".  (libecc spends about
// 1.5 ms of CPU per call on it -- it rebuilds the curve maps every time --, which is what made ec_verify_batch through
// libsign_amd.so host-bound by three orders of magnitude before this entry point existed.)
extern "C" int ec_eddsa_encode_point_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *points_prj,
					   uint8_t *enc, uint8_t *status)
{
	if (!ctx) {
		return fail("ec_eddsa_encode_point_batch: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	EcamdEdSignArgs T;
	if (eddsa_sign_setup("ec_eddsa_encode_point_batch", ctx, cv, n, points_prj, enc, status, &T)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	const size_t cl = (size_t)cv->clen, kl = T.is448 ? 57 : 32;
	const std::vector<HostArr> arrs = {{points_prj, nullptr, 3 * cl}, {nullptr, enc, kl}, {nullptr, status, 1}};
	return host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		// import status: 0 / 1 error / 2 infinity, the encode kernel's convention
		if (stage_need(ctx, EN_AFF, (size_t)m * 2 * cl) || stage_need(ctx, EN_PRE, m)) {
			return -1;
		}
		EcamdPrjInArgs I;
		I.in = ip[0];
		I.aff = ctx->stage[EN_AFF];
		I.pre = ctx->stage[EN_PRE];
		I.n = m;
		I.clen = (uint32_t)cl;
		I.for_mul = 0;
		I.slot = cv->slot;
		HIPCHK(launch_prj_import(cv, I, s));
		EcamdEdSignArgs A = T;
		A.n = m;
		A.Rw = ctx->stage[EN_AFF];
		A.stR = ctx->stage[EN_PRE];
		A.out = op[1];
		A.status = op[2];
		HIPCHK(launch_ed_sign_enc(cv, A, s));
		return 0;
	});
}

extern "C" int ec_eddsa_sign_S_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *r_hash,
				     const uint8_t *hram, const uint8_t *a_scalars, uint8_t *S_out)
{
	if (!ctx || (n && !S_out)) {
		return fail("ec_eddsa_sign_S_batch: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	EcamdEdSignArgs T;
	if (eddsa_sign_setup("ec_eddsa_sign_S_batch", ctx, cv, n, r_hash, hram, a_scalars, &T)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	const size_t hl = T.is448 ? 114 : 64, kl = T.is448 ? 57 : 32;
	const std::vector<HostArr> arrs = {{r_hash, nullptr, hl}, {hram, nullptr, hl}, {a_scalars, nullptr, kl}, {nullptr, S_out, kl}};
	return host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		EcamdEdSignArgs A = T;
		A.n = m;
		A.r_hash = ip[0];
		A.hram = ip[1];
		A.a = ip[2];
		A.out = op[3];
		HIPCHK(ecamd_launch_ed_sign_S(A, s));
		return 0;
	});
}

// ------------------------------------------------------------------------------------------
// one-call EdDSA signing (include/libecc_amd.h: ec_eddsa_sign_msg_batch, ec_eddsa_pub_key_batch): eddsa_import_key_pair_from_priv_key_buf
// (sig/eddsa.c:1028) + _eddsa_sign (:1554-1870) per item with every hash on the device (ecamd_eddsa_sign.hip).  Per chunk of at
// most max_chunk items:
//   k_eddsa_expand_r        h = H(sk), clamp, PH(M), r_hash: a into ES_A, r_hash into ES_RHASH, a zero-extended into ES_AWIDE (keys derived
//                           here), PH(M) into 40, the slot check into 36.  30 - 32 are secret: ensure() wipes what it frees,
//                           ecamd_ctx_wipe_scratch the rest
//   eddsa_sign_R_dev_locked pubkeys == NULL: A = encode([a]B) from ES_AWIDE (Ed448: a / 4 and the isogeny, as eddsa_init_pub_key :840
//                           does with a >> 2) into pub_out or ES_AENC, its status into ES_STA
//   eddsa_sign_R_dev_locked R = encode([r]B) into ES_R, its status into ES_STR
//   k_eddsa_hram            H(dom || R || A || M-or-PH(M)) into ES_HRAM, R into the signature
//   k_ed_sign_S             S = r + hram a mod q into ES_S
//   k_eddsa_sign_fin        S into the signature; status; zero bytes where the slot was bad
// Only enqueues.
// ------------------------------------------------------------------------------------------
static void eddsa_front_args(EcamdEddsaSignArgs *E, const eced::Dom &dom)
{
	memset(E, 0, sizeof(*E));
	E->dom_len = dom.len;
	static_assert(sizeof(E->dom) == sizeof(dom.b), "the dom buffer of the kernel arguments");
	memcpy(E->dom, dom.b, sizeof(E->dom));
}

// the messages of a ragged call (ec_eddsa_*_msgs_*): the packed array and the n + 1 offsets, in place of slots
struct EdRagged {
	const uint8_t *d_msgs;
	uint64_t msgs_len;
	const uint64_t *d_offsets;
};

static int eddsa_sign_msg_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, const EcamdEdSignArgs &T, int alg, const eced::Dom &dom, uint32_t n,
				     const uint8_t *d_sk, const uint8_t *d_pub, const uint8_t *d_slots, uint32_t stride, uint8_t *d_sigs,
				     uint8_t *d_pub_out, uint8_t *d_status, hipStream_t s, const EdRagged *rg = nullptr)
{
	const size_t kl = T.is448 ? 57 : 32, hl = 2 * kl;
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	const bool derive = d_pub == nullptr, ph = eced::alg_is_ph(alg);
	if (stage_need(ctx, {{ES_A, chunk * kl}, {ES_RHASH, chunk * hl}, {ES_AWIDE, derive ? chunk * hl : 0}, {ES_HRAM, chunk * hl}, {ES_R, chunk * kl},
			     {ES_S, chunk * kl}, {ES_BAD, chunk}, {ES_STR, chunk}, {ES_STA, derive ? chunk : 0},
			     {ES_AENC, derive && !d_pub_out ? chunk * kl : 0}, {ES_PH, ph ? (size_t)chunk * eced::PH_LEN : 0}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	for (uint32_t off = 0; off < n; off += chunk) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		EcamdEddsaSignArgs E;
		eddsa_front_args(&E, dom);
		E.n = m;
		E.sk = d_sk + off * kl;
		E.slots = d_slots + (size_t)off * stride;
		E.stride = stride;
		E.a = S[ES_A];
		E.r_hash = S[ES_RHASH];
		E.a_wide = derive ? S[ES_AWIDE] : nullptr;
		E.hram = S[ES_HRAM];
		E.bad = S[ES_BAD];
		E.ph = ph ? S[ES_PH] : nullptr;
		EcamdEddsaMsgsArgs M;
		if (rg) {   // k_eddsa_expand_r_msgs / k_eddsa_hram_msgs in place of the slot kernels; everything between them is the same
			E.slots = nullptr;
			E.stride = 0;
			M.vsigs = nullptr;
			M.msgs = rg->d_msgs;
			M.msgs_len = rg->msgs_len;
			M.offsets = rg->d_offsets + off;
			M.e = E;
			HIPCHK(ecamd_launch_eddsa_expand_msgs(alg, M, s));
		} else {
			HIPCHK(ecamd_launch_eddsa_expand(alg, E, s));
		}
		const uint8_t *A_enc = derive ? nullptr : d_pub + off * kl;
		if (derive) {
			uint8_t *dst = d_pub_out ? d_pub_out + off * kl : S[ES_AENC];
			if (eddsa_sign_R_dev_locked(ctx, cv, T, m, S[ES_AWIDE], dst, S[ES_STA], s)) {
				return -1;
			}
			A_enc = dst;
		} else if (d_pub_out) {
			HIPCHK(hipMemcpyAsync(d_pub_out + off * kl, A_enc, m * kl, hipMemcpyDeviceToDevice, s));
		}
		if (eddsa_sign_R_dev_locked(ctx, cv, T, m, S[ES_RHASH], S[ES_R], S[ES_STR], s)) {
			return -1;
		}
		E.R = S[ES_R];
		E.A = A_enc;
		E.sigs = d_sigs + off * 2 * kl;
		if (rg) {
			M.e = E;
			HIPCHK(ecamd_launch_eddsa_hram_msgs(alg, M, s));
		} else {
			HIPCHK(ecamd_launch_eddsa_hram(alg, E, s));
		}
		EcamdEdSignArgs G = T;
		G.n = m;
		G.r_hash = S[ES_RHASH];
		G.hram = S[ES_HRAM];
		G.a = S[ES_A];
		G.out = S[ES_S];
		HIPCHK(ecamd_launch_ed_sign_S(G, s));
		E.S = S[ES_S];
		E.stR = S[ES_STR];
		E.stA = derive ? S[ES_STA] : nullptr;
		E.status = d_status + off;
		HIPCHK(ecamd_launch_eddsa_sign_fin(alg, E, s));
	}
	return 0;
}

// ES_A, ES_AWIDE: a, and a zero-extended (both secret)
static int eddsa_pub_key_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, const EcamdEdSignArgs &T, uint32_t n, const uint8_t *d_sk,
				    uint8_t *d_pub_out, uint8_t *d_status, hipStream_t s)
{
	const size_t kl = T.is448 ? 57 : 32, hl = 2 * kl;
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	if (stage_need(ctx, ES_A, chunk * kl) || stage_need(ctx, ES_AWIDE, chunk * hl)) {
		return -1;
	}
	const int alg = T.is448 ? eced::EDDSA448 : eced::EDDSA25519;   // the key expansion is the family's (sig/eddsa.c:650-671)
	eced::Dom dom;
	eced::dom_build(eced::EDDSA25519, nullptr, 0, &dom);
	for (uint32_t off = 0; off < n; off += chunk) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		EcamdEddsaSignArgs E;
		eddsa_front_args(&E, dom);
		E.n = m;
		E.sk = d_sk + off * kl;
		E.a = ctx->stage[ES_A];
		E.a_wide = ctx->stage[ES_AWIDE];
		HIPCHK(ecamd_launch_eddsa_expand(alg, E, s));
		if (eddsa_sign_R_dev_locked(ctx, cv, T, m, ctx->stage[ES_AWIDE], d_pub_out + off * kl, d_status + off, s)) {
			return -1;
		}
	}
	return 0;
}

// the call-level checks every message-level EdDSA call shares (alg, its handle, the context); fills T and dom
static int eddsa_alg_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, const uint8_t *adata, uint32_t adata_len,
			     EcamdEdSignArgs *T, eced::Dom *dom)
{
	if (!eced::alg_ok(alg)) {
		return fail(std::string(fn) + ": alg must be EDDSA25519 (9), EDDSA25519CTX (10), EDDSA25519PH (11), EDDSA448 (12) or EDDSA448PH (13)");
	}
	if (!ctx) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (eddsa_sign_setup(fn, ctx, cv, 0, nullptr, nullptr, nullptr, T)) {
		return -1;
	}
	if (eced::alg_is448(alg) != (T->is448 != 0)) {
		return fail(std::string(fn) + ": EDDSA25519 / CTX / PH run on the WEI25519 handle, EDDSA448 / PH on the WEI448 handle");
	}
	if (eced::alg_takes_dom(alg)) {
		if (alg == eced::EDDSA25519CTX && !adata) {
			return fail(std::string(fn) + ": EDDSA25519CTX needs a context (sig/eddsa.c:1683)");
		}
		if (adata_len > (uint32_t)eced::MAX_ADATA) {
			return fail(std::string(fn) + ": adata_len must be at most 255 (sig/eddsa.c:64)");
		}
	}
	eced::dom_build(alg, adata, adata_len, dom);
	return 0;
}

// the call-level checks of ec_eddsa_sign_msg_batch[_dev]; fills T and dom
static int eddsa_msg_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const void *sk, const uint8_t *adata,
			     uint32_t adata_len, const void *slots, uint32_t stride, const void *sigs, const void *status, EcamdEdSignArgs *T,
			     eced::Dom *dom)
{
	if (eddsa_alg_args_ok(fn, ctx, cv, alg, adata, adata_len, T, dom)) {
		return -1;
	}
	if (stride < 4 || (stride & 3u) || stride > 4096) {
		return fail(std::string(fn) + ": msg_stride must be a multiple of 4 in 4 .. 4096");
	}
	if (n && (!sk || !slots || !sigs || !status)) {
		return fail(std::string(fn) + ": bad argument");
	}
	return 0;
}

extern "C" int ec_eddsa_sign_msg_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const void *d_secret_keys,
					   const void *d_pubkeys, const uint8_t *adata, uint32_t adata_len, const void *d_msg_slots,
					   uint32_t msg_stride, void *d_sigs, void *d_pub_out, void *d_status, void *hip_stream)
{
	if (!ctx) {
		return fail("ec_eddsa_sign_msg_batch_dev: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	EcamdEdSignArgs T;
	eced::Dom dom;
	if (eddsa_msg_args_ok("ec_eddsa_sign_msg_batch_dev", ctx, cv, alg, n, d_secret_keys, adata, adata_len, d_msg_slots, msg_stride, d_sigs, d_status,
			      &T, &dom)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
	StreamScope scope(ctx, s);
	return eddsa_sign_msg_dev_locked(ctx, cv, T, alg, dom, n, (const uint8_t *)d_secret_keys, (const uint8_t *)d_pubkeys, (const uint8_t *)d_msg_slots,
					 msg_stride, (uint8_t *)d_sigs, (uint8_t *)d_pub_out, (uint8_t *)d_status, s);
}

extern "C" int ec_eddsa_sign_msg_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *secret_keys,
				       const uint8_t *pubkeys, const uint8_t *adata, uint32_t adata_len, const uint8_t *msg_slots,
				       uint32_t msg_stride, uint8_t *sigs, uint8_t *pub_out, uint8_t *status)
{
	if (!ctx) {
		return fail("ec_eddsa_sign_msg_batch: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	EcamdEdSignArgs T;
	eced::Dom dom;
	if (eddsa_msg_args_ok("ec_eddsa_sign_msg_batch", ctx, cv, alg, n, secret_keys, adata, adata_len, msg_slots, msg_stride, sigs, status, &T, &dom)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	const size_t kl = T.is448 ? 57 : 32;
	// the optional arrays keep their places: an array with neither pointer is neither copied nor read
	const std::vector<HostArr> arrs = {{secret_keys, nullptr, kl}, {pubkeys, nullptr, pubkeys ? kl : 0}, {msg_slots, nullptr, msg_stride},
					   {nullptr, sigs, 2 * kl},    {nullptr, pub_out, pub_out ? kl : 0}, {nullptr, status, 1}};
	return host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return eddsa_sign_msg_dev_locked(ctx, cv, T, alg, dom, m, ip[0], ip[1], ip[2], msg_stride, op[3], op[4], op[5], s);
	});
}

extern "C" int ec_eddsa_pub_key_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *d_secret_keys, void *d_pub_out,
					  void *d_status, void *hip_stream)
{
	if (!ctx) {
		return fail("ec_eddsa_pub_key_batch_dev: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	EcamdEdSignArgs T;
	if (eddsa_sign_setup("ec_eddsa_pub_key_batch_dev", ctx, cv, n, d_secret_keys, d_pub_out, d_status, &T)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
	StreamScope scope(ctx, s);
	return eddsa_pub_key_dev_locked(ctx, cv, T, n, (const uint8_t *)d_secret_keys, (uint8_t *)d_pub_out, (uint8_t *)d_status, s);
}

extern "C" int ec_eddsa_pub_key_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *secret_keys, uint8_t *pub_out,
				      uint8_t *status)
{
	if (!ctx) {
		return fail("ec_eddsa_pub_key_batch: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	EcamdEdSignArgs T;
	if (eddsa_sign_setup("ec_eddsa_pub_key_batch", ctx, cv, n, secret_keys, pub_out, status, &T)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	const size_t kl = T.is448 ? 57 : 32;
	const std::vector<HostArr> arrs = {{secret_keys, nullptr, kl}, {nullptr, pub_out, kl}, {nullptr, status, 1}};
	return host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return eddsa_pub_key_dev_locked(ctx, cv, T, m, ip[0], op[1], op[2], s);
	});
}

// ------------------------------------------------------------------------------------------
// EdDSA from the ragged message array (include/libecc_amd.h: ec_eddsa_verify_msgs_batch, ec_eddsa_verify_msgs_all_batch,
// ec_eddsa_sign_msgs_batch; ecamd_eddsa_msgs.hip).  The kernels validate every item against the array's length themselves, so the
// _dev forms only enqueue, per chunk of at most max_chunk items:
//   verify      k_eddsa_vhram_msgs: hram into ST_DIGESTS, the unusable items into DM_BAD; eddsa_verify_dev_locked /
//               eddsa448_verify_dev_locked unchanged; k_reject_where: DM_BAD's items are result 1
//   verify all  k_eddsa_vhram_msgs over the whole batch: hram into EB_HRAM, DM_BAD (n octets and one more for the verdict);
//               eddsa_verify_all_dev_locked unchanged, its verdict into DM_BAD[n]; k_eddsa_msgs_all_fin: the bit
//   sign        eddsa_sign_msg_dev_locked with k_eddsa_expand_r_msgs / k_eddsa_hram_msgs in place of the slot kernels
// The host forms stage pieces through msgs_host_call (ecamd_host_sigfam.cpp).  It takes ctx->mu itself: the checks, which run the
// curve's one-time setup, take and drop the lock first.
// ------------------------------------------------------------------------------------------
static int eddsa_msgs_checks(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int alg, const uint8_t *adata, uint32_t adata_len,
			     EcamdEdSignArgs *T, eced::Dom *dom)
{
	if (!ctx) {
		return fail(std::string(fn) + ": bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);
	return eddsa_alg_args_ok(fn, ctx, cv, alg, adata, adata_len, T, dom);   // (runs the handle's one-time setup: the verification cores need it too)
}

static int eddsa_vhram_msgs_launch(int alg, const eced::Dom &dom, uint32_t m, const uint8_t *d_pub, const uint8_t *d_sig, const EdRagged &rg,
				   uint32_t off, uint8_t *d_hram, uint8_t *d_bad, hipStream_t s)
{
	EcamdEddsaMsgsArgs M;
	eddsa_front_args(&M.e, dom);
	M.e.n = m;
	M.e.A = d_pub;
	M.e.hram = d_hram;
	M.e.bad = d_bad;
	M.vsigs = d_sig;
	M.msgs = rg.d_msgs;
	M.msgs_len = rg.msgs_len;
	M.offsets = rg.d_offsets + off;
	HIPCHK(ecamd_launch_eddsa_vhram_msgs(alg, M, s));
	return 0;
}

static int eddsa_verify_msgs_dev_locked(ecamd_ctx *ctx, ecamd_curve *cv, int alg, const eced::Dom &dom, uint32_t n, const uint8_t *d_pub,
					const uint8_t *d_sig, const EdRagged &rg, uint8_t *d_res, hipStream_t s)
{
	const bool e448 = eced::alg_is448(alg);
	const size_t kl = e448 ? 57 : 32, hl = 2 * kl;
	const uint32_t chunk = chunk_items(ctx, n);
	if (stage_need(ctx, {{ST_DIGESTS, (size_t)chunk * hl}, {DM_BAD, chunk}})) {
		return -1;
	}
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		uint8_t **S = ctx->stage;   // (read per chunk: the cores below grow their own frames)
		if (eddsa_vhram_msgs_launch(alg, dom, m, d_pub + off * kl, d_sig + off * 2 * kl, rg, off, S[ST_DIGESTS], S[DM_BAD], s)) {
			return -1;
		}
		if (e448 ? eddsa448_verify_dev_locked(ctx, cv, m, d_pub + off * kl, d_sig + off * 2 * kl, S[ST_DIGESTS], d_res + off, s)
			 : eddsa_verify_dev_locked(ctx, cv, m, d_pub + off * kl, d_sig + off * 2 * kl, S[ST_DIGESTS], 64, d_res + off, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_reject_where(d_res + off, S[DM_BAD], m, s));
		return 0;
	});
}

extern "C" int ec_eddsa_verify_msgs_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const void *d_pubkeys, const void *d_sigs,
					      const uint8_t *adata, uint32_t adata_len, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
					      void *d_result, void *hip_stream)
{
	const char *fn = "ec_eddsa_verify_msgs_batch_dev";
	EcamdEdSignArgs T;
	eced::Dom dom;
	if (eddsa_msgs_checks(fn, ctx, cv, alg, adata, adata_len, &T, &dom)) {
		return -1;
	}
	if (n && (!d_pubkeys || !d_sigs || !d_offsets || !d_result)) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (msgs_dev_ptr_ok(fn, d_msgs, msgs_len, d_offsets)) {
		return -1;
	}
	const EdRagged rg = {(const uint8_t *)d_msgs, msgs_len, (const uint64_t *)d_offsets};
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return eddsa_verify_msgs_dev_locked(ctx, const_cast<ecamd_curve *>(cv), alg, dom, n, (const uint8_t *)d_pubkeys, (const uint8_t *)d_sigs, rg,
						    (uint8_t *)d_result, s);
	});
}

extern "C" int ec_eddsa_verify_msgs_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
					  const uint8_t *adata, uint32_t adata_len, const uint8_t *msgs, const uint64_t *offsets, uint8_t *result)
{
	const char *fn = "ec_eddsa_verify_msgs_batch";
	EcamdEdSignArgs T;
	eced::Dom dom;
	if (eddsa_msgs_checks(fn, ctx, cv, alg, adata, adata_len, &T, &dom)) {
		return -1;
	}
	if (n && (!pubkeys || !sigs || !offsets || !result)) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t kl = T.is448 ? 57 : 32;
	const std::vector<MsgsArr> arrs = {{pubkeys, nullptr, kl, kl}, {sigs, nullptr, 2 * kl, 2 * kl}, {nullptr, result, 1, 1}};
	return msgs_host_call(fn, ctx, n, msgs, offsets, arrs,
			      [&](uint32_t m, const uint8_t *d_msgs, uint64_t len, const uint64_t *d_offs, const DevIn &ip, const DevOut &op, hipStream_t s) {
		const EdRagged rg = {d_msgs, len, d_offs};
		return eddsa_verify_msgs_dev_locked(ctx, const_cast<ecamd_curve *>(cv), alg, dom, m, ip[0], ip[1], rg, op[2], s);
	});
}

static int eddsa_msgs_all_available(const char *fn, ecamd_curve *cv, uint32_t n)
{
	if (n == 0 || (cv->pbits == 448 ? !eddsa448_msm_available(cv) : !eddsa_msm_available(cv))) {
		return fail(std::string(fn) + ": needs n > 0 and Ed25519 (the WEI25519 handle on the 2^255 - 19 unit) or Ed448 (WEI448 on the Goldilocks unit)");
	}
	return 0;
}

static int eddsa_verify_msgs_all_batch_dev_impl(ecamd_ctx *ctx, const ecamd_curve *cv_in, int alg, uint32_t n, const void *d_pubkeys, const void *d_sigs,
						const uint8_t *adata, uint32_t adata_len, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
						void *d_all_valid, void *hip_stream)
{
	const char *fn = "ec_eddsa_verify_msgs_all_batch_dev";
	EcamdEdSignArgs T;
	eced::Dom dom;
	if (eddsa_msgs_checks(fn, ctx, cv_in, alg, adata, adata_len, &T, &dom)) {
		return -1;
	}
	if (!d_pubkeys || !d_sigs || !d_offsets || !d_all_valid) {
		return fail(std::string(fn) + ": bad argument");
	}
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	if (eddsa_msgs_all_available(fn, cv, n) || msgs_dev_ptr_ok(fn, d_msgs, msgs_len, d_offsets)) {
		return -1;
	}
	const EdRagged rg = {(const uint8_t *)d_msgs, msgs_len, (const uint64_t *)d_offsets};
	const size_t kl = T.is448 ? 57 : 32, hl = 2 * kl;
	return dev_call(ctx, hip_stream, [&](hipStream_t s) -> int {
		uint8_t seed[32];
		if (msm_seed(ctx, seed) || stage_need(ctx, {{EB_HRAM, (size_t)n * hl}, {DM_BAD, (size_t)n + 1}})) {
			return -1;
		}
		uint8_t *d_hram = ctx->stage[EB_HRAM], *d_bad = ctx->stage[DM_BAD];
		if (for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			    return eddsa_vhram_msgs_launch(alg, dom, m, (const uint8_t *)d_pubkeys + off * kl, (const uint8_t *)d_sigs + off * 2 * kl, rg, off,
							   d_hram + off * hl, d_bad + off, s);
		    }) ||
		    eddsa_verify_all_dev_locked(ctx, cv, n, d_pubkeys, d_sigs, d_hram, seed, d_bad + n, s)) {
			return -1;
		}
		HIPCHK(ecamd_launch_eddsa_msgs_all_fin(d_bad, n + 1, (uint8_t *)d_all_valid, s));
		return 0;
	});
}

extern "C" int ec_eddsa_verify_msgs_all_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const void *d_pubkeys, const void *d_sigs,
						  const uint8_t *adata, uint32_t adata_len, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
						  void *d_all_valid, void *hip_stream)
{
	const int r = eddsa_verify_msgs_all_batch_dev_impl(ctx, cv, alg, n, d_pubkeys, d_sigs, adata, adata_len, d_msgs, msgs_len, d_offsets, d_all_valid,
							   hip_stream);
	msm_seed_discard(ctx);
	return r;
}

extern "C" int ec_eddsa_verify_msgs_all_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
					      const uint8_t *adata, uint32_t adata_len, const uint8_t *msgs, const uint64_t *offsets, int *all_valid,
					      uint32_t *first_rejected)
{
	const char *fn = "ec_eddsa_verify_msgs_all_batch";
	EcamdEdSignArgs T;
	eced::Dom dom;
	if (eddsa_msgs_checks(fn, ctx, cv, alg, adata, adata_len, &T, &dom)) {
		msm_seed_discard(ctx);
		return -1;
	}
	if (n == 0 || !pubkeys || !sigs || !offsets || !all_valid) {
		msm_seed_discard(ctx);
		return fail(std::string(fn) + ": bad argument (the reference rejects num = 0 too)");
	}
	*all_valid = 0;
	if (first_rejected) {
		*first_rejected = n;
	}
	// the hram launch piece by piece, its output back on the host: what ec_eddsa_verify_all_batch takes
	const size_t kl = T.is448 ? 57 : 32, hl = 2 * kl;
	std::vector<uint8_t> hram((size_t)n * hl), bad(n);
	const std::vector<MsgsArr> arrs = {{pubkeys, nullptr, kl, kl}, {sigs, nullptr, 2 * kl, 2 * kl}, {nullptr, hram.data(), hl, hl}, {nullptr, bad.data(), 1, 1}};
	if (msgs_host_call(fn, ctx, n, msgs, offsets, arrs,
			   [&](uint32_t m, const uint8_t *d_msgs, uint64_t len, const uint64_t *d_offs, const DevIn &ip, const DevOut &op, hipStream_t s) {
		const EdRagged rg = {d_msgs, len, d_offs};
		return eddsa_vhram_msgs_launch(alg, dom, m, ip[0], ip[1], rg, 0, op[2], op[3], s);
	})) {
		msm_seed_discard(ctx);
		return -1;
	}
	uint32_t first_bad = 0;
	while (first_bad < n && bad[first_bad] == 0) {
		first_bad++;
	}
	int ok = 0;
	uint32_t first = n;
	if (ec_eddsa_verify_all_batch(ctx, cv, n, pubkeys, sigs, hram.data(), (uint32_t)hl, &ok, &first)) {   // (discards the seed itself)
		return -1;
	}
	*all_valid = (ok && first_bad == n) ? 1 : 0;
	if (first_rejected) {
		*first_rejected = first < first_bad ? first : first_bad;
	}
	return 0;
}

extern "C" int ec_eddsa_sign_msgs_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const void *d_secret_keys, const void *d_pubkeys,
					    const uint8_t *adata, uint32_t adata_len, const void *d_msgs, uint64_t msgs_len, const void *d_offsets,
					    void *d_sigs, void *d_pub_out, void *d_status, void *hip_stream)
{
	const char *fn = "ec_eddsa_sign_msgs_batch_dev";
	EcamdEdSignArgs T;
	eced::Dom dom;
	if (eddsa_msgs_checks(fn, ctx, cv, alg, adata, adata_len, &T, &dom)) {
		return -1;
	}
	if (n && (!d_secret_keys || !d_offsets || !d_sigs || !d_status)) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	if (msgs_dev_ptr_ok(fn, d_msgs, msgs_len, d_offsets)) {
		return -1;
	}
	const EdRagged rg = {(const uint8_t *)d_msgs, msgs_len, (const uint64_t *)d_offsets};
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return eddsa_sign_msg_dev_locked(ctx, cv, T, alg, dom, n, (const uint8_t *)d_secret_keys, (const uint8_t *)d_pubkeys, nullptr, 0, (uint8_t *)d_sigs,
						 (uint8_t *)d_pub_out, (uint8_t *)d_status, s, &rg);
	});
}

extern "C" int ec_eddsa_sign_msgs_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *secret_keys, const uint8_t *pubkeys,
					const uint8_t *adata, uint32_t adata_len, const uint8_t *msgs, const uint64_t *offsets, uint8_t *sigs,
					uint8_t *pub_out, uint8_t *status)
{
	const char *fn = "ec_eddsa_sign_msgs_batch";
	EcamdEdSignArgs T;
	eced::Dom dom;
	if (eddsa_msgs_checks(fn, ctx, cv, alg, adata, adata_len, &T, &dom)) {
		return -1;
	}
	if (n && (!secret_keys || !offsets || !sigs || !status)) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t kl = T.is448 ? 57 : 32;
	// the optional arrays keep their places: an array with neither pointer is neither copied nor read
	const std::vector<MsgsArr> arrs = {{secret_keys, nullptr, kl, kl}, {pubkeys, nullptr, pubkeys ? kl : 0, pubkeys ? kl : 0}, {nullptr, sigs, 2 * kl, 2 * kl},
					   {nullptr, pub_out, pub_out ? kl : 0, pub_out ? kl : 0}, {nullptr, status, 1, 1}};
	return msgs_host_call(fn, ctx, n, msgs, offsets, arrs,
			      [&](uint32_t m, const uint8_t *d_msgs, uint64_t len, const uint64_t *d_offs, const DevIn &ip, const DevOut &op, hipStream_t s) {
		const EdRagged rg = {d_msgs, len, d_offs};
		return eddsa_sign_msg_dev_locked(ctx, cv, T, alg, dom, m, ip[0], ip[1], nullptr, 0, op[2], op[3], op[4], s, &rg);
	});
}
