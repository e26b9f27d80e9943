// libecc_amd/csrc/ecamd_host.cpp -- host side of the C ABI declared in include/libecc_amd.h.
//
// What lives here (and mirrors in the reference, paths relative to /root/reference/src):
//   * the built-in curve table and import_params (curves/ec_params.c:24-194): domain parameters
//     -> Montgomery constants R, R^2, -p^-1, a*R, b*R, 3b*R, p-2 (derivations as in
//     scripts/expand_libecc.py:62-71, but for our radix 2^(32*NW)), uploaded to __constant__;
//   * batch plumbing: staging buffers, per-lane window-table scratch, chunking, streams.
// No arithmetic of the hot path runs on the host and there is no CPU fallback: every entry
// point needs a live HIP device.
#include "ecamd_host_internal.h"
#include "ecamd_rfc6979.h"

using namespace ecamd_host;

// ------------------------------------------------------------------------------------------
// error reporting
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int ecamd_host::fail(const std::string &m)
{
	g_err = m;
	return -1;
}

extern "C" const char *ecamd_last_error(void) { return g_err.c_str(); }
// for the other translation units of the library (ecamd_multi.cpp): not part of the public ABI
__attribute__((visibility("default"))) void ecamd_set_error(const char *msg) { g_err = msg ? msg : ""; }

// ------------------------------------------------------------------------------------------
// small host big integers (little-endian 32-bit words); only used to derive constants
// ------------------------------------------------------------------------------------------

void ecamd_host::big_trim(Big &a)
{
	while (a.size() > 1 && a.back() == 0) {
		a.pop_back();
	}
	if (a.empty()) {
		a.push_back(0);
	}
}
Big ecamd_host::big_from_be(const uint8_t *b, size_t len)
{
	Big r((len + 3) / 4 + 1, 0);
	for (size_t i = 0; i < len; i++) {
		size_t pos = len - 1 - i;
		r[pos / 4] |= (uint32_t)b[i] << (8 * (pos % 4));
	}
	big_trim(r);
	return r;
}
static Big big_from_hex(const char *h)
{
	size_t n = strlen(h);
	Big r(n / 8 + 2, 0);
	for (size_t i = 0; i < n; i++) {
		char c = h[n - 1 - i];
		uint32_t v = (c >= '0' && c <= '9') ? (uint32_t)(c - '0')
			     : (c >= 'a' && c <= 'f') ? (uint32_t)(c - 'a' + 10) : (uint32_t)(c - 'A' + 10);
		r[i / 8] |= v << (4 * (i % 8));
	}
	big_trim(r);
	return r;
}
int ecamd_host::big_cmp(const Big &a, const Big &b)
{
	size_t n = a.size() > b.size() ? a.size() : b.size();
	for (size_t i = n; i-- > 0;) {
		uint32_t x = i < a.size() ? a[i] : 0, y = i < b.size() ? b[i] : 0;
		if (x != y) {
			return x < y ? -1 : 1;
		}
	}
	return 0;
}
int ecamd_host::big_bitlen(const Big &a)
{
	for (size_t i = a.size(); i-- > 0;) {
		if (a[i]) {
			int b = 31;
			while (!((a[i] >> b) & 1)) {
				b--;
			}
			return (int)i * 32 + b + 1;
		}
	}
	return 0;
}
Big ecamd_host::big_add(const Big &a, const Big &b)
{
	size_t n = (a.size() > b.size() ? a.size() : b.size()) + 1;
	Big r(n, 0);
	uint64_t c = 0;
	for (size_t i = 0; i < n; i++) {
		c += (uint64_t)(i < a.size() ? a[i] : 0) + (i < b.size() ? b[i] : 0);
		r[i] = (uint32_t)c;
		c >>= 32;
	}
	big_trim(r);
	return r;
}
Big ecamd_host::big_sub(const Big &a, const Big &b)  // a >= b
{
	Big r(a.size(), 0);
	int64_t c = 0;
	for (size_t i = 0; i < a.size(); i++) {
		int64_t x = (int64_t)a[i] - (i < b.size() ? b[i] : 0) + c;
		r[i] = (uint32_t)x;
		c = x >> 32;
	}
	big_trim(r);
	return r;
}
Big ecamd_host::big_mul(const Big &a, const Big &b)
{
	Big r(a.size() + b.size() + 1, 0);
	for (size_t i = 0; i < a.size(); i++) {
		uint64_t c = 0;
		for (size_t j = 0; j < b.size(); j++) {
			c += (uint64_t)a[i] * b[j] + r[i + j];
			r[i + j] = (uint32_t)c;
			c >>= 32;
		}
		r[i + b.size()] += (uint32_t)c;
	}
	big_trim(r);
	return r;
}
Big ecamd_host::big_mod(const Big &a, const Big &m)  // bitwise shift-subtract; sizes are tiny
{
	Big r(1, 0);
	for (int bit = big_bitlen(a) - 1; bit >= 0; bit--) {
		// r = 2r + bit
		Big t(r.size() + 1, 0);
		for (size_t i = 0; i < r.size(); i++) {
			t[i] |= r[i] << 1;
			t[i + 1] |= r[i] >> 31;
		}
		t[0] |= (a[(size_t)bit / 32] >> (bit % 32)) & 1u;
		big_trim(t);
		r = (big_cmp(t, m) >= 0) ? big_sub(t, m) : t;
	}
	return r;
}
Big ecamd_host::big_pow2(int e)
{
	Big r((size_t)e / 32 + 1, 0);
	r[(size_t)e / 32] = 1u << (e % 32);
	return r;
}
Big ecamd_host::big_mulmod(const Big &a, const Big &b, const Big &m) { return big_mod(big_mul(a, b), m); }
Big ecamd_host::big_powmod(const Big &a, const Big &e, const Big &m)
{
	Big r(1, 1), base = big_mod(a, m);
	for (int i = big_bitlen(e) - 1; i >= 0; i--) {
		r = big_mulmod(r, r, m);
		if ((e[(size_t)i / 32] >> (i % 32)) & 1u) {
			r = big_mulmod(r, base, m);
		}
	}
	return r;
}
void ecamd_host::big_store(uint32_t *dst, int nw, const Big &a)
{
	for (int i = 0; i < nw; i++) {
		dst[i] = (size_t)i < a.size() ? a[(size_t)i] : 0;
	}
}
void ecamd_host::big_to_be(uint8_t *dst, int len, const Big &a)
{
	for (int i = 0; i < len; i++) {
		int pos = len - 1 - i;
		dst[i] = ((size_t)pos / 4 < a.size()) ? (uint8_t)(a[(size_t)pos / 4] >> (8 * (pos % 4))) : 0;
	}
}

// ------------------------------------------------------------------------------------------
// curve table (domain parameters only; generated by tools/gen_curve_table.py)
// ------------------------------------------------------------------------------------------
struct CurveRow {
	const char *name;
	int type;
	const char *p, *a, *b, *order, *gx, *gy, *q, *h;
};
static const CurveRow g_curve_rows[] = {
#include "ecamd_curve_table.inc"
};


static const int k_widths[] = {6, 7, 8, 10, 12, 14, 16, 17};

static int pick_nw(int pbits)
{
	for (int w : k_widths) {
		if (32 * w >= pbits) {
			return w;
		}
	}
	return 0;
}

extern "C" int ecamd_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) {
		return 0;
	}
	return n;
}

extern "C" int ecamd_ctx_create(ecamd_ctx **out, int device)
{
	if (!out) {
		return fail("ecamd_ctx_create: NULL out pointer");
	}
	*out = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) {
		return fail("ecamd_ctx_create: no HIP device available (this library has no CPU fallback)");
	}
	if (device < 0 || device >= n) {
		return fail("ecamd_ctx_create: device index out of range");
	}
	HIPCHK(hipSetDevice(device));
	ecamd_ctx *c = new ecamd_ctx();
	c->device = device;
	c->max_chunk = 1u << 20;
	{
		// fixed-base comb tables: built on the first fixed-base batch of at least this many items
		// (ECAMD_COMB_MIN_BATCH, default 4096; ECAMD_NO_COMB disables them)
		const char *e = getenv("ECAMD_COMB_MIN_BATCH");
		c->comb_min_batch = e ? (uint32_t)strtoul(e, nullptr, 10) : 4096u;
		if (getenv("ECAMD_NO_COMB") != nullptr) {
			c->comb_min_batch = 0;
		}
	}
	c->tbl = nullptr;
	c->tbl_bytes = 0;
	c->tbl_fast = nullptr;
	c->tbl_fast_bytes = 0;
	for (int i = 0; i < ECAMD_NSTAGE; i++) {
		c->stage[i] = nullptr;
		c->stage_bytes[i] = 0;
	}
	c->prep_scratch = nullptr;
	c->prep_scratch_bytes = 0;
	c->last_stream = nullptr;
	c->inflight = false;
	if (hipEventCreateWithFlags(&c->busy, hipEventDisableTiming) != hipSuccess) {
		delete c;
		return fail("ecamd_ctx_create: hipEventCreate failed");
	}
	c->timing = false;
	c->secret_scalars = false;
	c->eddsa_msm = 1;
	c->msm_min = 1u << 17;   // measured break-even: 1.16x at 2^17, 0.92x at 2^16 (profiles/r2l_eddsa_msm.json)
	c->msm_k = 0;
	{
		const char *e = getenv("ECAMD_MSM_MIN");
		if (e) {
			c->msm_min = (uint32_t)strtoul(e, nullptr, 10);
		}
		e = getenv("ECAMD_MSM_K");
		if (e) {
			c->msm_k = (uint32_t)strtoul(e, nullptr, 10);
		}
	}
	c->msm = nullptr;
	c->msm_bytes = 0;
	c->msm_seed_valid = false;
	c->ev_valid = false;
	c->ev_dom_valid = false;
	for (int i = 0; i <= ECAMD_NTIMED; i++) {
		if (hipEventCreate(&c->ev[i]) != hipSuccess) {
			delete c;
			return fail("ecamd_ctx_create: hipEventCreate failed");
		}
	}
	if (hipEventCreate(&c->ev_dom[0]) != hipSuccess || hipEventCreate(&c->ev_dom[1]) != hipSuccess) {
		delete c;
		return fail("ecamd_ctx_create: hipEventCreate failed");
	}
	memset(c->hbuf, 0, sizeof(c->hbuf));
	memset(c->hbuf_bytes, 0, sizeof(c->hbuf_bytes));
	{
		const char *e = getenv("ECAMD_HOST_CHUNK");
		// (round 4: 2^19 -- a 2^18-item launch runs the window kernels at 0.92 of their 2^20 rate, a 2^19-item one at 0.97,
		// and two pieces of a 2^20 batch still overlap the second's copy with the first's kernels; profiles/r4_batch_sweep.md)
		c->host_chunk = e ? (uint32_t)strtoul(e, nullptr, 10) : (1u << 19);
		if (c->host_chunk == 0) {
			c->host_chunk = 1u << 19;
		}
		e = getenv("ECAMD_HOST_RAMP_MIN");
		c->host_first_min = e ? (uint32_t)strtoul(e, nullptr, 10) : (1u << 16);
		if (c->host_first_min == 0) {
			c->host_first_min = 1u << 16;
		}
	}
	if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
	    hipEventCreateWithFlags(&c->in_ready[0], hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->in_ready[1], hipEventDisableTiming) != hipSuccess) {
		delete c;
		return fail("ecamd_ctx_create: copy stream creation failed");
	}
	if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
		delete c;
		return fail("ecamd_ctx_create: hipStreamCreate failed");
	}
	if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side_fork, hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side_done, hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side_mid, hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side_aux, hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side_hi, hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side_red, hipEventDisableTiming) != hipSuccess ||
	    hipStreamCreateWithFlags(&c->side2_stream, hipStreamNonBlocking) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side2_fork, hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side2_done, hipEventDisableTiming) != hipSuccess) {
		delete c;
		return fail("ecamd_ctx_create: side stream creation failed");
	}
	c->side_ok = getenv("ECAMD_NO_SIDE_STREAM") == nullptr;
	c->side2_ok = c->side_ok;
	*out = c;
	return 0;
}

extern "C" void ecamd_ctx_destroy(ecamd_ctx *c)
{
	if (!c) {
		return;
	}
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	if (c->tbl) {
		(void)hipFree(c->tbl);
	}
	if (c->tbl_fast) {
		(void)hipFree(c->tbl_fast);
	}
	if (c->msm) {
		(void)hipFree(c->msm);
	}
	for (int i = 0; i < ECAMD_NSTAGE; i++) {
		if (c->stage[i]) {
			(void)hipFree(c->stage[i]);
		}
	}
	if (c->prep_scratch) {
		(void)hipFree(c->prep_scratch);
	}
	for (int i = 0; i <= ECAMD_NTIMED; i++) {
		(void)hipEventDestroy(c->ev[i]);
	}
	(void)hipEventDestroy(c->ev_dom[0]);
	(void)hipEventDestroy(c->ev_dom[1]);
	(void)hipStreamDestroy(c->stream);
	(void)hipStreamDestroy(c->copy_stream);
	(void)hipStreamSynchronize(c->side_stream);
	(void)hipStreamDestroy(c->side_stream);
	(void)hipEventDestroy(c->side_fork);
	(void)hipEventDestroy(c->side_done);
	(void)hipEventDestroy(c->side_mid);
	(void)hipEventDestroy(c->side_aux);
	(void)hipEventDestroy(c->side_hi);
	(void)hipEventDestroy(c->side_red);
	(void)hipStreamSynchronize(c->side2_stream);
	(void)hipStreamDestroy(c->side2_stream);
	(void)hipEventDestroy(c->side2_fork);
	(void)hipEventDestroy(c->side2_done);
	(void)hipEventDestroy(c->in_ready[0]);
	(void)hipEventDestroy(c->in_ready[1]);
	(void)hipEventDestroy(c->busy);
	for (int b = 0; b < 2; b++) {
		for (int k = 0; k < 6; k++) {
			if (c->hbuf[b][k]) {
				(void)hipFree(c->hbuf[b][k]);
			}
		}
	}
	delete c;
}

extern "C" int ecamd_ctx_set_max_chunk(ecamd_ctx *c, uint32_t max_items)
{
	if (!c || max_items == 0) {
		return fail("ecamd_ctx_set_max_chunk: bad argument");
	}
	c->max_chunk = max_items;
	return 0;
}

extern "C" int ecamd_ctx_set_eddsa_msm(ecamd_ctx *c, int mode, uint32_t min_items, uint32_t items_per_lane)
{
	if (!c || mode < 0 || mode > 2 || items_per_lane > 64) {
		return fail("ecamd_ctx_set_eddsa_msm: bad argument");
	}
	std::lock_guard<std::mutex> lk(c->mu);
	c->eddsa_msm = mode;
	if (min_items) {
		c->msm_min = min_items;
	}
	c->msm_k = items_per_lane;
	return 0;
}

// The z_i of the next ec_eddsa_verify_all_batch[_dev] call on this context are ChaCha20(seed, item index) instead of being keyed
// by getrandom: an application that owns the randomness source of its libecc (get_random) keys the batch equation with it.
// Used once; the bytes are wiped when consumed.
extern "C" int ecamd_ctx_set_msm_seed(ecamd_ctx *c, const uint8_t seed[32])
{
	if (!c || !seed) {
		return fail("ecamd_ctx_set_msm_seed: bad argument");
	}
	std::lock_guard<std::mutex> lk(c->mu);
	memcpy(c->msm_seed_bytes, seed, 32);
	c->msm_seed_valid = true;
	return 0;
}

// Drops a seed that is still pending (ecamd_multi_*_verify_all_batch: a rank whose shard was empty never consumed its copy).
extern "C" int ecamd_ctx_discard_msm_seed(ecamd_ctx *c)
{
	if (!c) {
		return fail("ecamd_ctx_discard_msm_seed: NULL context");
	}
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->msm_seed_valid) {
		memset(c->msm_seed_bytes, 0, sizeof(c->msm_seed_bytes));
		c->msm_seed_valid = false;
	}
	return 0;
}

extern "C" int ecamd_ctx_set_secret_scalars(ecamd_ctx *c, int on)
{
	if (!c) {
		return fail("ecamd_ctx_set_secret_scalars: NULL context");
	}
	std::lock_guard<std::mutex> lk(c->mu);
	c->secret_scalars = on != 0;
	return 0;
}

extern "C" int ecamd_ctx_enable_kernel_timing(ecamd_ctx *c, int on)
{
	if (!c) {
		return fail("ecamd_ctx_enable_kernel_timing: NULL context");
	}
	std::lock_guard<std::mutex> lk(c->mu);
	c->timing = on != 0;
	c->ev_valid = false;
	c->ev_dom_valid = false;
	return 0;
}

extern "C" int ecamd_ctx_kernel_times(ecamd_ctx *c, double *ms, int n)
{
	if (!c || !ms || n < ECAMD_NTIMED - 1) {
		return fail("ecamd_ctx_kernel_times: bad argument (need room for 4 values)");
	}
	std::lock_guard<std::mutex> lk(c->mu);
	if (!c->timing || !c->ev_valid) {
		return fail("ecamd_ctx_kernel_times: timing not enabled or no fast-path batch ran since");
	}
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipEventSynchronize(c->ev[ECAMD_NTIMED - 1]));
	for (int i = 0; i < ECAMD_NTIMED - 1; i++) {
		float f = 0.0f;
		HIPCHK(hipEventElapsedTime(&f, c->ev[i], c->ev[i + 1]));
		ms[i] = (double)f;
	}
	return 0;
}

// duration of the dominant kernel of the last protocol call made with timing enabled: k_p256_verify_loop (ECDSA verification
// on secp256r1), k_x25519_ladder / k_x448_ladder (X25519 / X448), k_ed_smul_c25519<1> (the [h]A window loop of Ed25519
// verification); the first chunk of the call
extern "C" int ecamd_ctx_dominant_kernel_ms(ecamd_ctx *c, double *ms)
{
	if (!c || !ms) {
		return fail("ecamd_ctx_dominant_kernel_ms: bad argument");
	}
	std::lock_guard<std::mutex> lk(c->mu);
	if (!c->timing || !c->ev_dom_valid) {
		return fail("ecamd_ctx_dominant_kernel_ms: timing not enabled or no protocol call with a timed kernel ran since");
	}
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipEventSynchronize(c->ev_dom[1]));
	float f = 0.0f;
	HIPCHK(hipEventElapsedTime(&f, c->ev_dom[0], c->ev_dom[1]));
	*ms = (double)f;
	return 0;
}

extern "C" void *ecamd_ctx_stream(ecamd_ctx *c) { return c ? (void *)c->stream : nullptr; }

// Page-locked host memory for the arrays handed to the host-pointer entry points: the copies to and from the device then run
// as asynchronous DMA at PCIe rate instead of going through the runtime's pageable staging.  Portable: valid for every device.
extern "C" void *ecamd_host_alloc(size_t bytes)
{
	void *p = nullptr;
	if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
		(void)hipGetLastError();
		fail("ecamd_host_alloc: hipHostMalloc failed");
		return nullptr;
	}
	return p;
}

extern "C" void ecamd_host_free(void *p)
{
	if (p) {
		(void)hipHostFree(p);
	}
}

// Zero every scratch buffer of the context (window tables, recoded scalars, staged inputs and outputs): after calls that
// worked on secret scalars nothing derived from them stays in HBM.  Enqueued behind the context's last call; synchronous.
extern "C" int ecamd_ctx_wipe_scratch(ecamd_ctx *c)
{
	if (!c) {
		return fail("ecamd_ctx_wipe_scratch: NULL context");
	}
	std::lock_guard<std::mutex> lk(c->mu);
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (c->inflight && c->last_stream != s) {
		HIPCHK(hipStreamWaitEvent(s, c->busy, 0));
	}
	HIPCHK(hipStreamSynchronize(c->copy_stream));
	if (c->tbl) {
		HIPCHK(hipMemsetAsync(c->tbl, 0, c->tbl_bytes, s));
	}
	if (c->tbl_fast) {
		HIPCHK(hipMemsetAsync(c->tbl_fast, 0, c->tbl_fast_bytes, s));
	}
	if (c->msm) {
		HIPCHK(hipMemsetAsync(c->msm, 0, c->msm_bytes, s));
	}
	for (int i = 0; i < ECAMD_NSTAGE; i++) {
		if (c->stage[i]) {
			HIPCHK(hipMemsetAsync(c->stage[i], 0, c->stage_bytes[i], s));
		}
	}
	if (c->prep_scratch) {
		HIPCHK(hipMemsetAsync(c->prep_scratch, 0, c->prep_scratch_bytes, s));
	}
	for (int b = 0; b < 2; b++) {
		for (int k = 0; k < 6; k++) {
			if (c->hbuf[b][k]) {
				HIPCHK(hipMemsetAsync(c->hbuf[b][k], 0, c->hbuf_bytes[b][k], s));
			}
		}
	}
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

extern "C" int ecamd_ctx_synchronize(ecamd_ctx *c)
{
	if (!c) {
		return fail("ecamd_ctx_synchronize: NULL context");
	}
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	return 0;
}

// Every call works in the context's shared scratch (window tables, stage[] buffers).  A call enqueued on another
// stream than the previous one therefore first makes its stream wait for the previous call's last kernel, and
// leaves an event behind its own last kernel (ctx->mu held for the lifetime of the scope).
// (the stream of the innermost scope on this thread: what ensure() orders the wipe of a growing scratch buffer behind)
static thread_local hipStream_t t_scope_stream = nullptr;
static thread_local bool t_scope_active = false;
StreamScope::StreamScope(ecamd_ctx *ctx, hipStream_t stream) : c(ctx), s(stream), outer(t_scope_stream), outer_active(t_scope_active)
{
	if (c->inflight && c->last_stream != s) {
		(void)hipStreamWaitEvent(s, c->busy, 0);
	}
	t_scope_stream = s;
	t_scope_active = true;
}
StreamScope::~StreamScope()
{
	if (hipEventRecord(c->busy, s) == hipSuccess) {
		c->last_stream = s;
		c->inflight = true;
	}
	t_scope_stream = outer;
	t_scope_active = outer_active;
}


int ecamd_host::ensure(uint8_t **buf, size_t *have, size_t need)
{
	if (*have >= need) {
		return 0;
	}
	if (*buf) {
		// a scratch buffer that has to grow may hold values derived from secret scalars (window tables, recoded or staged
		// scalars of an earlier group of the same call): it goes back to the allocator zeroed.  The wipe is ordered
		// behind the call's own stream -- everything that used the buffer was enqueued on it or is waited for by it (StreamScope, the
		// side stream's join) -- and only that stream is drained: other contexts on the device keep running (a
		// device-wide synchronisation stalled every rank of a many-contexts-per-device run on each growth).
		if (t_scope_active) {
			HIPCHK(hipMemsetAsync(*buf, 0, *have, t_scope_stream));
			HIPCHK(hipStreamSynchronize(t_scope_stream));
		} else {
			HIPCHK(hipMemset(*buf, 0, *have));
			HIPCHK(hipDeviceSynchronize());
		}
		HIPCHK(hipFree(*buf));
		*buf = nullptr;
		*have = 0;
	}
	// grow with an eighth of headroom: a sequence of slowly growing batches reallocates (and wipes, and waits) a few times, not every call
	const size_t want = need + (need >> 3);
	if (hipMalloc((void **)buf, want) == hipSuccess) {
		*have = want;
		return 0;
	}
	(void)hipGetLastError();
	HIPCHK(hipMalloc((void **)buf, need));
	*have = need;
	return 0;
}

int ecamd_host::stage_need(ecamd_ctx *ctx, std::initializer_list<StageNeed> needs)
{
	for (const StageNeed &k : needs) {
		if (ensure(&ctx->stage[k.slot], &ctx->stage_bytes[k.slot], k.bytes)) {
			return -1;
		}
	}
	return 0;
}
int ecamd_host::stage_need(ecamd_ctx *ctx, StageSlot slot, size_t bytes) { return stage_need(ctx, {{slot, bytes}}); }


// ------------------------------------------------------------------------------------------
// __constant__ curve slots.  The tables the kernels index (g_curves_<NW>[slot], g_g29_<unit>[slot]) exist once per
// DEVICE and per process, whatever the number of contexts opened on that device, so their bookkeeping is
// process-global: one registry per device under one mutex, reference-counted, and handles whose constant image is
// byte-identical share a slot (two contexts that both load SECP256R1 use the same constants; two contexts that load
// different curves of one width get different slots instead of overwriting each other).  A slot is only written
// while no live handle refers to it, so an upload never races with a kernel that reads it.
// ------------------------------------------------------------------------------------------
#define ECAMD_MAX_DEVICES 64
#define ECAMD_G29_KEYS 640  /* pbits + flavour */
struct SlotEnt {
	int ref = 0;
	std::vector<uint32_t> img;  // what the slot holds (kept after the last release: a re-acquire needs no upload)
};
struct SlotRegistry {
	SlotEnt s[18][ECAMD_MAX_SLOTS_HOST];  // [nw][slot]: saturated-word units
	SlotEnt g[ECAMD_G29_KEYS][8];         // [pbits + flavour][slot]: radix-2^29 units
};
static std::mutex g_slot_mu;
static SlotRegistry *g_slots[ECAMD_MAX_DEVICES];

// find (or fill) a slot of `row` holding `img`; returns the slot or -1 (none free) / -2 (upload failed)
template <class Upload> static int slot_acquire(SlotEnt *row, int nslots, const std::vector<uint32_t> &img, Upload upload)
{
	for (int i = 0; i < nslots; i++) {
		if (row[i].ref > 0 && row[i].img == img) {
			row[i].ref++;
			return i;
		}
	}
	int pick = -1;
	for (int i = 0; i < nslots && pick < 0; i++) {
		if (row[i].ref == 0 && row[i].img == img) {
			pick = i;  // still resident from an earlier handle
		}
	}
	bool need_upload = pick < 0;
	for (int i = 0; i < nslots && pick < 0; i++) {
		if (row[i].ref == 0 && row[i].img.empty()) {
			pick = i;
		}
	}
	for (int i = 0; i < nslots && pick < 0; i++) {
		if (row[i].ref == 0) {
			pick = i;
		}
	}
	if (pick < 0) {
		return -1;
	}
	if (need_upload) {
		row[pick].img.clear();
		if (upload(pick) != hipSuccess) {
			return -2;
		}
		row[pick].img = img;
	}
	row[pick].ref = 1;
	return pick;
}
static SlotRegistry *slot_registry(int device)
{
	if (device < 0 || device >= ECAMD_MAX_DEVICES) {
		return nullptr;
	}
	if (!g_slots[device]) {
		g_slots[device] = new SlotRegistry();
	}
	return g_slots[device];
}

// CurveK<NW> as a flat word image: p r2 one pm2 a b b3 fix64 (NW words each), then
// mpinv pbits a_is_m3 fix_is_id -- must match ecamd_field.h.  Returns the slot holding it (g_slot_mu held).
static int acquire_modulus(int device, int nw, const Big &p, const Big &a_in, const Big &b_in, int *slot_out)
{
	Big a_red = big_mod(a_in, p), b_red = big_mod(b_in, p);
	struct {
		const Big &a, &b;
		int pbits;
	} cvv = {a_red, b_red, big_bitlen(p)};
	auto *cv = &cvv;
	const Big R = big_mod(big_pow2(32 * nw), p);
	const Big R2 = big_mulmod(R, R, p);
	Big two(1, 2), three(1, 3);
	const Big pm2 = big_sub(p, two);
	const Big aR = big_mulmod(cv->a, R, p);
	const Big bR = big_mulmod(cv->b, R, p);
	const Big b3R = big_mulmod(big_mulmod(cv->b, three, p), R, p);
	// fix64 = R^2 * 2^(-64*ceil(nw/2)) mod p
	const int n64 = (nw + 1) / 2;
	const Big R64 = big_mod(big_pow2(64 * n64), p);
	const Big R64inv = big_powmod(R64, pm2, p);
	const Big fix = big_mulmod(R2, R64inv, p);
	// -p^-1 mod 2^32 by Newton iteration
	uint32_t p0 = p[0], x = 1;
	for (int i = 0; i < 5; i++) {
		x *= 2u - p0 * x;
	}
	const uint32_t mpinv = 0u - x;
	std::vector<uint32_t> img((size_t)8 * nw + 4, 0);
	big_store(&img[0 * nw], nw, p);
	big_store(&img[1 * nw], nw, R2);
	big_store(&img[2 * nw], nw, R);
	big_store(&img[3 * nw], nw, pm2);
	big_store(&img[4 * nw], nw, aR);
	big_store(&img[5 * nw], nw, bR);
	big_store(&img[6 * nw], nw, b3R);
	big_store(&img[7 * nw], nw, fix);
	img[8 * nw + 0] = mpinv;
	img[8 * nw + 1] = (uint32_t)cv->pbits;
	img[8 * nw + 2] = (big_cmp(big_add(cv->a, three), p) == 0) ? 1u : 0u;
	img[8 * nw + 3] = (big_cmp(fix, R) == 0) ? 1u : 0u;
	if (img.size() * 4 != ecamd_curvek_bytes(nw)) {
		return fail("internal: CurveK image size mismatch");
	}
	SlotRegistry *reg = slot_registry(device);
	if (!reg || nw < 0 || nw >= 18) {
		return fail("internal: no slot registry for this device / width");
	}
	const int slot = slot_acquire(reg->s[nw], ECAMD_MAX_SLOTS_HOST, img,
				      [&](int sl) { return ecamd_upload_curve(nw, sl, img.data(), img.size() * 4); });
	if (slot == -1) {
		return fail("curve: all constant-memory curve slots of this width are in use on this device (free a curve first)");
	}
	if (slot < 0) {
		return fail("curve: upload of the curve constants failed");
	}
	*slot_out = slot;
	return 0;
}
static void release_modulus(int device, int nw, int slot)
{
	SlotRegistry *reg = slot_registry(device);
	if (reg && nw >= 0 && nw < 18 && slot >= 0 && slot < ECAMD_MAX_SLOTS_HOST && reg->s[nw][slot].ref > 0) {
		reg->s[nw][slot].ref--;
	}
}


// w-bit digits of a (nl of them, the last one takes whatever is left): 29 bits on every radix-2^29 unit but the Goldilocks one
// (flavour 5), which runs on 28-bit limbs so that 2^224 falls on a limb boundary (ecamd_u29g.h)
void ecamd_host::big_digits29(uint32_t *dst, int nl, const Big &a, int w)
{
	const int bits = big_bitlen(a);
	for (int i = 0; i < nl; i++) {
		uint64_t d = 0;
		const int lo = w * i, hi = (i == nl - 1) ? (bits > lo + w ? bits : lo + w) : lo + w;
		for (int b = lo; b < hi && b < bits; b++) {
			if ((a[(size_t)b / 32] >> (b % 32)) & 1u) {
				d |= 1ull << (b - lo);
			}
		}
		dst[i] = (uint32_t)d;
	}
}
static Big big_shl(const Big &a, int e)
{
	return big_mul(a, big_pow2(e));
}

// CurveG<NL> image of ecamd_u29g.h: p r2 one a b pm2 (NL digits each), 16 bias tables, ix iy ex ey, mpinv pbits
// a_is_m3 pad -- mirrored by tools/g29_consts.py, which the CPU tests use against Python integers
// (p, a, b, pbits, flavour): the curve's own field (upload_g29), or the group order q with a = b = 0 on the dense unit of its
// size (upload_g29_order: the mod-q algebra of ECDSA verification runs on the same field code, k_ecdsa_prep_g)
static int upload_g29_mod(ecamd_curve *cv, const Big &p, const Big &a_in, const Big &b_in, int pbits, int gflavour, int *slot_out)
{
	const int nl = ecamd_g29_nl(pbits, gflavour);
	// flavours 2 (p = 2^255 - 19), 4 (secp256k1's prime) and 5 (p = 2^448 - 2^224 - 1) keep plain residues: R = 1
	const int w = (gflavour == 5) ? 28 : 29;   // limb width of the unit (g29::W of its translation unit)
	// flavours 1 (p = 2^521 - 1 on 18 limbs), 2, 4 and 5 keep plain residues: R = 1
	const bool plain = gflavour == 1 || gflavour == 2 || gflavour == 4 || gflavour == 5;
	const Big R = plain ? Big(1, 1) : big_mod(big_pow2(w * nl), p);
	Big two(1, 2), three(1, 3);
	static const int step29[16] = {2, 4, 6, 8, 10, 12, 14, 16, 2, 4, 6, 8, 10, 12, 14, 16};
	static const int step28[16] = {1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4, 5, 6, 7, 8};    // g29::bias_step of the no-headroom flavours
	const int *step = (gflavour == 5 || gflavour == 1) ? step28 : step29;
	static const int sv[16] = {1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2};
	const int topsh = pbits - w * (nl - 1);
	const int off = (1 - topsh) > 0 ? (1 - topsh) : 0;
	// Isomorphism onto a curve with a = -3 (cheaper doubling): (x, y) -> (u^2 x, u^3 y) with u^4 a = -3, when such a u
	// exists.  Tried for p = 3 mod 4, where square roots are one exponentiation and exactly one of +-s is a square
	// (the brainpool r1 curves -- their t1 twins are these images --, two GOST 512-bit sets); ECAMD_NO_ISO disables it.
	Big u(1, 1);
	Big a_img = a_in, b_img = b_in;
	if ((gflavour == 0 || gflavour == 3 || gflavour == 5) && (p[0] & 3u) == 3u && big_bitlen(a_in) > 0 && big_cmp(big_add(a_in, three), p) != 0 &&
	    getenv("ECAMD_NO_ISO") == nullptr) {
		Big e = big_add(p, Big(1, 1));  // (p + 1) / 4
		Big q4(e.size(), 0);
		for (size_t i = 0; i < e.size(); i++) {
			q4[i] = (e[i] >> 2) | ((i + 1 < e.size()) ? (e[i + 1] << 30) : 0u);
		}
		big_trim(q4);
		const Big t = big_mulmod(big_sub(p, three), big_powmod(a_in, big_sub(p, two), p), p);  // -3 / a
		Big s1 = big_powmod(t, q4, p);
		if (big_cmp(big_mulmod(s1, s1, p), t) == 0) {
			Big r = big_powmod(s1, q4, p);
			if (big_cmp(big_mulmod(r, r, p), s1) != 0) {
				s1 = big_sub(p, s1);
				r = big_powmod(s1, q4, p);
			}
			if (big_cmp(big_mulmod(r, r, p), s1) == 0) {
				u = r;
				const Big u2 = big_mulmod(u, u, p), u4 = big_mulmod(u2, u2, p);
				a_img = big_mulmod(a_in, u4, p);
				b_img = big_mulmod(b_in, big_mulmod(u4, u2, p), p);
				if (big_cmp(big_add(a_img, three), p) != 0) {
					return fail("internal: isomorphism onto a = -3 failed");
				}
			}
		}
	}
	const Big u2 = big_mulmod(u, u, p), u3 = big_mulmod(u2, u, p);
	const Big RR = big_mulmod(R, R, p);
	std::vector<uint32_t> img((size_t)(10 + 16) * nl + 4, 0);
	big_digits29(&img[0 * nl], nl, p, w);
	big_digits29(&img[1 * nl], nl, RR, w);
	big_digits29(&img[2 * nl], nl, R, w);
	big_digits29(&img[3 * nl], nl, big_mulmod(a_img, R, p), w);
	big_digits29(&img[4 * nl], nl, big_mulmod(b_img, R, p), w);
	big_digits29(&img[5 * nl], nl, big_sub(p, two), w);
	big_digits29(&img[22 * nl], nl, big_mulmod(u2, RR, p), w);                             // ix
	big_digits29(&img[23 * nl], nl, big_mulmod(u3, RR, p), w);                             // iy
	big_digits29(&img[24 * nl], nl, big_powmod(u2, big_sub(p, two), p), w);                // ex = u^-2
	big_digits29(&img[25 * nl], nl, big_powmod(u3, big_sub(p, two), p), w);                // ey = u^-3
	for (int t = 0; t < 16; t++) {
		uint32_t *l = &img[(size_t)(6 + t) * nl];
		if (big_bitlen(p) + step[t] + off > w * (nl - 1) + 32) {
			continue;  // this multiple does not fit the limbs (only without a headroom limb); never selected
		}
		big_digits29(l, nl, big_shl(p, step[t] + off), w);
		const uint32_t M = 1u << (w + sv[t]), BW = 1u << sv[t];
		if (l[nl - 1] < BW) {
			if (gflavour == 5 || gflavour == 1) {
				memset(l, 0, sizeof(uint32_t) * (size_t)nl);
				continue;  // a multiple too small to lend the borrow; never selected (BiasB's static_asserts)
			}
			return fail("internal: bias table underflow");
		}
		l[0] += M;
		for (int j = 1; j < nl - 1; j++) {
			l[j] += M - BW;
		}
		l[nl - 1] -= BW;
	}
	uint32_t p0 = p[0], x = 1;
	for (int i = 0; i < 5; i++) {
		x *= 2u - p0 * x;
	}
	img[(size_t)26 * nl + 0] = (0u - x) & ((1u << w) - 1u);
	img[(size_t)26 * nl + 1] = (uint32_t)pbits;
	img[(size_t)26 * nl + 2] = (big_cmp(big_add(a_img, three), p) == 0) ? 1u : 0u;
	img[(size_t)26 * nl + 3] = (big_bitlen(a_img) == 0) ? 1u : 0u;
	if (img.size() * 4 != ecamd_g29_image_bytes(pbits, gflavour)) {
		return fail("internal: CurveG image size mismatch");
	}
	SlotRegistry *reg = slot_registry(cv->ctx->device);
	const int key = pbits + gflavour;
	if (!reg || key >= ECAMD_G29_KEYS) {
		return fail("internal: no slot registry for this device / field size");
	}
	const int flavour = gflavour;
	const int slot = slot_acquire(reg->g[key], ecamd_g29_slots() < 8 ? ecamd_g29_slots() : 8, img,
				      [&](int sl) { return ecamd_g29_upload(pbits, sl, img.data(), img.size() * 4, flavour); });
	if (slot == -2) {
		return fail("curve: upload of the radix-2^29 curve constants failed");
	}
	*slot_out = slot < 0 ? -1 : slot;  // no free slot: the saturated-word kernels serve this handle
	return 0;
}

static int upload_g29(ecamd_curve *cv)
{
	return upload_g29_mod(cv, cv->p, cv->a, cv->b, cv->pbits, cv->gflavour, &cv->gslot);
}

// prj_pt_import_from_buf + prj_pt_unique of a batch: the handle's radix-2^29 unit when it has one (one inversion per eight triples),
// else one Fermat inversion per triple on saturated words.  ECAMD_NO_PRJ_IMPORT_G29 keeps the latter (A/B hook).
hipError_t ecamd_host::launch_prj_import(const ecamd_curve *cv, const EcamdPrjInArgs &I, hipStream_t s)
{
	static const bool off = getenv("ECAMD_NO_PRJ_IMPORT_G29") != nullptr;
	if (!off && cv->gslot >= 0) {
		return ecamd_g29_prj_import(cv->pbits, cv->gslot, I, s, cv->gflavour);
	}
	if (!off && cv->is_p256 && cv->gpslot >= 0) {
		return ecamd_g29_prj_import(256, cv->gpslot, I, s, 0);
	}
	return ecamd_launch_prj_import(cv->nw, I, s);
}

// the group order as the modulus of the dense unit of its size (only sizes that unit exists for; failure is not an error:
// the saturated-word k_ecdsa_prep keeps serving)
static void upload_g29_order(ecamd_curve *cv)
{
	cv->gqslot = -1;
	const int qbits = big_bitlen(cv->q);
	if (!ecamd_g29_supported(qbits) || qbits == 255 || qbits == 448 || qbits >= ECAMD_G29_KEYS || getenv("ECAMD_NO_PREP_G29") != nullptr ||
	    getenv("ECAMD_NO_FAST_PATH") != nullptr) {
		return;
	}
	int slot = -1;
	if (upload_g29_mod(cv, cv->q, Big(), Big(), qbits, 0, &slot) == 0) {
		cv->gqslot = slot;
	}
}


// device allocations of a curve handle (also used on the failure paths of its construction)
static void curve_free_device(ecamd_curve *cv)
{
	if (cv->d_gen) {
		(void)hipFree(cv->d_gen);
		cv->d_gen = nullptr;
	}
	if (cv->d_comb) {
		(void)hipFree(cv->d_comb);
		cv->d_comb = nullptr;
	}
	if (cv->d_edcomb) {
		(void)hipFree(cv->d_edcomb);
		cv->d_edcomb = nullptr;
	}
	if (cv->d_gtab) {
		(void)hipFree(cv->d_gtab);
		cv->d_gtab = nullptr;
	}
	if (cv->d_comb4) {
		(void)hipFree(cv->d_comb4);
		cv->d_comb4 = nullptr;
	}
}

// constant slots of a handle back to the device's registry (g_slot_mu NOT held by the caller)
static void curve_release_slots(ecamd_curve *cv)
{
	if (!cv->ctx) {
		return;
	}
	std::lock_guard<std::mutex> lk(g_slot_mu);
	const int dev = cv->ctx->device;
	release_modulus(dev, cv->nw, cv->slot);
	release_modulus(dev, cv->qnw, cv->qslot);
	SlotRegistry *reg = slot_registry(dev);
	const int key = cv->pbits + cv->gflavour;
	{
		const int qkey = big_bitlen(cv->q);
		if (reg && cv->gqslot >= 0 && cv->gqslot < 8 && qkey < ECAMD_G29_KEYS && reg->g[qkey][cv->gqslot].ref > 0) {
			reg->g[qkey][cv->gqslot].ref--;
		}
		cv->gqslot = -1;
	}
	if (reg && cv->gslot >= 0 && cv->gslot < 8 && key < ECAMD_G29_KEYS && reg->g[key][cv->gslot].ref > 0) {
		reg->g[key][cv->gslot].ref--;
	}
	if (reg && cv->gpslot >= 0 && cv->gpslot < 8 && reg->g[256][cv->gpslot].ref > 0) {
		reg->g[256][cv->gpslot].ref--;
	}
	cv->slot = cv->qslot = cv->gslot = cv->gqslot = cv->gpslot = -1;
}

// failure exit of curve construction: releases the handle; msg == NULL keeps the error already recorded
static int curve_abort(ecamd_curve *cv, const char *msg)
{
	curve_free_device(cv);
	curve_release_slots(cv);
	delete cv;
	return msg ? fail(msg) : -1;
}

static int curve_finish(ecamd_ctx *ctx, ecamd_curve *cv, ecamd_curve **out)
{
	cv->ctx = nullptr;
	cv->slot = cv->qslot = cv->gslot = cv->gqslot = cv->gpslot = -1;
	cv->d_gen = nullptr;
	cv->d_comb = nullptr;
	cv->d_edcomb = nullptr;
	cv->edcomb_off = false;
	cv->d_gtab = nullptr;
	cv->d_comb4 = nullptr;
	cv->comb4_off = false;
	if (!(cv->p[0] & 1) || big_bitlen(cv->p) < 160) {
		return curve_abort(cv, "curve: p must be odd and at least 160 bits");
	}
	cv->pbits = big_bitlen(cv->p);
	cv->qbits = big_bitlen(cv->q);
	{
		// jmax = floor((p - 1) / q), tiny (1 for cofactor-1 curves with p > q, up to 8 for WEI25519)
		uint32_t j = 0;
		Big t = cv->q;
		while (big_cmp(t, cv->p) < 0 && j < 64) {
			t = big_add(t, cv->q);
			j++;
		}
		cv->jmax = j;
	}
	cv->nw = pick_nw(cv->pbits);
	if (!cv->nw || !ecamd_nw_supported(cv->nw)) {
		return curve_abort(cv, "curve: field size not supported (max 544 bits)");
	}
	if (big_cmp(cv->a, cv->p) >= 0 || big_cmp(cv->b, cv->p) >= 0 || big_cmp(cv->gx, cv->p) >= 0 ||
	    big_cmp(cv->gy, cv->p) >= 0) {
		return curve_abort(cv, "curve: a, b, gx, gy must be < p");
	}
	cv->clen = (cv->pbits + 7) / 8;
	cv->qlen = (cv->qbits + 7) / 8;
	cv->is_p256 =
	    big_cmp(cv->p, big_from_hex("ffffffff00000001000000000000000000000000ffffffffffffffffffffffff")) == 0 &&
	    big_cmp(cv->a, big_from_hex("ffffffff00000001000000000000000000000000fffffffffffffffffffffffc")) == 0 &&
	    big_cmp(cv->b, big_from_hex("5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b")) == 0 &&
	    big_cmp(cv->order, cv->q) == 0 && getenv("ECAMD_NO_FAST_PATH") == nullptr;
	cv->ctx = ctx;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hipSetDevice(ctx->device) != hipSuccess) {
		return curve_abort(cv, "curve: hipSetDevice failed");
	}
	cv->qnw = big_bitlen(cv->q) <= 32 * cv->nw ? cv->nw : pick_nw(big_bitlen(cv->q));
	{
		// slot: the field of definition (modulus p, curve coefficients);  qslot: Montgomery context of the generator
		// order q for the mod-q algebra of the protocol layer (only when q is odd and fits a supported width)
		std::lock_guard<std::mutex> sl(g_slot_mu);
		if (acquire_modulus(ctx->device, cv->nw, cv->p, cv->a, cv->b, &cv->slot)) {
			cv->slot = -1;
		} else if ((cv->q[0] & 1) && cv->qnw && ecamd_nw_supported(cv->qnw)) {
			Big zero(1, 0);
			if (acquire_modulus(ctx->device, cv->qnw, cv->q, zero, zero, &cv->qslot)) {
				cv->qslot = -1;  // protocol entry points unavailable on this handle
			}
		}
	}
	if (cv->slot < 0) {
		return curve_abort(cv, nullptr);
	}
	cv->gflavour = (cv->pbits == 521 && big_cmp(big_add(cv->p, Big(1, 1)), big_pow2(521)) == 0) ? 1 : 0;
	if (cv->pbits == 255 && big_cmp(big_add(cv->p, Big(1, 19)), big_pow2(255)) == 0 && getenv("ECAMD_NO_P25519") == nullptr) {
		cv->gflavour = 2;
	}
	if (cv->pbits == 256 && getenv("ECAMD_NO_K256") == nullptr &&
	    big_cmp(cv->p, big_from_hex("fffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f")) == 0) {
		cv->gflavour = 4;  // p = 2^256 - 2^32 - 977 (secp256k1): plain residues, pseudo-Mersenne folds
	}
	if (cv->pbits == 448 && getenv("ECAMD_NO_P448") == nullptr &&
	    big_cmp(cv->p, big_sub(big_sub(big_pow2(448), big_pow2(224)), Big(1, 1))) == 0) {
		cv->gflavour = 5;  // p = 2^448 - 2^224 - 1 (WEI448): plain residues, Goldilocks folds
	}
	if (getenv("ECAMD_NO_MPINV1") == nullptr) {
		// the other two NIST primes with a two-term p -+ 1: secp224r1 (2^224 - 2^96 + 1) and secp192r1 (2^192 - 2^64 - 1)
		if (cv->pbits == 224 && big_cmp(big_add(cv->p, big_pow2(96)), big_add(big_pow2(224), Big(1, 1))) == 0) {
			cv->gflavour = 6;
		}
		if (cv->pbits == 192 && big_cmp(big_add(cv->p, big_add(big_pow2(64), Big(1, 1))), big_pow2(192)) == 0) {
			cv->gflavour = 7;
		}
	}
	if (cv->pbits == 384 && getenv("ECAMD_NO_MPINV1") == nullptr &&
	    big_cmp(big_add(cv->p, big_add(big_pow2(128), big_pow2(96))), big_add(big_pow2(384), big_sub(big_pow2(32), Big(1, 1)))) == 0) {
		cv->gflavour = 3;  // secp384r1's prime: Montgomery reduction on the four signed digits of p + 1 (ecamd_u29g.h, -DG29_P384S)
	}
	if (!cv->is_p256 && ecamd_g29_supported(cv->pbits) && cv->pbits + 8 < ECAMD_G29_KEYS && getenv("ECAMD_NO_FAST_PATH") == nullptr) {
		int rc;
		{
			std::lock_guard<std::mutex> sl(g_slot_mu);
			rc = upload_g29(cv);
		}
		if (rc) {
			return curve_abort(cv, nullptr);
		}
	}
	{
		std::lock_guard<std::mutex> sl(g_slot_mu);
		upload_g29_order(cv);
		if (cv->is_p256 && getenv("ECAMD_NO_FAST_PATH") == nullptr) {
			int slot = -1;
			if (upload_g29_mod(cv, cv->p, cv->a, cv->b, 256, 0, &slot) == 0) {
				cv->gpslot = slot;   // failure is not an error: the saturated-word import keeps serving
			}
		}
	}
	// generator X || Y, then the two broadcast scalars of the subgroup / cofactor passes: q (qlen bytes) and h (1 byte)
	std::vector<uint8_t> g((size_t)2 * cv->clen + cv->qlen + 1, 0);
	big_to_be(g.data(), cv->clen, cv->gx);
	big_to_be(g.data() + cv->clen, cv->clen, cv->gy);
	big_to_be(g.data() + 2 * cv->clen, cv->qlen, cv->q);
	{
		Big t = cv->q;
		for (uint32_t c = 1; c <= 255; c++) {
			if (big_cmp(t, cv->order) == 0) {
				g[(size_t)2 * cv->clen + cv->qlen] = (uint8_t)c;   // stays 0 when order is not a small multiple of q
				cv->cofactor = c;
				break;
			}
			t = big_add(t, cv->q);
		}
	}
	if (hipMalloc((void **)&cv->d_gen, g.size()) != hipSuccess ||
	    hipMemcpy(cv->d_gen, g.data(), g.size(), hipMemcpyHostToDevice) != hipSuccess) {
		return curve_abort(cv, "curve: generator upload failed");
	}
	cv->d_gtab = nullptr;
	cv->d_comb4 = nullptr;
	cv->comb4_off = false;
	cv->d_comb = nullptr;
	cv->comb_off = false;
	cv->d_edcomb = nullptr;
	cv->edcomb_off = false;
	cv->sqrt_state = 0;
	cv->ed_state = 0;
	cv->ed448_state = 0;
	cv->ed448_err = nullptr;
	cv->xdh_state = 0;
	cv->ed_err = cv->xdh_err = nullptr;
	if (cv->is_p256) {
		// affine window table of the generator for the interleaved ECDSA verification loop:
		// [1..8]G through our own kernels, then x R mod p, y R mod p (R = 2^261) as 29-bit digits
		uint8_t sc[8 * 32], pts[8 * 64], st[8];
		memset(sc, 0, sizeof(sc));
		for (int i = 0; i < 8; i++) {
			sc[i * 32 + 31] = (uint8_t)(i + 1);
		}
		uint8_t *d = nullptr;
		if (hipMalloc((void **)&d, sizeof(sc) + sizeof(pts) + sizeof(st)) != hipSuccess) {
			return curve_abort(cv, "curve: generator table allocation failed");
		}
		if (hipMemcpy(d, sc, sizeof(sc), hipMemcpyHostToDevice) != hipSuccess) {
			(void)hipFree(d);
			return curve_abort(cv, "curve: generator table upload failed");
		}
		int rc = smul_dev_locked(ctx, cv, 8, d, 32, nullptr, d + sizeof(sc), d + sizeof(sc) + sizeof(pts), ctx->stream);
		if (!rc && (hipStreamSynchronize(ctx->stream) != hipSuccess ||
			    hipMemcpy(pts, d + sizeof(sc), sizeof(pts), hipMemcpyDeviceToHost) != hipSuccess ||
			    hipMemcpy(st, d + sizeof(sc) + sizeof(pts), sizeof(st), hipMemcpyDeviceToHost) != hipSuccess)) {
			rc = -1;
		}
		(void)hipFree(d);
		std::vector<uint32_t> tab(8 * 40, 0);
		const Big R261 = big_mod(big_pow2(261), cv->p);
		for (int i = 0; i < 8 && !rc; i++) {
			if (st[i] != 0) {
				rc = -1;
				break;
			}
			big_digits29(&tab[(size_t)i * 40], 9, big_mulmod(big_from_be(pts + i * 64, 32), R261, cv->p));
			big_digits29(&tab[(size_t)i * 40 + 9], 9, big_mulmod(big_from_be(pts + i * 64 + 32, 32), R261, cv->p));
		}
		if (rc || hipMalloc((void **)&cv->d_gtab, tab.size() * 4) != hipSuccess ||
		    hipMemcpy(cv->d_gtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
			return curve_abort(cv, "curve: generator table construction failed");
		}
		big_digits29(cv->qdig, 9, cv->q);
		// the masked 4-bit comb of the generator for secret scalars (k_p256_comb4m): [m 16^j]G, m = 1..8, j = 0..63, and [2^256]G, again
		// through our own kernels (public scalars: constants of the curve).  Not fatal when it fails: the masked window loop serves.
		if (getenv("ECAMD_NO_SECRET_COMB") == nullptr) {
			const uint32_t ne = 64 * 8 + 1;
			std::vector<uint8_t> hs((size_t)ne * 32, 0), hp((size_t)ne * 64), hst(ne, 1);
			for (uint32_t j = 0; j < 64; j++) {
				for (uint32_t m = 1; m <= 8; m++) {
					hs[((size_t)j * 8 + (m - 1)) * 32 + 31 - j / 2] = (uint8_t)(m << (4 * (j & 1)));
				}
			}
			big_to_be(&hs[(size_t)64 * 8 * 32], 32, big_mod(big_pow2(256), cv->q));
			uint8_t *dd = nullptr;
			bool ok = hipMalloc((void **)&dd, hs.size() + hp.size() + hst.size()) == hipSuccess &&
				  hipMemcpy(dd, hs.data(), hs.size(), hipMemcpyHostToDevice) == hipSuccess;
			if (ok) {
				PublicScalars pub_scope(ctx);
				ok = smul_dev_locked(ctx, cv, ne, dd, 32, nullptr, dd + hs.size(), dd + hs.size() + hp.size(), ctx->stream) == 0 &&
				     hipStreamSynchronize(ctx->stream) == hipSuccess &&
				     hipMemcpy(hp.data(), dd + hs.size(), hp.size(), hipMemcpyDeviceToHost) == hipSuccess &&
				     hipMemcpy(hst.data(), dd + hs.size() + hp.size(), hst.size(), hipMemcpyDeviceToHost) == hipSuccess;
			}
			if (dd) {
				(void)hipFree(dd);
			}
			std::vector<uint32_t> tab4((size_t)65 * 8 * 40, 0);
			for (uint32_t e = 0; ok && e < ne; e++) {
				ok = hst[e] == 0;
				big_digits29(&tab4[(size_t)e * 40], 9, big_mulmod(big_from_be(&hp[(size_t)e * 64], 32), R261, cv->p));
				big_digits29(&tab4[(size_t)e * 40 + 9], 9, big_mulmod(big_from_be(&hp[(size_t)e * 64 + 32], 32), R261, cv->p));
			}
			if (ok && hipMalloc((void **)&cv->d_comb4, tab4.size() * 4) == hipSuccess &&
			    hipMemcpy(cv->d_comb4, tab4.data(), tab4.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
				(void)hipFree(cv->d_comb4);
				cv->d_comb4 = nullptr;
			}
			(void)hipGetLastError();
		}
	}
	*out = cv;
	return 0;
}

extern "C" int ecamd_curve_by_name(ecamd_ctx *ctx, const char *name, ecamd_curve **out)
{
	if (!ctx || !name || !out) {
		return fail("ecamd_curve_by_name: NULL argument");
	}
	*out = nullptr;
	for (const CurveRow &r : g_curve_rows) {
		if (strcasecmp(r.name, name) == 0) {
			ecamd_curve *cv = new ecamd_curve();
			cv->curve_type = r.type;
			cv->p = big_from_hex(r.p);
			cv->a = big_from_hex(r.a);
			cv->b = big_from_hex(r.b);
			cv->order = big_from_hex(r.order);
			cv->gx = big_from_hex(r.gx);
			cv->gy = big_from_hex(r.gy);
			cv->q = big_from_hex(r.q);
			return curve_finish(ctx, cv, out);
		}
	}
	return fail(std::string("ecamd_curve_by_name: unknown curve ") + name);
}

extern "C" int ecamd_curve_from_params(ecamd_ctx *ctx, const uint8_t *p, uint32_t p_len, const uint8_t *a,
				       uint32_t a_len, const uint8_t *b, uint32_t b_len,
				       const uint8_t *curve_order, uint32_t curve_order_len,
				       const uint8_t *gx, uint32_t gx_len, const uint8_t *gy, uint32_t gy_len,
				       const uint8_t *gen_order, uint32_t gen_order_len, ecamd_curve **out)
{
	if (!ctx || !p || !a || !b || !curve_order || !gx || !gy || !gen_order || !out) {
		return fail("ecamd_curve_from_params: NULL argument");
	}
	*out = nullptr;
	ecamd_curve *cv = new ecamd_curve();
	cv->p = big_from_be(p, p_len);
	cv->a = big_from_be(a, a_len);
	cv->b = big_from_be(b, b_len);
	cv->order = big_from_be(curve_order, curve_order_len);
	cv->gx = big_from_be(gx, gx_len);
	cv->gy = big_from_be(gy, gy_len);
	cv->q = big_from_be(gen_order, gen_order_len);
	return curve_finish(ctx, cv, out);
}

extern "C" void ecamd_curve_free(ecamd_curve *cv)
{
	if (!cv) {
		return;
	}
	{
		std::lock_guard<std::mutex> lk(cv->ctx->mu);
		(void)hipSetDevice(cv->ctx->device);
		// kernels of this handle may still be in flight on the context's stream: let them finish before its constant
		// slots can be handed to another curve
		(void)hipStreamSynchronize(cv->ctx->stream);
		curve_free_device(cv);
	}
	curve_release_slots(cv);
	delete cv;
}

extern "C" int ecamd_curve_coord_len(const ecamd_curve *cv) { return cv ? cv->clen : -1; }
extern "C" int ecamd_curve_order_len(const ecamd_curve *cv) { return cv ? cv->qlen : -1; }
extern "C" int ecamd_curve_words(const ecamd_curve *cv) { return cv ? cv->nw : -1; }

// ------------------------------------------------------------------------------------------
// batched prj_pt_mul
// ------------------------------------------------------------------------------------------
// secp256r1 fast path scratch (ecamd_p256_kernel.hip): P256_TAB_BYTES of affine records + P256_STG_QUADS x 16-byte staging quads
// per item (ecamd_internal.h)
#define P256_SCRATCH_PER_ITEM ((size_t)P256_TAB_BYTES + P256_STG_QUADS * 16u)

static size_t tbl_bytes_for(const ecamd_curve *cv, uint32_t stride)
{
	return (size_t)ECAMD_TBL_ENTRIES * 3 * (size_t)cv->nw * 4 * (size_t)stride;
}

// 16-bit comb table of the generator: T[j][m-1] = [m 2^(16 j)]G (m = 1..32768, j over every 16-bit window of
// the longest scalar the fast path takes) plus [2^(8 slen)]G, computed by this engine itself through the
// window path and converted to the kernels' field representation on the device.  42 MB (256-bit curves) to
// 183 MB (521 bits) of the 288 GB per curve handle; turns [k]G into 2 NW + 1 additions.  ctx->mu held.
void ecamd_host::maybe_build_comb(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n)
{
	if (cv->d_comb || cv->comb_off || ctx->comb_min_batch == 0 || n < ctx->comb_min_batch) {
		return;
	}
	const bool p256 = cv->is_p256;
	if (!p256 && cv->gslot < 0) {
		return;
	}
	cv->comb_off = true;  // no recursion while building; stays set if anything fails
	// the build reuses the context's scratch tables on the context's stream: let kernels the caller has in
	// flight on other streams (earlier stages of the same entry point) finish first -- a one-time event
	if (hipDeviceSynchronize() != hipSuccess) {
		return;
	}
	const uint32_t nwords = (uint32_t)((cv->pbits + 31) / 32);
	const uint32_t slen = 4 * nwords, nwin = 2 * nwords;
	const uint32_t ne = nwin * 32768u + 1u;
	const uint32_t ew = p256 ? 20u : ecamd_g29_comb_entry_words(cv->pbits, cv->gflavour);
	if (!p256 && ne != ecamd_g29_comb_entries(cv->pbits)) {
		return;
	}
	std::vector<uint8_t> hs((size_t)ne * slen, 0);
	for (uint32_t j = 0; j < nwin; j++) {
		for (uint32_t m = 1; m <= 32768; m++) {
			uint8_t *e = &hs[((size_t)j * 32768 + (m - 1)) * slen];
			e[slen - 1 - 2 * j] = (uint8_t)(m & 0xff);
			e[slen - 2 - 2 * j] = (uint8_t)(m >> 8);
		}
	}
	big_to_be(&hs[(size_t)nwin * 32768 * slen], (int)slen, big_mod(big_pow2(8 * (int)slen), cv->q));
	const size_t plen = (size_t)2 * cv->clen;
	uint8_t *dsc = nullptr, *dpt = nullptr, *dst = nullptr;
	uint32_t *table = nullptr;
	std::vector<uint8_t> st(ne);
	hipStream_t s = ctx->stream;
	bool ok = hipMalloc((void **)&dsc, hs.size()) == hipSuccess && hipMalloc((void **)&dpt, (size_t)ne * plen) == hipSuccess &&
		  hipMalloc((void **)&dst, ne) == hipSuccess && hipMalloc((void **)&table, (size_t)ne * ew * 4) == hipSuccess &&
		  hipMemcpy(dsc, hs.data(), hs.size(), hipMemcpyHostToDevice) == hipSuccess;
	{
		// the build is one big batch of its own: do not let a small user chunk turn it into thousands of launches
		const uint32_t user_chunk = ctx->max_chunk;
		ctx->max_chunk = user_chunk < (1u << 20) ? (1u << 20) : user_chunk;
		ok = ok && smul_dev_locked(ctx, cv, ne, dsc, slen, nullptr, dpt, dst, s) == 0;
		ctx->max_chunk = user_chunk;
	}
	if (ok) {
		const hipError_t e = p256 ? ecamd_launch_comb_build_p256(dpt, ne, table, s)
					  : ecamd_g29_comb_build(cv->pbits, cv->gslot, dpt, ne, (uint32_t)cv->clen, table, s, cv->gflavour);
		ok = e == hipSuccess && hipMemcpyAsync(st.data(), dst, ne, hipMemcpyDeviceToHost, s) == hipSuccess &&
		     hipStreamSynchronize(s) == hipSuccess;
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
		return;  // the window path keeps serving fixed-base calls
	}
	cv->d_comb = table;
	cv->comb_off = false;
}

// The generator's 4-bit comb for SECRET scalars on a radix-2^29 unit (k_comb_g<.., SCAN4>): [m 16^j]G, m = 1..8, j = 0 .. 8 NW - 1, and
// [2^(32 NW)]G, (8 NW + 1) x 8 entries of the unit's comb-entry format, built on the first secret fixed-base call of the handle through
// the library's own (public-scalar) multiplication.  Failure is not an error: the masked window loop keeps serving.
static void maybe_build_comb4(ecamd_ctx *ctx, ecamd_curve *cv)
{
	static const bool off = getenv("ECAMD_NO_SECRET_COMB") != nullptr;
	if (off || cv->d_comb4 || cv->comb4_off || cv->is_p256 || cv->gslot < 0) {
		return;
	}
	cv->comb4_off = true;   // one attempt
	if (hipDeviceSynchronize() != hipSuccess) {
		return;
	}
	const uint32_t nwords = (uint32_t)((cv->pbits + 31) / 32);
	const uint32_t slen = 4 * nwords, nwin = 8 * nwords, ne = nwin * 8u + 1u;
	const uint32_t ew = ecamd_g29_comb_entry_words(cv->pbits, cv->gflavour);
	if (slen > ecamd_g29_comb_max_slen(cv->pbits)) {
		return;
	}
	std::vector<uint8_t> hs((size_t)ne * slen, 0), st(ne, 1);
	for (uint32_t j = 0; j < nwin; j++) {
		for (uint32_t m = 1; m <= 8; m++) {
			hs[((size_t)j * 8 + (m - 1)) * slen + slen - 1 - j / 2] = (uint8_t)(m << (4 * (j & 1)));
		}
	}
	big_to_be(&hs[(size_t)nwin * 8 * slen], (int)slen, big_mod(big_pow2(8 * (int)slen), cv->q));
	const size_t plen = (size_t)2 * cv->clen;
	uint8_t *dsc = nullptr, *dpt = nullptr, *dst = nullptr;
	uint32_t *table = nullptr;
	hipStream_t s = ctx->stream;
	bool ok = hipMalloc((void **)&dsc, hs.size()) == hipSuccess && hipMalloc((void **)&dpt, (size_t)ne * plen) == hipSuccess &&
		  hipMalloc((void **)&dst, ne) == hipSuccess && hipMalloc((void **)&table, (size_t)(nwin + 1) * 8 * ew * 4) == hipSuccess &&
		  hipMemset(table, 0, (size_t)(nwin + 1) * 8 * ew * 4) == hipSuccess &&
		  hipMemcpy(dsc, hs.data(), hs.size(), hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		PublicScalars pub_scope(ctx);   // constants of the curve
		ok = smul_dev_locked(ctx, cv, ne, dsc, slen, nullptr, dpt, dst, s) == 0 &&
		     ecamd_g29_comb_build(cv->pbits, cv->gslot, dpt, ne, (uint32_t)cv->clen, table, s, cv->gflavour) == hipSuccess &&
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
		return;
	}
	cv->d_comb4 = table;
}

// sstride = slen normally; 0 broadcasts one scalar to every item (subgroup / cofactor passes)
int ecamd_host::smul_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_scalars,
			   uint32_t slen, const uint8_t *d_points, uint8_t *d_out, uint8_t *d_status,
			   hipStream_t s, uint32_t sstride, bool redo_only, const uint8_t *d_scalars2)
{
	// d_scalars2 (generic radix-2^29 units with a comb table, see fused_verify_ok): out = [scalars]P + [scalars2]G by the fused
	// window loop; items that met an exceptional pair keep ECAMD_STATUS_REDO in d_status for the caller (no complete-formula pass here)
	// redo_only: d_status is given; only the items marked ECAMD_STATUS_REDO in it are computed (complete-formula kernel)
	if (sstride == 0xffffffffu) {
		sstride = slen;
	}
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	const uint32_t stride = (chunk + 63u) & ~63u;
	// secp256r1: the window loop takes scalars of up to 68 bytes (blinded scalars m + b #E of about 2 |q| bits stay on the fast
	// kernel); the fixed-base comb covers the 32-byte ones
	// secret-scalar mode: every item goes through the complete-formula kernel with masked full-table look-ups -- no digit-indexed
	// address (window or comb table), no exceptional-pair detour whose occurrence depends on the scalar
	// (secp256r1 keeps its radix-2^29 pipeline in this mode: k_p256_loop<KW, MASKED> scans the eight-entry tables, the comb is off)
	const bool secret = ctx->secret_scalars;
	const bool fast256 = cv->is_p256 && slen <= 68;
	const bool fastg = !fast256 && cv->gslot >= 0 && slen <= ecamd_g29_max_slen(cv->pbits);
	const bool comb_ok = !secret && (cv->is_p256 ? slen <= 32 : slen <= ecamd_g29_comb_max_slen(cv->pbits));
	const bool fast = !redo_only && (fast256 || fastg);
	if (fast && !d_points && comb_ok) {
		maybe_build_comb(ctx, const_cast<ecamd_curve *>(cv), n);
	}
	if (fast && fastg && !d_points && secret && n >= 64) {
		maybe_build_comb4(ctx, const_cast<ecamd_curve *>(cv));
	}
	{
		uint8_t *t = (uint8_t *)ctx->tbl;
		const int rc = ensure(&t, &ctx->tbl_bytes, tbl_bytes_for(cv, stride));
		ctx->tbl = (uint32_t *)t;
		if (rc) {
			return -1;
		}
	}
	if (fast) {
		uint8_t *t = (uint8_t *)ctx->tbl_fast;
		const size_t per_item = fast256 ? P256_SCRATCH_PER_ITEM
						: ((size_t)ecamd_g29_table_words(cv->pbits, cv->gflavour) + ecamd_g29_affine_words(cv->pbits, cv->gflavour)) * 4;
		const int rc = ensure(&t, &ctx->tbl_fast_bytes, (size_t)stride * per_item);
		ctx->tbl_fast = (uint32_t *)t;
		if (rc) {
			return -1;
		}
	}
	for (uint32_t off = 0; off < n; off += chunk) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		EcamdSmulArgs A;
		A.scalars = d_scalars + (size_t)off * sstride;
		A.sstride = sstride;
		A.pstride = d_points ? 2u * (uint32_t)cv->clen : 0u;
		A.points = d_points ? d_points + (size_t)off * 2 * cv->clen : cv->d_gen;
		A.out = d_out + (size_t)off * 2 * cv->clen;
		A.status = d_status + off;
		A.tbl = ctx->tbl;
		A.n = m;
		A.slen = slen;
		A.clen = (uint32_t)cv->clen;
		A.stride = stride;
		A.slot = cv->slot;
		A.only_redo = redo_only ? 1 : 0;
		A.lut = nullptr;
		A.lut_kind = 0;
		A.stg = nullptr;
		A.masked = secret ? 1 : 0;   // (copied into Fa below: the secp256r1 loop honours it too)
		A.scalars2 = nullptr;
		A.s2len = 0;
		if (d_scalars2) {
			if (!fastg || !d_points || !cv->d_comb) {
				return fail("internal: fused double-scalar loop requested without its preconditions");
			}
			EcamdSmulArgs Fa = A;
			Fa.tbl = ctx->tbl_fast;
			Fa.stg = ctx->tbl_fast + (size_t)stride * (size_t)ecamd_g29_table_words(cv->pbits, cv->gflavour);
			Fa.lut = cv->d_comb;
			Fa.lut_kind = 2u;
			Fa.scalars2 = d_scalars2 + (size_t)off * slen;
			Fa.s2len = slen;
			Fa.masked = 0;
			hipEvent_t *ev = (ctx->timing && off == 0) ? ctx->ev : nullptr;
			HIPCHK(ecamd_launch_smul_g29(cv->pbits, cv->gslot, Fa, s, ev, cv->gflavour));
			ctx->ev_valid = ctx->ev_valid || (ev != nullptr);
			continue;
		}
		if (fast) {
			// Jacobian fast path; lanes that met an exceptional pair come back as ECAMD_STATUS_REDO and
			// are recomputed by the complete-formula kernel (all other lanes exit at once)
			EcamdSmulArgs Fa = A;
			Fa.tbl = ctx->tbl_fast;
			Fa.stg = ctx->tbl_fast + (size_t)stride * (fast256 ? (size_t)(P256_TAB_BYTES / 4) : (size_t)ecamd_g29_table_words(cv->pbits, cv->gflavour));
			// fixed base: a constant table of the generator replaces the per-item table kernels
			if (!d_points) {
				const bool use_comb = cv->d_comb && comb_ok;
				Fa.lut = use_comb ? cv->d_comb : (fast256 ? cv->d_gtab : nullptr);
				Fa.lut_kind = use_comb ? 1u : 0u;
				if (secret && cv->d_comb4 && (fast256 ? slen <= 32 : slen <= 4 * (uint32_t)((cv->pbits + 31) / 32))) {
					Fa.lut = cv->d_comb4;   // secret scalars: the scanned 4-bit comb (8 NW + 1 additions) instead of the scanned window loop
					Fa.lut_kind = 3u;
				}
			}
			hipEvent_t *ev = (ctx->timing && off == 0) ? ctx->ev : nullptr;  // first chunk of the call
			if (fast256) {
				HIPCHK(ecamd_launch_smul_p256(Fa, s, ev));
			} else {
				HIPCHK(ecamd_launch_smul_g29(cv->pbits, cv->gslot, Fa, s, ev, cv->gflavour));
			}
			ctx->ev_valid = ctx->ev_valid || (ev != nullptr);
			A.only_redo = 1;
		}
		HIPCHK(ecamd_launch_smul(cv->nw, A, s));
	}
	return 0;
}

// ------------------------------------------------------------------------------------------
// Host-pointer entry points = the device-pointer cores behind copies of the caller's arrays.  The batch goes
// through in chunks of ctx->host_chunk items with double-buffered device staging: while the kernels of chunk
// c run on the compute stream, the host thread is inside the (pageable, hence host-blocking) copy of chunk
// c+1 on the copy stream, so PCIe and the GPU work concurrently.  `ins` / `outs`: the caller's arrays with
// their per-item strides (a NULL input is passed on as NULL); core(m, in_ptrs, out_ptrs, stream) enqueues one
// chunk and may synchronise (after calling `between`).  ctx->mu held.
// ------------------------------------------------------------------------------------------

int ecamd_host::host_pipeline(ecamd_ctx *ctx, int pbits, uint32_t n, const std::vector<HostArr> &arrs, const HostCore &core, uint32_t even_chunk)
{
	// even_chunk != 0 (the whole-batch forms that file a batch chunk by chunk: their per-chunk kernels are light, what matters is that the LAST
	// chunk -- whose copy nothing hides -- is small): a short first chunk, then equal chunks of that size
	const uint32_t chunk = even_chunk && even_chunk < ctx->host_chunk ? (n < even_chunk ? n : even_chunk) : (n < ctx->host_chunk ? n : ctx->host_chunk);
	const size_t na = arrs.size();
	if (na > 6) {
		return fail("internal: too many host arrays");
	}
	// The chunk schedule.  Nothing overlaps the copy of the FIRST chunk (and, with a producer hook, its packing), and the copy of chunk
	// c + 1 hides behind the kernels of chunk c only when it is not much larger than c: so a batch of several chunks starts short -- 2^16
	// items ($ECAMD_HOST_RAMP_MIN) -- and DOUBLES up to the chunk size (round 6: with an eighth of a chunk followed at once by a full
	// chunk the device sat idle for 1.7 ms of a 2^20-item verification, waiting for 111 MB to arrive behind 1.4 ms of kernels;
	// profiles/r6c_typed_boundary.md), and a remainder of up to a chunk and a quarter goes as ONE launch (2^20 items: 2^16, 2^17, 2^18,
	// 589 824 = three full rounds of the window kernels' 3 072 resident waves).  $ECAMD_HOST_SCHEDULE=a,b,c: explicit leading chunk
	// sizes (tests, measurements); $ECAMD_NO_HOST_RAMP: equal chunks.
	static const bool no_ramp = getenv("ECAMD_NO_HOST_RAMP") != nullptr;
	std::vector<uint32_t> sched;
	{
		uint32_t left = n;
		if (const char *e = getenv("ECAMD_HOST_SCHEDULE")) {
			while (*e && left) {
				uint32_t v = (uint32_t)strtoul(e, nullptr, 10);
				v = v < 1 ? 1 : (v > left ? left : v);
				sched.push_back(v);
				left -= v;
				e = strchr(e, ',');
				if (!e) {
					break;
				}
				e++;
			}
		} else if (even_chunk && n > chunk) {
			const uint32_t m = ctx->host_first_min < chunk ? ctx->host_first_min : chunk;
			if (m < chunk && left > m) {
				sched.push_back(m);
				left -= m;
			}
		} else if (n > chunk && !no_ramp && pbits <= 256) {
			for (uint32_t m = ctx->host_first_min < chunk ? ctx->host_first_min : chunk; m < chunk && left > m + m; m += m) {
				sched.push_back(m);
				left -= m;
			}
		} else if (n > chunk && !no_ramp) {
			// fields above 256 bits: the kernels of a 2^16-item chunk outlast the copy of a full one (secp384r1: 4 ms against 2.7), and
			// their window loops lose more to short launches than the doubling wins (measured: 60.6 against 63.6 ms per 2^20
			// verifications) -- one short chunk, then full ones
			const uint32_t m = chunk / 8 < ctx->host_first_min ? ctx->host_first_min : chunk / 8;
			if (m < chunk) {
				sched.push_back(m);
				left -= m;
			}
		}
		while (left) {
			const uint32_t m = (left <= chunk + chunk / 4) ? left : chunk;
			sched.push_back(m);
			left -= m;
		}
	}
	uint32_t largest = 0;
	for (uint32_t m : sched) {
		largest = m > largest ? m : largest;
	}
	const int nbuf = sched.size() > 1 ? 2 : 1;
	for (int b = 0; b < nbuf; b++) {
		for (size_t k = 0; k < na; k++) {
			if (ensure(&ctx->hbuf[b][k], &ctx->hbuf_bytes[b][k], (size_t)largest * arrs[k].stride)) {
				return -1;
			}
		}
	}
	hipStream_t cs = ctx->copy_stream, s = ctx->stream;
	StreamScope scope(ctx, s);
	auto copy_in = [&](uint32_t off, uint32_t m, int b) -> int {
		if (ctx->ready_fn) {
			ctx->ready_fn(ctx->ready_arg, off, m);   // the producer of the arrays completes [off, off + m) first
		}
		for (size_t k = 0; k < na; k++) {
			if (arrs[k].in) {
				HIPCHK(hipMemcpyAsync(ctx->hbuf[b][k], arrs[k].in + (size_t)off * arrs[k].stride, (size_t)m * arrs[k].stride,
						      hipMemcpyHostToDevice, cs));
			}
		}
		HIPCHK(hipEventRecord(ctx->in_ready[b], cs));
		return 0;
	};
	if (copy_in(0, sched[0], 0)) {
		return -1;
	}
	int b = 0;
	uint32_t off = 0;
	for (size_t ci = 0; ci < sched.size(); off += sched[ci], ci++, b ^= (nbuf - 1)) {
		const uint32_t m = sched[ci];
		std::vector<const uint8_t *> ip(na, nullptr);
		std::vector<uint8_t *> op(na, nullptr);
		for (size_t k = 0; k < na; k++) {
			ip[k] = arrs[k].in ? ctx->hbuf[b][k] : nullptr;
			op[k] = arrs[k].out ? ctx->hbuf[b][k] : nullptr;
		}
		HIPCHK(hipStreamWaitEvent(s, ctx->in_ready[b], 0));
		// `between`: called once this chunk's kernels are enqueued and before anything waits for them -- by the
		// core itself if it has to synchronise (ECDSA re-checks exceptional items), otherwise right after it
		bool next_issued = false;
		const uint32_t noff = off + m;
		const std::function<int()> between = [&]() -> int {
			if (next_issued || ci + 1 >= sched.size()) {
				return 0;
			}
			next_issued = true;
			// the other staging set is free: its chunk was drained at the end of the previous iteration
			return copy_in(noff, sched[ci + 1], b ^ 1);
		};
		if (core(m, ip, op, s, between) || between()) {
			// leave nothing in flight on the staging buffers of a failed call
			(void)hipStreamSynchronize(cs);
			(void)hipStreamSynchronize(s);
			return -1;
		}
		for (size_t k = 0; k < na; k++) {
			if (arrs[k].out) {
				HIPCHK(hipMemcpyAsync(arrs[k].out + (size_t)off * arrs[k].stride, ctx->hbuf[b][k], (size_t)m * arrs[k].stride,
						      hipMemcpyDeviceToHost, s));
			}
		}
		HIPCHK(hipStreamSynchronize(s));
	}
	return 0;
}


int ecamd_host::host_call(ecamd_ctx *ctx, int pbits, uint32_t n, const std::vector<HostArr> &arrs, const HostCore &core)
{
	std::lock_guard<std::mutex> lk(ctx->mu);
	HIPCHK(hipSetDevice(ctx->device));
	return host_pipeline(ctx, pbits, n, arrs, core);
}

extern "C" int ecamd_ctx_set_host_ready_hook(ecamd_ctx *ctx, ecamd_host_ready_fn fn, void *arg)
{
	if (!ctx) {
		return fail("ecamd_ctx_set_host_ready_hook: NULL context");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);
	ctx->ready_fn = fn;
	ctx->ready_arg = fn ? arg : nullptr;
	return 0;
}

extern "C" int ec_prj_pt_mul_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n,
				       const void *d_scalars, uint32_t slen, const void *d_points,
				       void *d_out, void *d_status, void *hip_stream)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!d_scalars || !d_out || !d_status))) {
		return fail("ec_prj_pt_mul_batch_dev: bad argument");
	}
	if (slen == 0 || slen > 1024) {
		return fail("ec_prj_pt_mul_batch_dev: scalar_len must be in 1..1024");
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return smul_dev_locked(ctx, cv, n, (const uint8_t *)d_scalars, slen, (const uint8_t *)d_points,
				       (uint8_t *)d_out, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_prj_pt_mul_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *scalars,
				   uint32_t slen, const uint8_t *points, uint8_t *out, uint8_t *status)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!scalars || !out || !status))) {
		return fail("ec_prj_pt_mul_batch: bad argument");
	}
	if (slen == 0 || slen > 1024) {
		return fail("ec_prj_pt_mul_batch: scalar_len must be in 1..1024");
	}
	if (n == 0) {
		return 0;
	}
	const size_t plen = (size_t)2 * cv->clen;
	const std::vector<HostArr> arrs = {{scalars, nullptr, slen}, {points, nullptr, plen}, {nullptr, out, plen}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return smul_dev_locked(ctx, cv, m, ip[0], slen, ip[1], op[2], op[3], s);
	});
}

// prj_pt_mul_blind in batch: the scalar multiplied is m + b #E (curves/prj_pt.c:1782-1822), b supplied by the caller
extern "C" int ec_prj_pt_mul_blind_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *scalars, uint32_t slen,
					 const uint8_t *blinds, uint32_t blen, const uint8_t *points, uint8_t *out, uint8_t *status)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!scalars || !blinds || !out || !status))) {
		return fail("ec_prj_pt_mul_blind_batch: bad argument");
	}
	if (slen == 0 || slen > 128 || blen == 0 || blen > 72) {
		return fail("ec_prj_pt_mul_blind_batch: scalar_len must be in 1..128, blind_len in 1..72");
	}
	if (n == 0) {
		return 0;
	}
	const uint32_t ow = (uint32_t)((big_bitlen(cv->order) + 31) / 32);
	uint32_t outlen = blen + 4 * ow;
	outlen = (outlen > slen ? outlen : slen) + 1;
	if (ow > 18 || (outlen + 3) / 4 > 72) {
		return fail("ec_prj_pt_mul_blind_batch: blinded scalar too long");
	}
	const size_t plen = (size_t)2 * cv->clen;
	const std::vector<HostArr> arrs = {{scalars, nullptr, slen}, {blinds, nullptr, blen}, {points, nullptr, plen}, {nullptr, out, plen}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		if (stage_need(ctx, BL_SCALARS, (size_t)m * outlen) || stage_need(ctx, BL_BAD, m)) {
			return -1;
		}
		EcamdBlindArgs B;
		B.m = ip[0];
		B.b = ip[1];
		B.out = ctx->stage[BL_SCALARS];
		B.bad = ctx->stage[BL_BAD];
		B.n = m;
		B.mlen = slen;
		B.blen = blen;
		B.outlen = outlen;
		B.owords = ow;
		for (uint32_t w = 0; w < 18; w++) {
			B.order[w] = w < cv->order.size() ? cv->order[w] : 0u;
		}
		HIPCHK(ecamd_launch_blind_scalar(B, s));
		if (smul_dev_locked(ctx, cv, m, ctx->stage[BL_SCALARS], outlen, ip[2], op[3], op[4], s)) {
			return -1;
		}
		// a blind outside [1, #E) is not something the reference would have drawn: report it as an error of the item
		HIPCHK(ecamd_launch_status_or(op[4], ctx->stage[BL_BAD], op[3], (uint32_t)plen, m, s));
		return 0;
	});
}

// ------------------------------------------------------------------------------------------
// batched prj_pt_add / prj_pt_dbl
// ------------------------------------------------------------------------------------------
static int pt_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *p1, const uint8_t *p2,
		    uint8_t *out, uint8_t *status, int dbl)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!p1 || (!dbl && !p2) || !out || !status))) {
		return fail("ec_prj_pt_add/dbl_batch: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: stages by hand on the context's stream, and sizes its slots before the scope opens
	HIPCHK(hipSetDevice(ctx->device));
	const size_t plen = (size_t)2 * cv->clen;
	if (stage_need(ctx, HW_IN0, (size_t)n * plen) ||
	    stage_need(ctx, HW_IN1, (size_t)n * plen) ||
	    stage_need(ctx, HW_OUT, (size_t)n * plen) ||
	    stage_need(ctx, HW_STATUS, (size_t)n)) {
		return -1;
	}
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	HIPCHK(hipMemcpyAsync(ctx->stage[HW_IN0], p1, (size_t)n * plen, hipMemcpyHostToDevice, s));
	if (!dbl) {
		HIPCHK(hipMemcpyAsync(ctx->stage[HW_IN1], p2, (size_t)n * plen, hipMemcpyHostToDevice, s));
	}
	EcamdPtArgs A;
	A.p1 = ctx->stage[HW_IN0];
	A.p2 = ctx->stage[HW_IN1];
	A.out = ctx->stage[HW_OUT];
	A.status = ctx->stage[HW_STATUS];
	A.n = n;
	A.clen = (uint32_t)cv->clen;
	A.dbl = dbl;
	A.slot = cv->slot;
	HIPCHK(ecamd_launch_pt(cv->nw, A, s));
	HIPCHK(hipMemcpyAsync(out, ctx->stage[HW_OUT], (size_t)n * plen, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(status, ctx->stage[HW_STATUS], (size_t)n, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

extern "C" int ec_prj_pt_add_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *p1,
				   const uint8_t *p2, uint8_t *out, uint8_t *status)
{
	return pt_batch(ctx, cv, n, p1, p2, out, status, 0);
}

extern "C" int ec_prj_pt_dbl_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *p,
				   uint8_t *out, uint8_t *status)
{
	return pt_batch(ctx, cv, n, p, nullptr, out, status, 1);
}

// ------------------------------------------------------------------------------------------
// Round 4: prj_pt_add / prj_pt_dbl / prj_pt_is_on_curve in either wire format (k_ptf), and _prj_pt_unprotected_mult /
// check_prj_pt_order statement for statement (k_unprot) -- SURVEY.md 8a rows a17, a18, a21, a22 as callable batch operations
// ------------------------------------------------------------------------------------------
extern "C" int ec_prj_pt_op_batch_fmt(ecamd_ctx *ctx, const ecamd_curve *cv, int op, uint32_t n, const uint8_t *p1, const uint8_t *p2,
				      int in_fmt, uint8_t *out, int out_fmt, uint8_t *status)
{
	const bool two = op == ECAMD_PT_OP_ADD || op == ECAMD_PT_OP_CMP || op == ECAMD_PT_OP_EQ_OR_OPP;
	if (!ctx || !cv || cv->ctx != ctx || op < 0 || op > ECAMD_PT_OP_EQ_OR_OPP || (in_fmt != 0 && in_fmt != 1) ||
	    (out_fmt != 0 && out_fmt != 1) || (n && (!p1 || (two && !p2) || (op != ECAMD_PT_OP_ON_CURVE && !out) || !status))) {
		return fail("ec_prj_pt_op_batch_fmt: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: stages by hand on the context's stream, and sizes its slots before the scope opens
	HIPCHK(hipSetDevice(ctx->device));
	// the two predicates hand back one byte per item, the other operations a point
	const size_t iw = (size_t)(in_fmt ? 3 : 2) * cv->clen, ow = op >= ECAMD_PT_OP_CMP ? 1 : (size_t)(out_fmt ? 3 : 2) * cv->clen;
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		if (stage_need(ctx, HW_IN0, (size_t)m * iw) || stage_need(ctx, HW_IN1, (size_t)m * iw) ||
		    stage_need(ctx, HW_OUT, (size_t)m * ow) || stage_need(ctx, HW_STATUS, (size_t)m)) {
			return -1;
		}
		HIPCHK(hipMemcpyAsync(ctx->stage[HW_IN0], p1 + (size_t)off * iw, (size_t)m * iw, hipMemcpyHostToDevice, s));
		if (two) {
			HIPCHK(hipMemcpyAsync(ctx->stage[HW_IN1], p2 + (size_t)off * iw, (size_t)m * iw, hipMemcpyHostToDevice, s));
		}
		EcamdPtfArgs A;
		memset(&A, 0, sizeof(A));
		A.p1 = ctx->stage[HW_IN0];
		A.p2 = ctx->stage[HW_IN1];
		A.out = ctx->stage[HW_OUT];
		A.status = ctx->stage[HW_STATUS];
		A.n = m;
		A.clen = (uint32_t)cv->clen;
		A.op = op;
		A.in_fmt = in_fmt;
		A.out_fmt = out_fmt;
		A.slot = cv->slot;
		HIPCHK(ecamd_launch_ptf(cv->nw, A, s));
		if (op != 2) {
			HIPCHK(hipMemcpyAsync(out + (size_t)off * ow, ctx->stage[HW_OUT], (size_t)m * ow, hipMemcpyDeviceToHost, s));
		}
		HIPCHK(hipMemcpyAsync(status + off, ctx->stage[HW_STATUS], (size_t)m, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		return 0;
	});
}

extern "C" int ec_prj_pt_unprotected_mult_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *scalars,
						uint32_t scalar_len, uint32_t scalar_stride, const uint8_t *points, int in_fmt, uint8_t *out,
						int out_fmt, uint8_t *status)
{
	if (!ctx || !cv || cv->ctx != ctx || (in_fmt != 0 && in_fmt != 1) || (out_fmt != 0 && out_fmt != 1) || scalar_len == 0 ||
	    scalar_len > 4096 || (scalar_stride != 0 && scalar_stride != scalar_len) || (n && (!scalars || !points || !out || !status))) {
		return fail("ec_prj_pt_unprotected_mult_batch: bad argument (scalar_stride is scalar_len, or 0 for one scalar for every item)");
	}
	if (n == 0) {
		return 0;
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: stages by hand on the context's stream, and sizes its slots before the scope opens
	HIPCHK(hipSetDevice(ctx->device));
	const size_t iw = (size_t)(in_fmt ? 3 : 2) * cv->clen, ow = (size_t)(out_fmt ? 3 : 2) * cv->clen;
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
		const size_t sbytes = scalar_stride ? (size_t)m * scalar_len : (size_t)scalar_len;
		if (stage_need(ctx, HW_IN0, (size_t)m * iw) || stage_need(ctx, HW_IN1, sbytes) ||
		    stage_need(ctx, HW_OUT, (size_t)m * ow) || stage_need(ctx, HW_STATUS, (size_t)m)) {
			return -1;
		}
		HIPCHK(hipMemcpyAsync(ctx->stage[HW_IN0], points + (size_t)off * iw, (size_t)m * iw, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(ctx->stage[HW_IN1], scalars + (size_t)off * scalar_stride, sbytes, hipMemcpyHostToDevice, s));
		EcamdUnprotArgs A;
		memset(&A, 0, sizeof(A));
		A.points = ctx->stage[HW_IN0];
		A.scalars = ctx->stage[HW_IN1];
		A.out = ctx->stage[HW_OUT];
		A.status = ctx->stage[HW_STATUS];
		A.n = m;
		A.clen = (uint32_t)cv->clen;
		A.slen = scalar_len;
		A.sstride = scalar_stride;
		A.in_fmt = in_fmt;
		A.out_fmt = out_fmt;
		A.slot = cv->slot;
		HIPCHK(ecamd_launch_unprot(cv->nw, A, s));
		HIPCHK(hipMemcpyAsync(out + (size_t)off * ow, ctx->stage[HW_OUT], (size_t)m * ow, hipMemcpyDeviceToHost, s));
		HIPCHK(hipMemcpyAsync(status + off, ctx->stage[HW_STATUS], (size_t)m, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		return 0;
	});
}

// ------------------------------------------------------------------------------------------
// batched field ops on libecc's 64-bit limb layout
// ------------------------------------------------------------------------------------------
extern "C" int ec_fp_op_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int op, uint32_t n, const uint64_t *a,
			      const uint64_t *b, uint64_t *out)
{
	if (!ctx || !cv || cv->ctx != ctx || op < 0 || op > 4 || (n && (!a || !b || !out))) {
		return fail("ec_fp_op_batch: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: stages by hand on the context's stream, and sizes its slots before the scope opens
	HIPCHK(hipSetDevice(ctx->device));
	const uint32_t nl = (uint32_t)(cv->pbits + 63) / 64;
	const size_t bytes = (size_t)n * nl * 8;
	if (stage_need(ctx, HW_IN0, bytes) || stage_need(ctx, HW_IN1, bytes) ||
	    stage_need(ctx, HW_OUT, bytes)) {
		return -1;
	}
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	HIPCHK(hipMemcpyAsync(ctx->stage[HW_IN0], a, bytes, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(ctx->stage[HW_IN1], b, bytes, hipMemcpyHostToDevice, s));
	EcamdFpArgs A;
	A.a = (const uint32_t *)ctx->stage[HW_IN0];
	A.b = (const uint32_t *)ctx->stage[HW_IN1];
	A.out = (uint32_t *)ctx->stage[HW_OUT];
	A.n = n;
	A.wstride = 2 * nl;
	A.op = op;
	A.slot = cv->slot;
	HIPCHK(ecamd_launch_fp(cv->nw, A, s));
	HIPCHK(hipMemcpyAsync(out, ctx->stage[HW_OUT], bytes, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// ------------------------------------------------------------------------------------------
// batched ECDSA verification (digest supplied by the caller)
// ------------------------------------------------------------------------------------------
// `alg` (SIG_ECDSA, or ECAMD_SIG_ECGDSA / ECRDSA / SM2) selects the front end of the three verification paths below; for the
// three other schemes the back ends compare W'.x with the front end's comparison target (ST_TARGET, in the layout of a signature
// array) instead of the caller's signatures.  ECDSA: exactly the launches there were before `alg` existed.
static const uint8_t *sig_target(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *d_sig, uint8_t **target)
{
	*target = nullptr;
	if (alg == SIG_ECDSA) {
		return d_sig;
	}
	if (stage_need(ctx, ST_TARGET, (size_t)n * 2 * cv->qlen)) {
		return nullptr;
	}
	*target = ctx->stage[ST_TARGET];
	return ctx->stage[ST_TARGET];
}
// ------------------------------------------------------------------------------------------
// W' = [u]G + [v]Y, the body of every verification but EdDSA's and of public-key recovery, in the ST_ frame: the caller's prep
// kernel has left u in ST_U, v in ST_V and its flag byte in ST_FLAGS.  Only enqueues; PublicScalars is the caller's.
// ------------------------------------------------------------------------------------------
// the slots both halves below work in, for chunks of `chunk` items; ST_SUB and up are sized by the callers, whose uses differ
static int two_mul_need(ecamd_ctx *ctx, const ecamd_curve *cv, size_t chunk)
{
	const size_t plen = (size_t)2 * cv->clen, ql = (size_t)cv->qlen;
	return stage_need(ctx, {{ST_U, chunk * ql}, {ST_V, chunk * ql}, {ST_A, chunk * plen}, {ST_B, chunk * plen}, {ST_STA, chunk}, {ST_STB, chunk},
				{ST_FLAGS, chunk}});
}

// A = [u]G into ST_A / ST_STA and B = [v]Y into ST_B / ST_STB: two independent prj_pt_mul, as in the reference (sig/ecdsa_common.c:788,793).
// d_Y == NULL: every Y is the point at infinity, B is not computed.
// subgroup: Y is a public key.  On a curve with a cofactor ec_pub_key_import_from_aff_buf also requires [q]Y == infinity
// (sig/ec_key.c:199-205): one more pass with the broadcast scalar q (it sits behind the generator in HBM) into ST_QY / ST_SUB, and
// a key outside the subgroup becomes an import error (status 1) in ST_STB for the final stage, on the device.
// d_only: a status array; only the items marked ECAMD_STATUS_REDO in it are computed (by the complete-formula kernel), the others
// keep what they have.
static int two_mul_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t m, const uint8_t *d_Y, bool subgroup, const uint8_t *d_only, hipStream_t s)
{
	uint8_t **S = ctx->stage;
	const size_t plen = (size_t)2 * cv->clen;
	const uint32_t ql = (uint32_t)cv->qlen;
	const bool redo = d_only != nullptr;
	if (redo) {
		// the marks select the lanes of the complete-formula kernel (A.only_redo)
		HIPCHK(hipMemcpyAsync(S[ST_STA], d_only, m, hipMemcpyDeviceToDevice, s));
		HIPCHK(hipMemcpyAsync(S[ST_STB], d_only, m, hipMemcpyDeviceToDevice, s));
	}
	if (smul_dev_locked(ctx, cv, m, S[ST_U], ql, nullptr, S[ST_A], S[ST_STA], s, 0xffffffffu, redo)) {
		return -1;
	}
	if (!d_Y) {
		HIPCHK(hipMemsetAsync(S[ST_B], 0, m * plen, s));
		HIPCHK(hipMemsetAsync(S[ST_STB], 2, m, s));
		return 0;
	}
	if (smul_dev_locked(ctx, cv, m, S[ST_V], ql, d_Y, S[ST_B], S[ST_STB], s, 0xffffffffu, redo)) {
		return -1;
	}
	if (subgroup && big_cmp(cv->order, cv->q) != 0) {
		if (redo) {
			HIPCHK(hipMemcpyAsync(S[ST_SUB], d_only, m, hipMemcpyDeviceToDevice, s));
		}
		if (smul_dev_locked(ctx, cv, m, cv->d_gen + plen, ql, d_Y, S[ST_QY], S[ST_SUB], s, 0, redo)) {
			return -1;
		}
		// ST_SUB holds 2 (infinity) for keys in the subgroup; anything else rejects: fold into stB
		// (redo pass: items that were not marked keep their old result byte there, and the final stage skips them)
		HIPCHK(ecamd_launch_status_require(S[ST_STB], S[ST_SUB], 2, m, s));
	}
	return 0;
}

// The two multiplications, then W' = A + B as affine bytes into out1 / st1: k_recover_fin, one shared inversion per eight items, and
// k_recover_redo, the items with A or B at infinity or x_A = x_B on the complete formulas (nothing marked: a near-empty launch).
// The kernels also write A - B into out2 / st2: recovery's second key; the verifications pass the sinks ST_WSINK / ST_STWSINK and
// never read them.  d_yst: a second byte per item that, like ST_FLAGS, says "no sum for this item" when it is not zero.
static int two_mul_sum_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t m, const uint8_t *d_Y, bool subgroup, const uint8_t *d_yst,
			   uint8_t *out1, uint8_t *out2, uint8_t *st1, uint8_t *st2, hipStream_t s)
{
	if (two_mul_dev(ctx, cv, m, d_Y, subgroup, nullptr, s)) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	EcamdRecoverFinArgs F;
	F.A = S[ST_A];
	F.stA = S[ST_STA];
	F.B = S[ST_B];
	F.stB = S[ST_STB];
	F.flags = S[ST_FLAGS];
	F.yst = d_yst;
	F.out1 = out1;
	F.out2 = out2;
	F.st1 = st1;
	F.st2 = st2;
	F.n = m;
	F.clen = (uint32_t)cv->clen;
	F.slot = cv->slot;
	HIPCHK(ecamd_launch_recover_fin(cv->nw, F, s));
	HIPCHK(ecamd_launch_recover_redo(cv->nw, F, s));
	return 0;
}
// the verifications: a public key, W' into ST_W / ST_STW
int ecamd_host::verify_sum_need(ecamd_ctx *ctx, const ecamd_curve *cv, size_t chunk)
{
	const size_t plen = (size_t)2 * cv->clen;
	return two_mul_need(ctx, cv, chunk) || stage_need(ctx, {{ST_SUB, chunk}, {ST_QY, chunk * plen + 256}, {ST_W, chunk * plen},
							       {ST_WSINK, chunk * plen}, {ST_STW, chunk}, {ST_STWSINK, chunk}});
}
int ecamd_host::verify_sum_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t m, const uint8_t *d_Y, hipStream_t s)
{
	uint8_t **S = ctx->stage;
	return two_mul_sum_dev(ctx, cv, m, d_Y, true, S[ST_FLAGS], S[ST_W], S[ST_WSINK], S[ST_STW], S[ST_STWSINK], s);
}

// The mod-q algebra in front of a verification: on the dense radix-2^29 unit of the order's size when the handle has q in a slot
// there (round 4: k_ecdsa_prep_g, sixteen items per inversion from 320 bits on, eight below), else on the saturated words.
// The caller has sized ctx->prep_scratch (prep_scratch_ok).
static bool prep_g29(const ecamd_curve *cv)
{
	return cv->gqslot >= 0 && getenv("ECAMD_NO_PREP_G29") == nullptr;
}
static int prep_scratch_ok(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n)
{
	if (!prep_g29(cv)) {
		return 0;
	}
	return ensure(&ctx->prep_scratch, &ctx->prep_scratch_bytes, (size_t)n * (size_t)ecamd_g29_nl(big_bitlen(cv->q), 0) * 4);
}
// alg != SIG_ECDSA: the front end of ECGDSA / ECRDSA / SM2 (k_sig_prep, saturated words), which also writes the comparison target
static hipError_t launch_ecdsa_prep(ecamd_ctx *ctx, const ecamd_curve *cv, const EcamdEcdsaPrepArgs &P, hipStream_t s, int alg = SIG_ECDSA,
				    uint8_t *target = nullptr)
{
	if (alg != SIG_ECDSA) {
		EcamdSigPrepArgs SP;
		SP.p = P;
		SP.target = target;
		SP.alg = alg;
		return ecamd_launch_sig_prep(cv->qnw, SP, s);
	}
	if (prep_g29(cv) && ctx->prep_scratch) {
		const int qbits = big_bitlen(cv->q);
		static const int kp_env = getenv("ECAMD_PREP_KP") ? atoi(getenv("ECAMD_PREP_KP")) : 0;   // A/B hook
		const int kp = (kp_env >= 1 && kp_env <= 64) ? kp_env : (qbits > 320 ? 16 : 8);
		return ecamd_g29_ecdsa_prep(qbits, cv->gqslot, P, (uint32_t *)ctx->prep_scratch, kp, s);
	}
	return ecamd_launch_ecdsa_prep(cv->qnw, P, s);
}

// ECDSA the reference's way: two independent scalar multiplications and one addition per item (k_ecdsa_fin: x mod q == r over the
// candidates r + j q < p).  All pointers are device pointers.
// d_pub == NULL: every public key is the point at infinity (libecc imports (0 : 1 : 0) as a key, and its verification
// then computes W' = uG + v*infinity = uG, sig/ecdsa_common.c:788-800): [u2]Y is not computed and W' = [u1]G.
// d_only (may be d_res itself): a status array; only the items marked ECAMD_STATUS_REDO in it are verified (by the complete-formula
// kernel) and get a result -- the redo pass of the interleaved secp256r1 loop, entirely on the device.  Only enqueues.
static int ecdsa_two_smul_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_pub,
			      const uint8_t *d_sig, const uint8_t *d_dig, uint32_t hlen, uint8_t *d_res, hipStream_t s,
			      const uint8_t *d_only = nullptr, int alg = SIG_ECDSA)
{
	if (n > ctx->max_chunk) {  // bound the scratch: pieces of max_chunk items, in order on the stream
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return ecdsa_two_smul_dev(ctx, cv, m, d_pub ? d_pub + (size_t)off * 2 * cv->clen : nullptr, d_sig + (size_t)off * 2 * cv->qlen,
						  d_dig + (size_t)off * hlen, hlen, d_res + off, s, d_only ? d_only + off : nullptr, alg);
		});
	}
	const size_t plen = (size_t)2 * cv->clen;
	PublicScalars pub_scope(ctx);   // u1, u2 and the group order are public
	if (two_mul_need(ctx, cv, n) || stage_need(ctx, {{ST_SUB, n}, {ST_QY, n * plen + 256}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	EcamdEcdsaPrepArgs P;
	P.sigs = d_sig;
	P.digests = d_dig;
	P.u1 = S[ST_U];
	P.u2 = S[ST_V];
	P.flags = S[ST_FLAGS];
	P.n = n;
	P.qlen = (uint32_t)cv->qlen;
	P.hlen = hlen;
	P.qbits = (uint32_t)cv->qbits;
	P.qslot = cv->qslot;
	P.only = d_only;
	uint8_t *target;
	const uint8_t *cmp_sig = sig_target(ctx, cv, alg, n, d_sig, &target);
	if (!cmp_sig || prep_scratch_ok(ctx, cv, n)) {
		return -1;
	}
	HIPCHK(launch_ecdsa_prep(ctx, cv, P, s, alg, target));
	if (two_mul_dev(ctx, cv, n, d_pub, true, d_only, s)) {
		return -1;
	}
	EcamdEcdsaFinArgs Fn;
	Fn.A = S[ST_A];
	Fn.stA = S[ST_STA];
	Fn.B = S[ST_B];
	Fn.stB = S[ST_STB];
	Fn.sigs = cmp_sig;
	Fn.flags = S[ST_FLAGS];
	Fn.result = d_res;
	Fn.n = n;
	Fn.clen = (uint32_t)cv->clen;
	Fn.qlen = (uint32_t)cv->qlen;
	Fn.jmax = cv->jmax;
	for (int w = 0; w < 17; w++) {
		Fn.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
	}
	Fn.slot = cv->slot;
	Fn.only = d_only;
	HIPCHK(ecamd_launch_ecdsa_fin(cv->nw, Fn, s));
	return 0;
}

// k_ecdsa_prep of a chunk on the side stream: it starts when everything enqueued on s so far is done (the stage buffers it
// writes are read by the previous chunk's loop) and the caller makes the consumer of u1 / u2 wait for side_done.
// Returns the event to wait for, or nullptr when the kernel was enqueued on s itself.
static hipEvent_t ecdsa_prep_beside(ecamd_ctx *ctx, const ecamd_curve *cv, const EcamdEcdsaPrepArgs &P, hipStream_t s, hipError_t *err,
				    int alg = SIG_ECDSA, uint8_t *target = nullptr)
{
	if (!ctx->side_ok) {
		*err = launch_ecdsa_prep(ctx, cv, P, s, alg, target);
		return nullptr;
	}
	*err = hipEventRecord(ctx->side_fork, s);
	if (*err == hipSuccess) {
		*err = hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0);
	}
	if (*err == hipSuccess) {
		*err = launch_ecdsa_prep(ctx, cv, P, ctx->side_stream, alg, target);
	}
	if (*err == hipSuccess) {
		*err = hipEventRecord(ctx->side_done, ctx->side_stream);
	}
	return ctx->side_done;
}

// device pointers in and out; only enqueues on s
// The fused double-scalar loop of the generic radix-2^29 units (k_loop_g then k_comb_add_g): curves on the affine-table pipeline (every
// flavour but the two nine-limb ones), prime-order groups (no subgroup check of the key to run beside it), u1 within the comb
// table's reach, and a comb table of the generator (built on the first batch of at least comb_min_batch items).
static bool fused_verify_ok(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n)
{
	if (cv->is_p256 || cv->gslot < 0 || getenv("ECAMD_NO_FUSED_VERIFY") != nullptr) {
		return false;
	}
	if (!(cv->gflavour == 0 || cv->gflavour == 1 || cv->gflavour == 3 || cv->gflavour == 5 || cv->gflavour == 6 || cv->gflavour == 7)) {
		return false;
	}
	if (big_cmp(cv->order, cv->q) != 0 || (uint32_t)cv->qlen > ecamd_g29_comb_max_slen(cv->pbits)) {
		return false;
	}
	{
		PublicScalars pub_scope(ctx);
		maybe_build_comb(ctx, const_cast<ecamd_curve *>(cv), n);
	}
	return cv->d_comb != nullptr;
}

// W' = [u1]G + [u2]Q by ONE window loop over Q's affine table plus 2 NW + 1 comb additions for G, for every field size (the
// reference: two prj_pt_mul and a prj_pt_add, sig/ecdsa_common.c:786-796); the affine W' then meets the same final stage as the
// two-multiplication path (x mod q == r over the candidates r + j q < p).  Items whose loop met an exceptional pair come back
// marked and are verified again by ecdsa_two_smul_dev (complete formulas), entirely on the device.
static int ecdsa_fused_g_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_pub, const uint8_t *d_sig,
			     const uint8_t *d_dig, uint32_t hlen, uint8_t *d_res, hipStream_t s, int alg = SIG_ECDSA)
{
	const size_t plen = (size_t)2 * cv->clen, ql = (size_t)cv->qlen;
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	PublicScalars pub_scope(ctx);
	uint8_t *target;
	if (!sig_target(ctx, cv, alg, chunk, d_sig, &target)) {
		return -1;
	}
	// ST_A / ST_STA: the affine W' and its status; ST_STB says "the other point is infinity" for the final stage
	if (stage_need(ctx, {{ST_U, chunk * ql}, {ST_V, chunk * ql}, {ST_A, chunk * plen}, {ST_STA, chunk}, {ST_STB, chunk}, {ST_FLAGS, chunk}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	for (uint32_t off = 0; off < n; off += chunk) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		EcamdEcdsaPrepArgs P;
		P.sigs = d_sig + (size_t)off * 2 * ql;
		P.digests = d_dig + (size_t)off * hlen;
		P.u1 = S[ST_U];
		P.u2 = S[ST_V];
		P.flags = S[ST_FLAGS];
		P.n = m;
		P.qlen = (uint32_t)cv->qlen;
		P.hlen = hlen;
		P.qbits = (uint32_t)cv->qbits;
		P.qslot = cv->qslot;
		P.only = nullptr;
		// (on s itself: k_table_g already reads the scalars -- it stores their recoding beside the window table -- so there is
		// nothing for this kernel to run beside; the secp256r1 path below does overlap it)
		if (prep_scratch_ok(ctx, cv, m)) {
			return -1;
		}
		HIPCHK(launch_ecdsa_prep(ctx, cv, P, s, alg, target));
		if (smul_dev_locked(ctx, cv, m, S[ST_V], (uint32_t)ql, d_pub + (size_t)off * plen, S[ST_A], S[ST_STA], s, 0xffffffffu, false, S[ST_U])) {
			return -1;
		}
		HIPCHK(hipMemsetAsync(S[ST_STB], 2, m, s));
		EcamdEcdsaFinArgs Fn;
		Fn.A = S[ST_A];
		Fn.stA = S[ST_STA];
		Fn.B = S[ST_A];            // never read: its status says infinity
		Fn.stB = S[ST_STB];
		Fn.sigs = target ? target : d_sig + (size_t)off * 2 * ql;
		Fn.flags = S[ST_FLAGS];
		Fn.result = d_res + off;
		Fn.n = m;
		Fn.clen = (uint32_t)cv->clen;
		Fn.qlen = (uint32_t)cv->qlen;
		Fn.jmax = cv->jmax;
		for (int w = 0; w < 17; w++) {
			Fn.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
		}
		Fn.slot = cv->slot;
		Fn.only = nullptr;
		HIPCHK(ecamd_launch_ecdsa_fin(cv->nw, Fn, s));
	}
	// the redo pass: only the marked items (with nothing marked: near-empty launches)
	return ecdsa_two_smul_dev(ctx, cv, n, d_pub, d_sig, d_dig, hlen, d_res, s, d_res, alg);
}

int ecamd_host::ecdsa_verify_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_pub,
				   const uint8_t *d_sig, const uint8_t *d_dig, uint32_t hlen, uint8_t *d_res, hipStream_t s,
				   const Between *between, int alg)
{
	if (!cv->is_p256 || !cv->d_gtab) {
		if (fused_verify_ok(ctx, cv, n) ? ecdsa_fused_g_dev(ctx, cv, n, d_pub, d_sig, d_dig, hlen, d_res, s, alg)
						: ecdsa_two_smul_dev(ctx, cv, n, d_pub, d_sig, d_dig, hlen, d_res, s, nullptr, alg)) {
			return -1;
		}
		if (between && (*between)()) {
			return -1;
		}
		return 0;
	}
	// secp256r1: interleaved [u1]G + [u2]Q loop (ecamd_launch_verify_p256), in chunks
	PublicScalars pub_scope(ctx);   // everything a verification multiplies by is public
	maybe_build_comb(ctx, const_cast<ecamd_curve *>(cv), n);
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	{
		uint8_t *t = (uint8_t *)ctx->tbl_fast;
		const int rc = ensure(&t, &ctx->tbl_fast_bytes, (size_t)((chunk + 63u) & ~63u) * P256_SCRATCH_PER_ITEM);
		ctx->tbl_fast = (uint32_t *)t;
		if (rc) {
			return -1;
		}
	}
	uint8_t *target;
	if (!sig_target(ctx, cv, alg, chunk, d_sig, &target)) {
		return -1;
	}
	if (stage_need(ctx, {{ST_U, (size_t)chunk * 32}, {ST_V, (size_t)chunk * 32}, {VP_FLAGS, chunk}, {VP_KEYS, (size_t)chunk * 64 + chunk}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	for (uint32_t off = 0; off < n; off += chunk) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		EcamdEcdsaPrepArgs P;
		P.sigs = d_sig + (size_t)off * 64;
		P.digests = d_dig + (size_t)off * hlen;
		P.u1 = S[ST_U];
		P.u2 = S[ST_V];
		P.flags = S[VP_FLAGS];
		P.n = m;
		P.qlen = 32;
		P.hlen = hlen;
		P.qbits = (uint32_t)cv->qbits;
		P.qslot = cv->qslot;
		P.only = nullptr;
		hipError_t perr = hipSuccess;
		if (prep_scratch_ok(ctx, cv, m)) {
			return -1;
		}
		const hipEvent_t prep_done = ecdsa_prep_beside(ctx, cv, P, s, &perr, alg, target);
		HIPCHK(perr);
		EcamdSmulArgs K;
		memset(&K, 0, sizeof(K));
		K.points = d_pub + (size_t)off * 64;
		K.pstride = 64;
		K.out = S[VP_KEYS];           // zeroed for rejected keys; otherwise unused
		K.status = S[VP_KEYS] + (size_t)m * 64;
		K.tbl = ctx->tbl_fast;
		K.stg = ctx->tbl_fast + (size_t)((chunk + 63u) & ~63u) * (P256_TAB_BYTES / 4);
		K.n = m;
		K.clen = 32;
		K.slot = cv->slot;
		hipEvent_t *dom = (ctx->timing && off == 0) ? ctx->ev_dom : nullptr;
		HIPCHK(ecamd_launch_verify_p256(K, S[ST_U], S[ST_V], target ? target : d_sig + (size_t)off * 64, S[VP_FLAGS],
						cv->d_comb ? cv->d_comb : cv->d_gtab, cv->d_comb ? 1 : 0, cv->qdig, d_res + off, s, dom, prep_done));
		ctx->ev_dom_valid = ctx->ev_dom_valid || (dom != nullptr);
	}
	// exceptional pairs inside the interleaved loop (never for honest signatures) come back as ECAMD_STATUS_REDO: those
	// items are verified again the reference's way -- two complete-formula multiplications -- by kernels whose other
	// lanes exit at once (with nothing marked: five near-empty launches)
	if (ecdsa_two_smul_dev(ctx, cv, n, d_pub, d_sig, d_dig, hlen, d_res, s, d_res, alg)) {
		return -1;
	}
	if (between && (*between)()) {
		return -1;
	}
	return 0;
}

static int ecdsa_verify_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *a,
				const void *b, const void *c, const void *d, uint32_t hlen)
{
	static thread_local char msg[160];
	if (!ctx || !cv || cv->ctx != ctx || (n && (!a || !b || !c || !d))) {
		snprintf(msg, sizeof(msg), "%s: bad argument", fn);
		return fail(msg);
	}
	if (cv->qslot < 0) {
		snprintf(msg, sizeof(msg), "%s: generator order not supported for this curve", fn);
		return fail(msg);
	}
	if (hlen == 0 || hlen > 128) {
		snprintf(msg, sizeof(msg), "%s: digest length must be in 1..128", fn);
		return fail(msg);
	}
	return 0;
}

extern "C" int ec_ecdsa_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *d_pubkeys,
					 const void *d_sigs, const void *d_digests, uint32_t hlen, void *d_result,
					 void *hip_stream)
{
	if (ecdsa_verify_args_ok("ec_ecdsa_verify_batch_dev", ctx, cv, n, d_pubkeys, d_sigs, d_digests, d_result, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return ecdsa_verify_dev_locked(ctx, cv, n, (const uint8_t *)d_pubkeys, (const uint8_t *)d_sigs,
					       (const uint8_t *)d_digests, hlen, (uint8_t *)d_result, s);
	});
}

// Messages instead of digests (round 4): `data` then holds one fixed-stride SLOT per item -- a little-endian u32 length and the
// message bytes (ecamd_hash.hip) -- and the digests H(m) are computed on the device (hash_type: libecc's hash_alg_type numbers,
// SHA224 = 1 ... SHA512 = 4) into ST_DIGESTS before the verification core runs; dig_out (host, n x digest length, may be NULL)
// receives them for the callers that need a digest on the host again.
int ecamd_host::ecdsa_hash_stage(ecamd_ctx *ctx, int hash_type, uint32_t m, const uint8_t *d_slots, uint32_t stride, uint32_t dlen, hipStream_t s)
{
	if (stage_need(ctx, ST_DIGESTS, (size_t)m * dlen)) {
		return -1;
	}
	if (hash_type == 5) {
		HIPCHK(ecamd_launch_shake256_slots(d_slots, stride, m, ctx->stage[ST_DIGESTS], dlen, dlen, s));   // SHAKE256, dlen octets of output
	} else {
		HIPCHK(ecamd_launch_sha2_slots(hash_type, d_slots, stride, m, ctx->stage[ST_DIGESTS], dlen, s));
	}
	return 0;
}

static int ecdsa_verify_host_aff(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
				 const uint8_t *data, uint32_t data_stride, int hash_type, uint32_t hlen, uint8_t *result, const char *fn)
{
	if (ecdsa_verify_args_ok(fn, ctx, cv, n, pubkeys, sigs, data, result, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t plen = (size_t)2 * cv->clen, slen2 = (size_t)2 * cv->qlen;
	const std::vector<HostArr> arrs = {{pubkeys, nullptr, plen}, {sigs, nullptr, slen2}, {data, nullptr, data_stride}, {nullptr, result, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &between) {
		const uint8_t *d_dig = ip[2];
		if (hash_type) {
			if (ecdsa_hash_stage(ctx, hash_type, m, ip[2], data_stride, hlen, s)) {
				return -1;
			}
			d_dig = ctx->stage[ST_DIGESTS];
		}
		return ecdsa_verify_dev_locked(ctx, cv, m, ip[0], ip[1], d_dig, hlen, op[3], s, &between);
	});
}

extern "C" int ec_ecdsa_verify_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys,
				     const uint8_t *sigs, const uint8_t *digests, uint32_t hlen, uint8_t *result)
{
	return ecdsa_verify_host_aff(ctx, cv, n, pubkeys, sigs, digests, hlen, 0, hlen, result, "ec_ecdsa_verify_batch");
}

// ECDSA verification with the public keys in either point wire format.  ECAMD_PT_PROJECTIVE is what an ec_pub_key holds
// (ec_pub_key_export_to_buf: X || Y || Z of pub_key->y): imported as prj_pt_import_from_buf does, normalised on the device,
// and a key that is the point at infinity -- which libecc imports and verifies against, W' = uG -- is handled as the
// reference does.
static int ecdsa_verify_host_fmt(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys, int pub_fmt, const uint8_t *sigs,
				 const uint8_t *data, uint32_t data_stride, int hash_type, uint32_t hlen, uint8_t *result, const char *fn)
{
	if (pub_fmt == ECAMD_PT_AFFINE) {
		return ecdsa_verify_host_aff(ctx, cv, n, pubkeys, sigs, data, data_stride, hash_type, hlen, result, fn);
	}
	if (pub_fmt != ECAMD_PT_PROJECTIVE) {
		return fail("ec_ecdsa_verify_batch_fmt: point format must be ECAMD_PT_AFFINE or ECAMD_PT_PROJECTIVE");
	}
	if (ecdsa_verify_args_ok(fn, ctx, cv, n, pubkeys, sigs, data, result, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t alen = (size_t)2 * cv->clen, sl = (size_t)2 * cv->qlen;
	std::vector<uint8_t> st(n);
	{
		// keys, signatures and digests go to the device once, chunk by chunk behind the double-buffered staging; the keys are
		// imported and normalised there (k_prj_import) and the verification core consumes the affine form in HBM
		std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the lock is dropped for the host pass over the import status and retaken below
		HIPCHK(hipSetDevice(ctx->device));
		std::vector<HostArr> arrs = {{pubkeys, nullptr, 3 * (size_t)cv->clen}, {sigs, nullptr, sl}, {data, nullptr, data_stride},
					     {nullptr, result, 1}, {nullptr, st.data(), 1}};
		if (host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &between) {
			    if (stage_need(ctx, EF_AFF, (size_t)m * alen)) {
				    return -1;
			    }
			    const uint8_t *d_dig = ip[2];
			    if (hash_type) {
				    if (ecdsa_hash_stage(ctx, hash_type, m, ip[2], data_stride, hlen, s)) {
					    return -1;
				    }
				    d_dig = ctx->stage[ST_DIGESTS];
			    }
			    EcamdPrjInArgs I;
			    I.in = ip[0];
			    I.aff = ctx->stage[EF_AFF];
			    I.pre = op[4];
			    I.n = m;
			    I.clen = (uint32_t)cv->clen;
			    I.for_mul = 0;
			    I.slot = cv->slot;
			    HIPCHK(launch_prj_import(cv, I, s));
			    return ecdsa_verify_dev_locked(ctx, cv, m, ctx->stage[EF_AFF], ip[1], d_dig, hlen, op[3], s, &between);
		    })) {
			return -1;
		}
	}
	std::vector<uint32_t> inf;
	for (uint32_t i = 0; i < n; i++) {
		if (st[i] == ECAMD_ERR) {
			result[i] = 1;
		} else if (st[i] == ECAMD_INF) {
			// (0 : 0 : 0) passes prj_pt_import_from_buf too; the reference's scalar multiplication then fails on it
			bool allzero = true;
			for (size_t b = 0; b < 3 * (size_t)cv->clen && allzero; b++) {
				allzero = pubkeys[(size_t)i * 3 * cv->clen + b] == 0;
			}
			result[i] = 1;
			if (!allzero) {
				inf.push_back(i);
			}
		}
	}
	if (inf.empty()) {
		return 0;
	}
	// keys at infinity: W' = [u1]G.  Their signatures and digests (or message slots, hashed on the device again: the digests of
	// the batch never travel back) are gathered on the host -- a handful of items at most.
	const uint32_t r = (uint32_t)inf.size();
	const size_t dl = hash_type ? (size_t)data_stride : (size_t)hlen;
	std::vector<uint8_t> hs((size_t)r * sl), hd((size_t)r * dl), hr(r);
	for (uint32_t j = 0; j < r; j++) {
		memcpy(&hs[(size_t)j * sl], sigs + (size_t)inf[j] * sl, sl);
		memcpy(&hd[(size_t)j * dl], data + (size_t)inf[j] * dl, dl);
	}
	std::lock_guard<std::mutex> lk(ctx->mu);
	HIPCHK(hipSetDevice(ctx->device));
	if (stage_need(ctx, {{EF_INF_SIGS, (size_t)r * sl}, {EF_INF_DATA, (size_t)r * dl}, {EF_INF_RES, r}})) {
		return -1;
	}
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	uint8_t **S = ctx->stage;
	HIPCHK(hipMemcpyAsync(S[EF_INF_SIGS], hs.data(), hs.size(), hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(S[EF_INF_DATA], hd.data(), hd.size(), hipMemcpyHostToDevice, s));
	const uint8_t *d_dig = S[EF_INF_DATA];
	if (hash_type) {
		if (ecdsa_hash_stage(ctx, hash_type, r, S[EF_INF_DATA], data_stride, hlen, s)) {
			return -1;
		}
		d_dig = S[ST_DIGESTS];
	}
	if (ecdsa_two_smul_dev(ctx, cv, r, nullptr, S[EF_INF_SIGS], d_dig, hlen, S[EF_INF_RES], s)) {
		return -1;
	}
	HIPCHK(hipMemcpyAsync(hr.data(), S[EF_INF_RES], r, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	for (uint32_t j = 0; j < r; j++) {
		result[inf[j]] = hr[j];
	}
	return 0;
}

extern "C" int ec_ecdsa_verify_batch_fmt(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys, int pub_fmt,
					 const uint8_t *sigs, const uint8_t *digests, uint32_t hlen, uint8_t *result)
{
	return ecdsa_verify_host_fmt(ctx, cv, n, pubkeys, pub_fmt, sigs, digests, hlen, 0, hlen, result, "ec_ecdsa_verify_batch_fmt");
}

// ECDSA verification from MESSAGES: item i's message sits in a slot of msg_stride bytes (a multiple of 4, at most 4096): a
// little-endian u32 length, then the bytes (4 + length <= msg_stride); H(m) is SHA-224 / 256 / 384 / 512 (hash_type 1 .. 4,
// libecc's hash_alg_type numbers) computed on the device, the rest is ec_ecdsa_verify_batch_fmt.
extern "C" int ec_ecdsa_verify_msg_batch_fmt(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *pubkeys, int pub_fmt,
					     const uint8_t *sigs, int hash_type, const uint8_t *msg_slots, uint32_t msg_stride, uint8_t *result)
{
	const int dl = ecamd_sha2_digest_len(hash_type);
	if (dl == 0 || msg_stride < 4 || (msg_stride & 3u) || msg_stride > 4096) {
		return fail("ec_ecdsa_verify_msg_batch_fmt: hash_type must be 1 .. 4 (SHA-224 / 256 / 384 / 512), msg_stride a multiple of 4 in 4 .. 4096");
	}
	return ecdsa_verify_host_fmt(ctx, cv, n, pubkeys, pub_fmt, sigs, msg_slots, msg_stride, hash_type, (uint32_t)dl, result,
				     "ec_ecdsa_verify_msg_batch_fmt");
}

// ------------------------------------------------------------------------------------------
// batched ECDSA signing with caller-supplied nonces
// ------------------------------------------------------------------------------------------
// Device core of ECDSA signing: every pointer a device pointer; kG and its status live in SG_KG, SG_STKG.
int ecamd_host::ecdsa_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_privs,
				      const uint8_t *d_nonces, const uint8_t *d_digests, uint32_t hlen, uint8_t *d_sigs,
				      uint8_t *d_status, hipStream_t s)
{
	const size_t plen = (size_t)2 * cv->clen, ql = (size_t)cv->qlen;
	if (n > ctx->max_chunk) {  // bound the scratch: pieces of max_chunk items, in order on the stream
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return ecdsa_sign_dev_locked(ctx, cv, m, d_privs + off * ql, d_nonces + off * ql, d_digests + (size_t)off * hlen,
						     hlen, d_sigs + off * 2 * ql, d_status + off, s);
		});
	}
	if (stage_need(ctx, SG_KG, n * plen) || stage_need(ctx, SG_STKG, n)) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	if (smul_dev_locked(ctx, cv, n, d_nonces, (uint32_t)ql, nullptr, S[SG_KG], S[SG_STKG], s)) {  // kG (:479)
		return -1;
	}
	EcamdEcdsaSignArgs A;
	A.privs = d_privs;
	A.nonces = d_nonces;
	A.digests = d_digests;
	A.kG = S[SG_KG];
	A.stkG = S[SG_STKG];
	A.sigs = d_sigs;
	A.status = d_status;
	A.n = n;
	A.clen = (uint32_t)cv->clen;
	A.qlen = (uint32_t)cv->qlen;
	A.hlen = hlen;
	A.qbits = (uint32_t)cv->qbits;
	A.jmax = cv->jmax;
	A.qslot = cv->qslot;
	HIPCHK(ecamd_launch_ecdsa_sign(cv->qnw, A, s));
	return 0;
}

static int ecdsa_sign_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *a,
			      const void *b, const void *c, const void *d, const void *e, uint32_t hlen)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!a || !b || !c || !d || !e))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->qslot < 0) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	if (hlen == 0 || hlen > 128) {
		return fail(std::string(fn) + ": digest length must be in 1..128");
	}
	return 0;
}

extern "C" int ec_ecdsa_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *d_privs,
				       const void *d_nonces, const void *d_digests, uint32_t hlen, void *d_sigs,
				       void *d_status, void *hip_stream)
{
	if (ecdsa_sign_args_ok("ec_ecdsa_sign_batch_dev", ctx, cv, n, d_privs, d_nonces, d_digests, d_sigs, d_status, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return ecdsa_sign_dev_locked(ctx, cv, n, (const uint8_t *)d_privs, (const uint8_t *)d_nonces, (const uint8_t *)d_digests,
					     hlen, (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_ecdsa_sign_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *privs,
				   const uint8_t *nonces, const uint8_t *digests, uint32_t hlen, uint8_t *sigs,
				   uint8_t *status)
{
	if (ecdsa_sign_args_ok("ec_ecdsa_sign_batch", ctx, cv, n, privs, nonces, digests, sigs, status, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {nonces, nullptr, ql}, {digests, nullptr, hlen},
					   {nullptr, sigs, 2 * ql}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return ecdsa_sign_dev_locked(ctx, cv, m, ip[0], ip[1], ip[2], hlen, op[3], op[4], s);
	});
}

// ------------------------------------------------------------------------------------------
// batched ECGDSA / ECRDSA / SM2 (include/libecc_amd.h: ec_sig_*): the ECDSA verification paths with the scheme's front end
// (k_sig_prep) and the ECDSA signing path with the scheme's back end (k_sig_sign)
// ------------------------------------------------------------------------------------------
int ecamd_host::sig_alg_ok(const char *fn, int alg)
{
	if (alg != ECAMD_SIG_ECGDSA && alg != ECAMD_SIG_ECRDSA && alg != ECAMD_SIG_SM2) {
		return fail(std::string(fn) + ": alg must be ECAMD_SIG_ECGDSA, ECAMD_SIG_ECRDSA or ECAMD_SIG_SM2");
	}
	return 0;
}

extern "C" int ec_sig_verify_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const void *d_pubkeys, const void *d_sigs,
				       const void *d_digests, uint32_t hlen, void *d_result, void *hip_stream)
{
	if (sig_alg_ok("ec_sig_verify_batch_dev", alg) ||
	    ecdsa_verify_args_ok("ec_sig_verify_batch_dev", ctx, cv, n, d_pubkeys, d_sigs, d_digests, d_result, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return ecdsa_verify_dev_locked(ctx, cv, n, (const uint8_t *)d_pubkeys, (const uint8_t *)d_sigs, (const uint8_t *)d_digests, hlen,
					       (uint8_t *)d_result, s, nullptr, alg);
	});
}

extern "C" int ec_sig_verify_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *pubkeys, const uint8_t *sigs,
				   const uint8_t *digests, uint32_t hlen, uint8_t *result)
{
	if (sig_alg_ok("ec_sig_verify_batch", alg) || ecdsa_verify_args_ok("ec_sig_verify_batch", ctx, cv, n, pubkeys, sigs, digests, result, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t plen = (size_t)2 * cv->clen, slen2 = (size_t)2 * cv->qlen;
	const std::vector<HostArr> arrs = {{pubkeys, nullptr, plen}, {sigs, nullptr, slen2}, {digests, nullptr, hlen}, {nullptr, result, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &between) {
		return ecdsa_verify_dev_locked(ctx, cv, m, ip[0], ip[1], ip[2], hlen, op[3], s, &between, alg);
	});
}

// Device core of signing: every pointer a device pointer; [k]G and its status live in SG_KG, SG_STKG as for ECDSA.
int ecamd_host::sig_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *d_privs, const uint8_t *d_nonces,
			       const uint8_t *d_digests, uint32_t hlen, uint8_t *d_sigs, uint8_t *d_status, hipStream_t s)
{
	const size_t plen = (size_t)2 * cv->clen, ql = (size_t)cv->qlen;
	if (n > ctx->max_chunk) {  // bound the scratch: pieces of max_chunk items, in order on the stream
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return sig_sign_dev_locked(ctx, cv, alg, m, d_privs + off * ql, d_nonces + off * ql, d_digests + (size_t)off * hlen, hlen,
						   d_sigs + off * 2 * ql, d_status + off, s);
		});
	}
	if (stage_need(ctx, SG_KG, n * plen) || stage_need(ctx, SG_STKG, n)) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	if (smul_dev_locked(ctx, cv, n, d_nonces, (uint32_t)ql, nullptr, S[SG_KG], S[SG_STKG], s)) {  // [k]G, secret-scalar mode as the context says
		return -1;
	}
	EcamdSigSignArgs A;
	A.a.privs = d_privs;
	A.a.nonces = d_nonces;
	A.a.digests = d_digests;
	A.a.kG = S[SG_KG];
	A.a.stkG = S[SG_STKG];
	A.a.sigs = d_sigs;
	A.a.status = d_status;
	A.a.n = n;
	A.a.clen = (uint32_t)cv->clen;
	A.a.qlen = (uint32_t)cv->qlen;
	A.a.hlen = hlen;
	A.a.qbits = (uint32_t)cv->qbits;
	A.a.jmax = cv->jmax;
	A.a.qslot = cv->qslot;
	A.alg = alg;
	HIPCHK(ecamd_launch_sig_sign(cv->qnw, A, s));
	return 0;
}

extern "C" int ec_sig_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const void *d_privs, const void *d_nonces,
				     const void *d_digests, uint32_t hlen, void *d_sigs, void *d_status, void *hip_stream)
{
	if (sig_alg_ok("ec_sig_sign_batch_dev", alg) ||
	    ecdsa_sign_args_ok("ec_sig_sign_batch_dev", ctx, cv, n, d_privs, d_nonces, d_digests, d_sigs, d_status, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return sig_sign_dev_locked(ctx, cv, alg, n, (const uint8_t *)d_privs, (const uint8_t *)d_nonces, (const uint8_t *)d_digests, hlen,
					   (uint8_t *)d_sigs, (uint8_t *)d_status, s);
	});
}

extern "C" int ec_sig_sign_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int alg, uint32_t n, const uint8_t *privs, const uint8_t *nonces,
				 const uint8_t *digests, uint32_t hlen, uint8_t *sigs, uint8_t *status)
{
	if (sig_alg_ok("ec_sig_sign_batch", alg) || ecdsa_sign_args_ok("ec_sig_sign_batch", ctx, cv, n, privs, nonces, digests, sigs, status, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {nonces, nullptr, ql}, {digests, nullptr, hlen},
					   {nullptr, sigs, 2 * ql}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return sig_sign_dev_locked(ctx, cv, alg, m, ip[0], ip[1], ip[2], hlen, op[3], op[4], s);
	});
}

// ------------------------------------------------------------------------------------------
// Round 4: the secret-key half without libecc's division on the host.  nn_get_random_mod (nn/nn_rand.c:92-150) is get_random for
// 2 * qlen bytes, then a constant-time reduction modulo q - 1 that costs a host thread about a microsecond: more than everything else
// a signature or a key pair needs from the host.  The random bytes stay the application's; the reduction moves to the
// device (k_rand_mod, ecamd_randmod.h), and so does H(m) (k_sha2_slots).
// ------------------------------------------------------------------------------------------
static int rand_mod_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_raw, uint8_t *d_out, hipStream_t s)
{
	(void)ctx;
	EcamdRandModArgs R;
	R.raw = d_raw;
	R.out = d_out;
	R.n = n;
	R.qlen = (uint32_t)cv->qlen;
	R.rawlen = 2 * (uint32_t)cv->qlen;
	for (int w = 0; w < 18; w++) {
		R.q[w] = (size_t)w < cv->q.size() ? cv->q[(size_t)w] : 0;
	}
	HIPCHK(ecamd_launch_rand_mod(cv->qnw, R, s));
	return 0;
}
static int rand_mod_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv)
{
	if (!ctx || !cv || cv->ctx != ctx) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (!(cv->q[0] & 1) || big_bitlen(cv->q) < 2 || !cv->qnw || !ecamd_nw_supported(cv->qnw) || cv->q.size() > 18) {
		return fail(std::string(fn) + ": generator order not supported (odd, at most 544 bits)");
	}
	return 0;
}

extern "C" int ec_nn_random_mod_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *raw, uint8_t *out)
{
	if (rand_mod_args_ok("ec_nn_random_mod_batch", ctx, cv)) {
		return -1;
	}
	if (n && (!raw || !out)) {
		return fail("ec_nn_random_mod_batch: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{raw, nullptr, 2 * ql}, {nullptr, out, ql}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return rand_mod_dev_locked(ctx, cv, m, ip[0], op[1], s);
	});
}

// ECDSA signatures from messages and RAW nonce material: k = nn_get_random_mod's value for the 2 * qlen random bytes of the item,
// h = SHA-2(m) of its message slot (hash_type 1 .. 4; 0: the slots ARE the digests, msg_stride bytes each), then ec_ecdsa_sign_batch.
extern "C" int ec_ecdsa_sign_msg_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *privs, const uint8_t *nonce_raw,
				       int hash_type, const uint8_t *msg_slots, uint32_t msg_stride, uint8_t *sigs, uint8_t *status)
{
	const uint32_t hlen = hash_type ? (uint32_t)ecamd_sha2_digest_len(hash_type) : msg_stride;
	if (hash_type && (hlen == 0 || msg_stride < 4 || (msg_stride & 3u) || msg_stride > 4096)) {
		return fail("ec_ecdsa_sign_msg_batch: hash_type must be 0 (digests) or 1 .. 4 (SHA-224 / 256 / 384 / 512) with a slot stride that is a multiple of 4 in 4 .. 4096");
	}
	if (rand_mod_args_ok("ec_ecdsa_sign_msg_batch", ctx, cv) ||
	    ecdsa_sign_args_ok("ec_ecdsa_sign_msg_batch", ctx, cv, n, privs, nonce_raw, msg_slots, sigs, status, hlen)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {nonce_raw, nullptr, 2 * ql}, {msg_slots, nullptr, msg_stride},
					   {nullptr, sigs, 2 * ql}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		// SG_NONCES: secret (ensure() wipes what it frees, ecamd_ctx_wipe_scratch the rest)
		if (stage_need(ctx, SG_NONCES, (size_t)m * ql) || rand_mod_dev_locked(ctx, cv, m, ip[1], ctx->stage[SG_NONCES], s)) {
			return -1;
		}
		const uint8_t *d_dig = ip[2];
		if (hash_type) {
			if (ecdsa_hash_stage(ctx, hash_type, m, ip[2], msg_stride, hlen, s)) {
				return -1;
			}
			d_dig = ctx->stage[ST_DIGESTS];
		}
		return ecdsa_sign_dev_locked(ctx, cv, m, ip[0], ctx->stage[SG_NONCES], d_dig, hlen, op[3], op[4], s);
	});
}

// ------------------------------------------------------------------------------------------
// deterministic ECDSA (include/libecc_amd.h: ec_rfc6979_nonce_batch, ec_decdsa_sign_batch): the nonce of RFC 6979 section 3.2
// derived on the device (k_rfc6979_nonce, ecamd_rfc6979.hip), then the ECDSA signing core.  Per chunk of at most max_chunk items:
//   k_sha2_slots       in_is_digest = 0: h1 = H(m) into ST_DIGESTS
//   k_rfc6979_nonce    k into SG_NONCES (secret: ensure() wipes what it frees, ecamd_ctx_wipe_scratch the rest); a slot whose length
//                      does not fit gets k = 0
//   ecdsa_sign_dev_locked   [k]G as the context's secret-scalar mode says, r, s; k = 0 is status 1 with zero bytes
// Only enqueues.
// ------------------------------------------------------------------------------------------
static int rfc6979_nonce_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_privs, const uint8_t *d_digests,
				    const uint8_t *d_slots, uint32_t stride, uint8_t *d_nonces, uint8_t *d_status, hipStream_t s)
{
	(void)ctx;
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
	HIPCHK(ecamd_launch_rfc6979_nonce(hash_type, R, s));
	return 0;
}

static int rfc6979_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type)
{
	if (ecrfc::hash_size(hash_type) == 0) {
		return fail(std::string(fn) + ": hash_type must be 1 .. 4 (SHA-224 / 256 / 384 / 512)");
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

extern "C" int ec_rfc6979_nonce_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs,
					  const void *d_digests, void *d_nonces, void *d_status, void *hip_stream)
{
	if (rfc6979_args_ok("ec_rfc6979_nonce_batch_dev", ctx, cv, hash_type)) {
		return -1;
	}
	if (n && (!d_privs || !d_digests || !d_nonces || !d_status)) {
		return fail("ec_rfc6979_nonce_batch_dev: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return rfc6979_nonce_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_digests, nullptr, 0, (uint8_t *)d_nonces,
						(uint8_t *)d_status, s);
	});
}

extern "C" int ec_rfc6979_nonce_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs,
				      const uint8_t *digests, uint8_t *nonces, uint8_t *status)
{
	if (rfc6979_args_ok("ec_rfc6979_nonce_batch", ctx, cv, hash_type)) {
		return -1;
	}
	if (n && (!privs || !digests || !nonces || !status)) {
		return fail("ec_rfc6979_nonce_batch: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {digests, nullptr, (size_t)ecrfc::hash_size(hash_type)}, {nullptr, nonces, ql},
					   {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return rfc6979_nonce_dev_locked(ctx, cv, hash_type, m, ip[0], ip[1], nullptr, 0, op[2], op[3], s);
	});
}

static int decdsa_sign_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *d_privs, const uint8_t *d_in,
				  uint32_t stride, int in_is_digest, uint8_t *d_sigs, uint8_t *d_status, hipStream_t s)
{
	const size_t ql = (size_t)cv->qlen;
	const uint32_t hlen = (uint32_t)ecrfc::hash_size(hash_type);
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	if (stage_need(ctx, SG_NONCES, (size_t)chunk * ql)) {
		return -1;
	}
	for (uint32_t off = 0; off < n; off += chunk) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		const uint8_t *in = d_in + (size_t)off * stride, *d_dig = in;
		if (!in_is_digest) {
			if (ecdsa_hash_stage(ctx, hash_type, m, in, stride, hlen, s)) {
				return -1;
			}
			d_dig = ctx->stage[ST_DIGESTS];
		}
		// (the nonce kernel's status lands in the caller's status bytes and is replaced by the signing core's: a zero nonce is status 1 there)
		if (rfc6979_nonce_dev_locked(ctx, cv, hash_type, m, d_privs + off * ql, d_dig, in_is_digest ? nullptr : in, stride, ctx->stage[SG_NONCES],
					     d_status + off, s) ||
		    ecdsa_sign_dev_locked(ctx, cv, m, d_privs + off * ql, ctx->stage[SG_NONCES], d_dig, hlen, d_sigs + off * 2 * ql, d_status + off, s)) {
			return -1;
		}
	}
	return 0;
}

static int decdsa_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *a, const void *b,
			  uint32_t stride, int in_is_digest, const void *c, const void *d)
{
	if (rfc6979_args_ok(fn, ctx, cv, hash_type)) {
		return -1;
	}
	if (in_is_digest != 0 && in_is_digest != 1) {
		return fail(std::string(fn) + ": in_is_digest must be 0 or 1");
	}
	if (in_is_digest ? stride != (uint32_t)ecrfc::hash_size(hash_type) : (stride < 4 || (stride & 3u) || stride > 4096)) {
		return fail(std::string(fn) + ": in_stride must be the digest length (in_is_digest = 1) or a multiple of 4 in 4 .. 4096 (message slots)");
	}
	if (n && (!a || !b || !c || !d)) {
		return fail(std::string(fn) + ": bad argument");
	}
	return 0;
}

extern "C" int ec_decdsa_sign_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const void *d_privs, const void *d_in,
					uint32_t in_stride, int in_is_digest, void *d_sigs, void *d_status, void *hip_stream)
{
	if (decdsa_args_ok("ec_decdsa_sign_batch_dev", ctx, cv, hash_type, n, d_privs, d_in, in_stride, in_is_digest, d_sigs, d_status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return decdsa_sign_dev_locked(ctx, cv, hash_type, n, (const uint8_t *)d_privs, (const uint8_t *)d_in, in_stride, in_is_digest, (uint8_t *)d_sigs,
					      (uint8_t *)d_status, s);
	});
}

extern "C" int ec_decdsa_sign_batch(ecamd_ctx *ctx, const ecamd_curve *cv, int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *in,
				    uint32_t in_stride, int in_is_digest, uint8_t *sigs, uint8_t *status)
{
	if (decdsa_args_ok("ec_decdsa_sign_batch", ctx, cv, hash_type, n, privs, in, in_stride, in_is_digest, sigs, status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {in, nullptr, in_stride}, {nullptr, sigs, 2 * ql}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return decdsa_sign_dev_locked(ctx, cv, hash_type, m, ip[0], ip[1], in_stride, in_is_digest, op[2], op[3], s);
	});
}

// Key pairs from RAW random material: x = nn_get_random_mod's value for the item's 2 * qlen random bytes (ec_key_pair_gen ->
// generic_gen_priv_key, sig/ec_key.c:602), Y = [x]G.  priv_out: n x qlen big-endian; pub_out: n x 2 clen affine X || Y.
extern "C" int ec_key_pair_gen_raw_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *raw, uint8_t *priv_out,
					 uint8_t *pub_out, uint8_t *status)
{
	if (rand_mod_args_ok("ec_key_pair_gen_raw_batch", ctx, cv)) {
		return -1;
	}
	if (n && (!raw || !priv_out || !pub_out || !status)) {
		return fail("ec_key_pair_gen_raw_batch: bad argument");
	}
	if (n == 0) {
		return 0;
	}
	const size_t ql = (size_t)cv->qlen, plen = (size_t)2 * cv->clen;
	const std::vector<HostArr> arrs = {{raw, nullptr, 2 * ql}, {nullptr, priv_out, ql}, {nullptr, pub_out, plen}, {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		if (rand_mod_dev_locked(ctx, cv, m, ip[0], op[1], s)) {
			return -1;
		}
		return smul_dev_locked(ctx, cv, m, op[1], (uint32_t)ql, nullptr, op[2], op[3], s);
	});
}

// ------------------------------------------------------------------------------------------
// batched ECC-CDH (ecccdh_derive_secret, ecdh/ecccdh.c:167-233)
// ------------------------------------------------------------------------------------------
// Device core: CD_OUT / CD_ST [d]Q' and its status, CD_HQ / CD_STH [h]Q, CD_QP / CD_STSUB [q]Q (discarded) and its status.
static int ecccdh_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *d_privs,
			     const uint8_t *d_peers, uint8_t *d_secrets, uint8_t *d_status, hipStream_t s)
{
	const size_t plen = (size_t)2 * cv->clen, ql = (size_t)cv->qlen;
	if (n > ctx->max_chunk) {  // bound the scratch: pieces of max_chunk items, in order on the stream
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			return ecccdh_dev_locked(ctx, cv, m, d_privs + off * ql, d_peers + off * plen,
						 d_secrets + (size_t)off * cv->clen, d_status + off, s);
		});
	}
	const bool cof = cv->cofactor != 1;
	if (stage_need(ctx, {{CD_OUT, n * plen}, {CD_ST, n}, {CD_HQ, cof ? n * plen : 0}, {CD_STH, cof ? n : 0}, {CD_QP, cof ? n * plen : 0},
			     {CD_STSUB, cof ? n : 0}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	EcamdCdhArgs A;
	memset(&A, 0, sizeof(A));
	A.n = n;
	A.clen = (uint32_t)cv->clen;
	const uint8_t *pts_in = d_peers;
	if (cof) {
		// cofactor h != 1 (ecdh/ecccdh.c:187-217): the peer key must lie in the subgroup ([q]Q = infinity,
		// sig/ec_key.c:199-205), then Q' = [h]Q must not be infinity, then [d]Q'
		const uint8_t *d_q = cv->d_gen + plen, *d_h = d_q + ql;
		PublicScalars pub_scope(ctx);   // the order and the cofactor are public; the private key below is not
		if (smul_dev_locked(ctx, cv, n, d_q, (uint32_t)ql, d_peers, S[CD_QP], S[CD_STSUB], s, 0) ||
		    smul_dev_locked(ctx, cv, n, d_h, 1, d_peers, S[CD_HQ], S[CD_STH], s, 0)) {
			return -1;
		}
		A.st_sub = S[CD_STSUB];
		A.st_h = S[CD_STH];
		A.hq = S[CD_HQ];
		HIPCHK(ecamd_launch_cdh_gate(A, s));
		pts_in = S[CD_HQ];
	}
	// cofactor 1: import + prj_pt_mul + prj_pt_unique in one pass
	if (smul_dev_locked(ctx, cv, n, d_privs, (uint32_t)ql, pts_in, S[CD_OUT], S[CD_ST], s)) {
		return -1;
	}
	A.pts = S[CD_OUT];
	A.st = S[CD_ST];
	A.secrets = d_secrets;
	A.status = d_status;
	HIPCHK(ecamd_launch_cdh_fin(A, s));
	return 0;
}

static int ecccdh_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *a, const void *b,
			  const void *c, const void *d)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!a || !b || !c || !d))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->cofactor == 0) {
		return fail(std::string(fn) + ": unexpected cofactor");
	}
	return 0;
}

extern "C" int ec_ecccdh_derive_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *d_privs,
					  const void *d_peers, void *d_secrets, void *d_status, void *hip_stream)
{
	if (ecccdh_args_ok("ec_ecccdh_derive_batch_dev", ctx, cv, n, d_privs, d_peers, d_secrets, d_status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return ecccdh_dev_locked(ctx, cv, n, (const uint8_t *)d_privs, (const uint8_t *)d_peers, (uint8_t *)d_secrets,
					 (uint8_t *)d_status, s);
	});
}

extern "C" int ec_ecccdh_derive_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *privs,
				      const uint8_t *peers, uint8_t *secrets, uint8_t *status)
{
	if (ecccdh_args_ok("ec_ecccdh_derive_batch", ctx, cv, n, privs, peers, secrets, status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t plen = (size_t)2 * cv->clen, ql = (size_t)cv->qlen;
	const std::vector<HostArr> arrs = {{privs, nullptr, ql}, {peers, nullptr, plen}, {nullptr, secrets, (size_t)cv->clen},
					   {nullptr, status, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return ecccdh_dev_locked(ctx, cv, m, ip[0], ip[1], op[2], op[3], s);
	});
}

// ------------------------------------------------------------------------------------------
// batched X25519 / X448 (x25519() / x448(), ecdh/x25519_448.c:380-425 -> x25519_448_core :146)
// ------------------------------------------------------------------------------------------
Big ecamd_host::big_sqrt_m1(const Big &p)  // 2^((p-1)/4) mod p, a square root of -1 when p = 5 mod 8
{
	Big one(1, 1), two(1, 2);
	Big e = big_sub(p, one);
	// divide by 4
	Big q(e.size(), 0);
	for (size_t i = 0; i < e.size(); i++) {
		q[i] = (e[i] >> 2) | ((i + 1 < e.size()) ? (e[i + 1] << 30) : 0u);
	}
	big_trim(q);
	return big_powmod(two, q, p);
}

// constants of the X25519 / X448 path for this handle; ctx->mu held
static void xdh_setup(ecamd_curve *cv)
{
	cv->xdh_state = -1;
	// the Weierstrass models of Curve25519 / Curve448: A = 486662 / 156326, B = 1
	uint32_t Aval = 0;
	if (cv->pbits == 255 && cv->clen == 32 && big_cmp(cv->p, big_sub(big_pow2(255), Big(1, 19))) == 0) {
		Aval = 486662;
	} else if (cv->pbits == 448 && cv->clen == 56 &&
		   big_cmp(cv->p, big_sub(big_sub(big_pow2(448), big_pow2(224)), Big(1, 1))) == 0) {
		Aval = 156326;
	} else {
		cv->xdh_err = "ec_xdh_batch: the curve is neither WEI25519 nor WEI448";
		return;
	}
	const Big &p = cv->p;
	const int nw = cv->nw;
	const Big A(1, Aval), one(1, 1), two(1, 2), three(1, 3), nine(1, 9), tw7(1, 27);
	const Big pm2 = big_sub(p, two);
	{
		// make sure the handle really is the birationally equivalent Weierstrass curve:
		// a = (3 - A^2) / 3, b = (2 A^3 - 9 A) / 27
		Big A2 = big_mulmod(A, A, p);
		Big a_exp = big_mulmod(big_mod(big_add(big_sub(p, A2), three), p), big_powmod(three, pm2, p), p);
		Big A3c = big_mulmod(A2, A, p);
		Big num = big_mod(big_add(big_mulmod(two, A3c, p), big_sub(p, big_mulmod(nine, A, p))), p);
		Big b_exp = big_mulmod(num, big_powmod(tw7, pm2, p), p);
		if (big_cmp(a_exp, cv->a) != 0 || big_cmp(b_exp, cv->b) != 0) {
			cv->xdh_err = "ec_xdh_batch: curve coefficients do not match the Montgomery curve";
			return;
		}
	}
	const Big R = big_mod(big_pow2(32 * nw), p);
	const Big A3 = big_mulmod(A, big_powmod(three, pm2, p), p);
	EcamdXdhPrepArgs &P = cv->xdh_tmpl;
	memset(&P, 0, sizeof(P));
	P.len = (uint32_t)cv->clen;
	Big e;
	if ((p[0] & 7u) == 5u) {
		P.mode = 0;
		e = big_add(p, three);  // (p + 3) / 8
		Big q(e.size(), 0);
		for (size_t i = 0; i < e.size(); i++) {
			q[i] = (e[i] >> 3) | ((i + 1 < e.size()) ? (e[i + 1] << 29) : 0u);
		}
		e = q;
		big_store(P.sm1, nw, big_mulmod(big_sqrt_m1(p), R, p));
	} else {
		P.mode = 1;
		e = big_add(p, one);  // (p + 1) / 4
		Big q(e.size(), 0);
		for (size_t i = 0; i < e.size(); i++) {
			q[i] = (e[i] >> 2) | ((i + 1 < e.size()) ? (e[i + 1] << 30) : 0u);
		}
		e = q;
	}
	big_trim(e);
	P.ebits = (uint32_t)big_bitlen(e);
	big_store(P.e, 17, e);
	big_store(P.A, nw, big_mulmod(A, R, p));
	big_store(P.A3, nw, big_mulmod(A3, R, p));
	if (Aval == 486662) {
		big_digits29(P.g_A, 9, A);
		big_digits29(P.g_A3, 9, A3);
		big_digits29(P.g_sm1, 9, big_sqrt_m1(p));
	} else if (cv->pbits == 448) {
		big_digits29(P.g_A, 16, A, 28);      // the Goldilocks unit's 28-bit limbs
		big_digits29(P.g_A3, 16, A3, 28);
	}
	P.slot = cv->slot;
	big_store(cv->xdh_A3, 17, A3);
	// cofactor h: order = h q
	uint32_t hval = 0;
	Big t = cv->q;
	for (uint32_t c = 1; c <= 16; c++) {
		if (big_cmp(t, cv->order) == 0) {
			hval = c;
			break;
		}
		t = big_add(t, cv->q);
	}
	if (hval != 4 && hval != 8) {
		cv->xdh_err = "ec_xdh_batch: unexpected cofactor";
		return;
	}
	cv->xdh_cof = (uint8_t)hval;
	P.cof_dbl = hval == 8 ? 3u : 2u;
	cv->xdh_state = 1;
}

// device pointers in and out; only enqueues on s
static int xdh_dev_locked(ecamd_ctx *ctx, ecamd_curve *cv, uint32_t n, const uint8_t *d_k, const uint8_t *d_u,
			  uint8_t *d_out, uint8_t *d_status, hipStream_t s)
{
	if (n > ctx->max_chunk) {  // bound the scratch: pieces of max_chunk items, in order on the stream
		return for_chunks(ctx, n, [&](uint32_t off, uint32_t m) -> int {
			const size_t l = (size_t)cv->clen;
			return xdh_dev_locked(ctx, cv, m, d_k + off * l, d_u + off * l, d_out + off * l, d_status + off, s);
		});
	}
	const size_t len = (size_t)cv->clen, plen = 2 * len;
	if (stage_need(ctx, {{XD_SCALARS, n * len}, {XD_POINTS, n * plen}, {XD_FLAGS, n}, {XD_OUT, n * plen}, {XD_STK, n}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	const int nw = cv->nw;
	EcamdXdhPrepArgs P = cv->xdh_tmpl;
	P.k = d_k;
	P.u = d_u;
	P.scalars = S[XD_SCALARS];
	P.points = S[XD_POINTS];
	P.flags = S[XD_FLAGS];
	P.n = n;
	if (cv->gflavour == 2 && cv->gslot >= 0) {
		// X25519 on the radix-2^29 field of the 2^255 - 19 unit: validation + clamping, then the x-only
		// Montgomery ladder with a shared inversion (the u coordinate is all the reference exposes)
		HIPCHK(ecamd_launch_xdh_prep_c25519(P, cv->gslot, s));
		if (getenv("ECAMD_NO_X25519_LADDER") == nullptr) {
			if (stage_need(ctx, XD_REC, (size_t)n * ECAMD_XDH_REC_WORDS * 4)) {
				return -1;
			}
			EcamdXdhLadderArgs L;
			L.u = d_u;
			L.scalars = S[XD_SCALARS];
			L.flags = S[XD_FLAGS];
			L.rec = (uint32_t *)S[XD_REC];
			L.out = d_out;
			L.status = d_status;
			L.n = n;
			HIPCHK(ecamd_launch_x25519_ladder(L, cv->gslot, s, ctx->timing ? ctx->ev_dom : nullptr));
			ctx->ev_dom_valid = ctx->ev_dom_valid || ctx->timing;
			return 0;
		}
	} else if (cv->gflavour == 5 && cv->gslot >= 0 && P.mode == 1 && getenv("ECAMD_NO_G448_DECODE") == nullptr) {
		HIPCHK(ecamd_launch_xdh_prep_c448(P, cv->gslot, s));   // X448: the same front end on the Goldilocks radix-2^29 field
		if (getenv("ECAMD_NO_X448_LADDER") == nullptr) {
			// and the x-only Montgomery ladder with a shared inversion, as for X25519
			if (stage_need(ctx, XD_REC, (size_t)n * ECAMD_X448_REC_WORDS * 4)) {
				return -1;
			}
			EcamdXdhLadderArgs L;
			L.u = d_u;
			L.scalars = S[XD_SCALARS];
			L.flags = S[XD_FLAGS];
			L.rec = (uint32_t *)S[XD_REC];
			L.out = d_out;
			L.status = d_status;
			L.n = n;
			HIPCHK(ecamd_launch_x448_ladder(L, cv->gslot, s, ctx->timing ? ctx->ev_dom : nullptr));
			ctx->ev_dom_valid = ctx->ev_dom_valid || ctx->timing;
			return 0;
		}
	} else {
		HIPCHK(ecamd_launch_xdh_prep(nw, P, s));
	}
	// [k]Q  ([h]Q != infinity was checked by the prep kernel)
	if (smul_dev_locked(ctx, cv, n, S[XD_SCALARS], (uint32_t)len, S[XD_POINTS], S[XD_OUT], S[XD_STK], s)) {
		return -1;
	}
	EcamdXdhFinArgs Fn;
	memset(&Fn, 0, sizeof(Fn));
	Fn.pts = S[XD_OUT];
	Fn.stk = S[XD_STK];
	Fn.flags = S[XD_FLAGS];
	Fn.out = d_out;
	Fn.status = d_status;
	Fn.n = n;
	Fn.len = (uint32_t)len;
	memcpy(Fn.A3, cv->xdh_A3, sizeof(Fn.A3));
	Fn.slot = cv->slot;
	HIPCHK(ecamd_launch_xdh_fin(nw, Fn, s));
	return 0;
}

static int xdh_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const void *a, const void *b,
		       const void *c, const void *d)
{
	if (!ctx || !cv_in || cv_in->ctx != ctx || (n && (!a || !b || !c || !d))) {
		return fail(std::string(fn) + ": bad argument");
	}
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	if (cv->xdh_state == 0) {
		xdh_setup(cv);
	}
	if (cv->xdh_state < 0) {
		return fail(cv->xdh_err);
	}
	return 0;
}

extern "C" int ec_xdh_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const void *d_k, const void *d_u,
				void *d_out, void *d_status, void *hip_stream)
{
	if (!ctx) {
		return fail("ec_xdh_batch_dev: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	if (xdh_args_ok("ec_xdh_batch_dev", ctx, cv_in, n, d_k, d_u, d_out, d_status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
	StreamScope scope(ctx, s);
	return xdh_dev_locked(ctx, const_cast<ecamd_curve *>(cv_in), n, (const uint8_t *)d_k, (const uint8_t *)d_u,
			      (uint8_t *)d_out, (uint8_t *)d_status, s);
}

extern "C" int ec_xdh_batch(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const uint8_t *k, const uint8_t *u,
			    uint8_t *out, uint8_t *status)
{
	if (!ctx) {
		return fail("ec_xdh_batch: bad argument");
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: the checks run the curve's one-time setup, under the lock
	if (xdh_args_ok("ec_xdh_batch", ctx, cv_in, n, k, u, out, status)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	HIPCHK(hipSetDevice(ctx->device));
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	const size_t len = (size_t)cv->clen;
	const std::vector<HostArr> arrs = {{k, nullptr, len}, {u, nullptr, len}, {nullptr, out, len}, {nullptr, status, 1}};
	return host_pipeline(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return xdh_dev_locked(ctx, cv, m, ip[0], ip[1], op[2], op[3], s);
	});
}

// ------------------------------------------------------------------------------------------
// scalar multiplication / normalisation with a choice of point wire formats
// ------------------------------------------------------------------------------------------
static int pt_fmt_batch(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *scalars,
			uint32_t slen, const uint8_t *points, int in_fmt, uint8_t *out, int out_fmt, uint8_t *status,
			bool mul)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!out || !status || (mul && !scalars) || (!mul && !points)))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if ((in_fmt != 0 && in_fmt != 1) || (out_fmt != 0 && out_fmt != 1)) {
		return fail(std::string(fn) + ": point format must be ECAMD_PT_AFFINE or ECAMD_PT_PROJECTIVE");
	}
	if (mul && (slen == 0 || slen > 1024)) {
		return fail(std::string(fn) + ": scalar_len must be in 1..1024");
	}
	if (n == 0) {
		return 0;
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: stages by hand on the context's stream, and sizes its slots before the scope opens
	HIPCHK(hipSetDevice(ctx->device));
	const size_t clen = (size_t)cv->clen, alen = 2 * clen;
	const size_t ilen = (in_fmt ? 3 : 2) * clen, olen = (out_fmt ? 3 : 2) * clen;
	// the points as given, their affine form and import status, the affine results and their status, the output in out_fmt
	if (stage_need(ctx, {{PF_SCALARS, mul ? (size_t)n * slen : 0}, {PF_IN, points ? n * ilen : 0}, {PF_AFF, n * alen}, {PF_PRE, n},
			     {PF_RES, n * alen}, {PF_RST, n}, {PF_OUT, n * olen}, {PF_OST, n}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	if (mul) {
		HIPCHK(hipMemcpyAsync(S[PF_SCALARS], scalars, (size_t)n * slen, hipMemcpyHostToDevice, s));
	}
	if (points) {
		HIPCHK(hipMemcpyAsync(S[PF_IN], points, n * ilen, hipMemcpyHostToDevice, s));
	}
	const uint8_t *d_aff = points ? S[PF_IN] : nullptr;  // affine inputs of the scalar multiplication (NULL: generator)
	const uint8_t *d_pre = nullptr;
	if (points && in_fmt == 1) {
		EcamdPrjInArgs I;
		I.in = S[PF_IN];
		I.aff = S[PF_AFF];
		I.pre = S[PF_PRE];
		I.n = n;
		I.clen = (uint32_t)clen;
		I.for_mul = mul ? 1 : 0;
		I.slot = cv->slot;
		HIPCHK(launch_prj_import(cv, I, s));
		d_aff = S[PF_AFF];
		d_pre = S[PF_PRE];
	}
	const uint8_t *d_res = d_aff, *d_st = nullptr;
	if (mul) {
		if (smul_dev_locked(ctx, cv, n, S[PF_SCALARS], slen, d_aff, S[PF_RES], S[PF_RST], s)) {
			return -1;
		}
		d_res = S[PF_RES];
		d_st = S[PF_RST];
	} else if (in_fmt == 0) {
		// affine in, no multiplication: validation only, through the group-law kernel's import checks
		// (P + P is computed and dropped; its status carries the import result)
		EcamdPtArgs A;
		A.p1 = S[PF_IN];
		A.p2 = nullptr;
		A.out = S[PF_RES];
		A.status = S[PF_RST];
		A.n = n;
		A.clen = (uint32_t)clen;
		A.dbl = 1;
		A.slot = cv->slot;
		HIPCHK(ecamd_launch_pt(cv->nw, A, s));
		// a valid point may double to infinity (order 2): only the import error matters here
		std::vector<uint8_t> st(n);
		HIPCHK(hipMemcpyAsync(st.data(), S[PF_RST], n, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		for (uint32_t i = 0; i < n; i++) {
			st[i] = st[i] == 1 ? 1 : 0;
		}
		HIPCHK(hipMemcpyAsync(S[PF_RST], st.data(), n, hipMemcpyHostToDevice, s));
		HIPCHK(hipStreamSynchronize(s));
		d_st = S[PF_RST];
	}
	EcamdPrjOutArgs O;
	O.aff = d_res;
	O.st = d_st;
	O.pre = d_pre;
	O.out = S[PF_OUT];
	O.status = S[PF_OST];
	O.n = n;
	O.clen = (uint32_t)clen;
	O.out_prj = out_fmt;
	HIPCHK(ecamd_launch_prj_export(O, s));
	HIPCHK(hipMemcpyAsync(out, S[PF_OUT], n * olen, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(status, S[PF_OST], n, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

extern "C" int ec_prj_pt_mul_batch_fmt(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *scalars,
				       uint32_t slen, const uint8_t *points, int in_fmt, uint8_t *out, int out_fmt,
				       uint8_t *status)
{
	return pt_fmt_batch("ec_prj_pt_mul_batch_fmt", ctx, cv, n, scalars, slen, points, in_fmt, out, out_fmt, status, true);
}

extern "C" int ec_prj_pt_unique_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *points, int in_fmt,
				      uint8_t *out, int out_fmt, uint8_t *status)
{
	return pt_fmt_batch("ec_prj_pt_unique_batch", ctx, cv, n, nullptr, 0, points, in_fmt, out, out_fmt, status, false);
}

// ------------------------------------------------------------------------------------------
// point decompression: aff_pt_y_from_x (curves/aff_pt.c:102) / fp_sqrt (fp/fp_sqrt.c:107)
// ------------------------------------------------------------------------------------------
static int sqrt_setup(ecamd_curve *cv)
{
	if (cv->sqrt_state == 1) {
		return 0;
	}
	const Big &p = cv->p;
	const Big one(1, 1);
	Big q = big_sub(p, one);
	uint32_t s = 0;
	while (!(q[0] & 1u)) {           // p - 1 = q 2^s
		Big t(q.size(), 0);
		for (size_t i = 0; i < q.size(); i++) {
			t[i] = (q[i] >> 1) | ((i + 1 < q.size()) ? (q[i + 1] << 31) : 0u);
		}
		big_trim(t);
		q = t;
		s++;
	}
	// z: the smallest quadratic non-residue, found as fp_sqrt finds it (counting up from 0, fp/fp_sqrt.c:197-200)
	Big half = big_sub(p, one);
	{
		Big t(half.size(), 0);
		for (size_t i = 0; i < half.size(); i++) {
			t[i] = (half[i] >> 1) | ((i + 1 < half.size()) ? (half[i + 1] << 31) : 0u);
		}
		big_trim(t);
		half = t;
	}
	Big z(1, 2);
	const Big pm1 = big_sub(p, one);
	for (uint32_t zz = 2; zz < 100000; zz++) {
		z = Big(1, zz);
		if (big_cmp(big_powmod(z, half, p), pm1) == 0) {
			break;
		}
	}
	if (big_cmp(big_powmod(z, half, p), pm1) != 0) {
		return fail("ec_aff_pt_y_from_x_batch: no small quadratic non-residue (is p prime?)");
	}
	EcamdYfromXArgs &T = cv->sqrt_tmpl;
	memset(&T, 0, sizeof(T));
	T.s = s;
	Big e = big_sub(q, one);         // (q - 1) / 2
	{
		Big t(e.size(), 0);
		for (size_t i = 0; i < e.size(); i++) {
			t[i] = (e[i] >> 1) | ((i + 1 < e.size()) ? (e[i + 1] << 31) : 0u);
		}
		big_trim(t);
		e = t;
	}
	T.ebits = (uint32_t)big_bitlen(e);
	big_store(T.e, 17, e);
	const Big R = big_mod(big_pow2(32 * cv->nw), p);
	big_store(T.c, 17, big_mulmod(big_powmod(z, q, p), R, p));
	T.clen = (uint32_t)cv->clen;
	T.slot = cv->slot;
	cv->sqrt_state = 1;
	return 0;
}

static int y_from_x_common(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const uint8_t *in, uint32_t in_stride,
			   uint8_t *o1, uint8_t *o2, uint8_t *status, uint32_t mode)
{
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	if (!ctx || !cv || cv->ctx != ctx || (n && (!in || !o1 || !status || (mode == 0 && !o2)))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (n == 0) {
		return 0;
	}
	std::lock_guard<std::mutex> lk(ctx->mu);   // own head: stages by hand on the context's stream, and sizes its slots before the scope opens
	HIPCHK(hipSetDevice(ctx->device));
	if (sqrt_setup(cv)) {
		return -1;
	}
	const size_t cl = (size_t)cv->clen;
	const size_t in_bytes = (size_t)n * in_stride, y1_bytes = (size_t)n * cl * (mode ? 2 : 1), y2_bytes = (size_t)n * cl;
	if (stage_need(ctx, {{YX_IN, in_bytes}, {YX_Y1, y1_bytes}, {YX_Y2, y2_bytes}, {YX_ST, n}})) {
		return -1;
	}
	hipStream_t s = ctx->stream;
	StreamScope scope(ctx, s);
	uint8_t **S = ctx->stage;
	HIPCHK(hipMemcpyAsync(S[YX_IN], in, in_bytes, hipMemcpyHostToDevice, s));
	EcamdYfromXArgs A = cv->sqrt_tmpl;
	A.x = S[YX_IN];
	A.xstride = in_stride;
	A.y1 = S[YX_Y1];
	A.y2 = S[YX_Y2];
	A.aff = S[YX_Y1];
	A.status = S[YX_ST];
	A.n = n;
	A.mode = mode;
	HIPCHK(ecamd_launch_y_from_x(cv->nw, A, s));
	HIPCHK(hipMemcpyAsync(o1, S[YX_Y1], y1_bytes, hipMemcpyDeviceToHost, s));
	if (mode == 0) {
		HIPCHK(hipMemcpyAsync(o2, S[YX_Y2], y2_bytes, hipMemcpyDeviceToHost, s));
	}
	HIPCHK(hipMemcpyAsync(status, S[YX_ST], n, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

extern "C" int ec_aff_pt_y_from_x_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *x, uint8_t *y1, uint8_t *y2,
					uint8_t *status)
{
	return y_from_x_common("ec_aff_pt_y_from_x_batch", ctx, cv, n, x, cv ? (uint32_t)cv->clen : 0, y1, y2, status, 0);
}

extern "C" int ec_point_decompress_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *compressed, uint8_t *out_aff,
					 uint8_t *status)
{
	return y_from_x_common("ec_point_decompress_batch", ctx, cv, n, compressed, cv ? (uint32_t)cv->clen + 1 : 0, out_aff, nullptr, status, 1);
}

// ------------------------------------------------------------------------------------------
// batched ECDSA public-key recovery: ecdsa_public_key_from_sig / decdsa_public_key_from_sig (sig/ecdsa.c, sig/decdsa.c ->
// __ecdsa_public_key_from_sig, sig/ecdsa_common.c:867-1049) + ec_pub_key_export_to_aff_buf (sig/ec_key.c) of the two keys
// ------------------------------------------------------------------------------------------
// The reference: three prj_pt_mul and two prj_pt_add per item (:988-994).  Here, per chunk of at most max_chunk items:
//   k_recover_prep    range checks, e, u = -(e / r), v = s / r mod q, x = r as a field element (r >= p: the reference's -1)
//   k_y_from_x        the two roots in fp_sqrt's order; an x that is no abscissa is the reference's -1 (its "restart" with
//                     r + 2q can only fail: the comparison at :921 refuses a candidate below p, fp_set_nn one that is not)
//   k_recover_point   R = (x, y1)
//   A = [u]G          ONE fixed-base pass (the generator's comb table where the handle has one)
//   B = [v]R          ONE variable-base window loop; (x, y2) = -R, so [v](x, y2) = -B is never computed
//   k_recover_fin     Y1 = A + B, Y2 = A - B, two chords with the denominator x_B - x_A, inverted together for eight items
//   k_recover_redo    the items with A or B at infinity or x_A = x_B, on the complete formulas (nothing marked: a near-empty launch)
// Every multiplier is a function of the signature and the digest: public, whatever ecamd_ctx_set_secret_scalars says.
// R is no key: no [q]R pass.  Frame: ST_U .. ST_FLAGS and RC_.  Only enqueues.
static int ecdsa_recover_dev_locked(ecamd_ctx *ctx, const ecamd_curve *cv_in, uint32_t n, const uint8_t *d_sig, const uint8_t *d_dig,
				    uint32_t hlen, uint8_t *d_pub1, uint8_t *d_pub2, uint8_t *d_st1, uint8_t *d_st2, hipStream_t s)
{
	ecamd_curve *cv = const_cast<ecamd_curve *>(cv_in);
	if (sqrt_setup(cv)) {
		return -1;
	}
	PublicScalars pub_scope(ctx);
	const size_t cl = (size_t)cv->clen, plen = 2 * cl, ql = (size_t)cv->qlen;
	const uint32_t chunk = n < ctx->max_chunk ? n : ctx->max_chunk;
	if (two_mul_need(ctx, cv, chunk) ||
	    stage_need(ctx, {{RC_YST, chunk}, {RC_X, chunk * cl}, {RC_Y1, chunk * cl}, {RC_Y2, chunk * cl}, {RC_R, chunk * plen}})) {
		return -1;
	}
	uint8_t **S = ctx->stage;
	for (uint32_t off = 0; off < n; off += chunk) {
		const uint32_t m = (n - off) < chunk ? (n - off) : chunk;
		EcamdRecoverPrepArgs P;
		memset(&P, 0, sizeof(P));
		P.sigs = d_sig + (size_t)off * 2 * ql;
		P.digests = d_dig + (size_t)off * hlen;
		P.u = S[ST_U];
		P.v = S[ST_V];
		P.x = S[RC_X];
		P.flags = S[ST_FLAGS];
		P.n = m;
		P.qlen = (uint32_t)ql;
		P.clen = (uint32_t)cl;
		P.hlen = hlen;
		P.qbits = (uint32_t)cv->qbits;
		P.qslot = cv->qslot;
		big_to_be(P.p_be, (int)cl, cv->p);
		HIPCHK(ecamd_launch_recover_prep(cv->qnw, P, s));
		EcamdYfromXArgs Y = cv->sqrt_tmpl;
		Y.x = S[RC_X];
		Y.xstride = (uint32_t)cl;
		Y.y1 = S[RC_Y1];
		Y.y2 = S[RC_Y2];
		Y.aff = S[RC_Y1];
		Y.status = S[RC_YST];
		Y.n = m;
		Y.mode = 0;
		HIPCHK(ecamd_launch_y_from_x(cv->nw, Y, s));
		EcamdRecoverPointArgs R;
		R.x = S[RC_X];
		R.y1 = S[RC_Y1];
		R.flags = S[ST_FLAGS];
		R.yst = S[RC_YST];
		R.R = S[RC_R];
		R.n = m;
		R.clen = (uint32_t)cl;
		HIPCHK(ecamd_launch_recover_point(R, s));
		// A = [u]G (:988), B = [v](x, y1) (:990), Y1 = A + B and Y2 = A - B straight into the caller's arrays
		if (two_mul_sum_dev(ctx, cv, m, S[RC_R], false, S[RC_YST], d_pub1 + (size_t)off * plen, d_pub2 + (size_t)off * plen, d_st1 + off,
				    d_st2 + off, s)) {
			return -1;
		}
	}
	return 0;
}

static int ecdsa_recover_args_ok(const char *fn, ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *sigs, const void *digests,
				 uint32_t hlen, const void *o1, const void *o2, const void *s1, const void *s2)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!sigs || !digests || !o1 || !o2 || !s1 || !s2))) {
		return fail(std::string(fn) + ": bad argument");
	}
	if (cv->qslot < 0) {
		return fail(std::string(fn) + ": generator order not supported for this curve");
	}
	if (hlen == 0 || hlen > 128) {
		return fail(std::string(fn) + ": digest length must be in 1..128");
	}
	return 0;
}

extern "C" int ec_ecdsa_recover_batch_dev(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const void *d_sigs, const void *d_digests,
					  uint32_t hlen, void *d_pub1_aff, void *d_pub2_aff, void *d_status1, void *d_status2, void *hip_stream)
{
	if (ecdsa_recover_args_ok("ec_ecdsa_recover_batch_dev", ctx, cv, n, d_sigs, d_digests, hlen, d_pub1_aff, d_pub2_aff, d_status1, d_status2)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	return dev_call(ctx, hip_stream, [&](hipStream_t s) {
		return ecdsa_recover_dev_locked(ctx, cv, n, (const uint8_t *)d_sigs, (const uint8_t *)d_digests, hlen, (uint8_t *)d_pub1_aff,
						(uint8_t *)d_pub2_aff, (uint8_t *)d_status1, (uint8_t *)d_status2, s);
	});
}

extern "C" int ec_ecdsa_recover_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *sigs, const uint8_t *digests,
				      uint32_t hlen, uint8_t *pub1_aff, uint8_t *pub2_aff, uint8_t *status1, uint8_t *status2)
{
	if (ecdsa_recover_args_ok("ec_ecdsa_recover_batch", ctx, cv, n, sigs, digests, hlen, pub1_aff, pub2_aff, status1, status2)) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	const size_t plen = (size_t)2 * cv->clen;
	const std::vector<HostArr> arrs = {{sigs, nullptr, (size_t)2 * cv->qlen}, {digests, nullptr, hlen}, {nullptr, pub1_aff, plen},
					   {nullptr, pub2_aff, plen}, {nullptr, status1, 1}, {nullptr, status2, 1}};
	return host_call(ctx, cv->pbits, n, arrs, [&](uint32_t m, const DevIn &ip, const DevOut &op, hipStream_t s, const Between &) {
		return ecdsa_recover_dev_locked(ctx, cv, m, ip[0], ip[1], hlen, op[2], op[3], op[4], op[5], s);
	});
}

// ------------------------------------------------------------------------------------------
// structured signatures and private keys: 3 header bytes in front of the raw bytes (sig/sig_algs.c:702-780, sig/ec_key.c:312-360)
// ------------------------------------------------------------------------------------------
extern "C" int ec_structured_sig_import_batch(const ecamd_curve *cv, uint32_t n, const uint8_t *structured, uint32_t structured_len,
					      int alg_type, int hash_type, uint8_t *raw_sigs, uint8_t *status)
{
	if (!cv || (n && (!structured || !raw_sigs || !status)) || structured_len <= 3 || structured_len > 3 + 255) {
		return fail("ec_structured_sig_import_batch: bad argument");
	}
	if (cv->curve_type <= 0) {
		return fail("ec_structured_sig_import_batch: the curve handle is not one of libecc's built-in curves");
	}
	const size_t raw = structured_len - 3;
	for (uint32_t i = 0; i < n; i++) {
		const uint8_t *k = structured + (size_t)i * structured_len;
		// ec_structured_sig_import_from_buf hands the three bytes back; a caller then checks them against what it expects
		// (tests/ec_utils.c:verify_bin_file): algorithm, hash, curve
		const bool ok = k[0] == (uint8_t)alg_type && k[1] == (uint8_t)hash_type && k[2] == (uint8_t)cv->curve_type;
		status[i] = ok ? 0 : 1;
		if (ok) {
			memcpy(raw_sigs + (size_t)i * raw, k + 3, raw);
		} else {
			memset(raw_sigs + (size_t)i * raw, 0, raw);
		}
	}
	return 0;
}

// ec_structured_key_pair_import_from_priv_key_buf (sig/ec_key.c:443-470) for the algorithms whose public key is Y = xG
// (ECDSA = 1, DECDSA = 14 in lib_ecc_types.h; __ecdsa_init_pub_key, sig/ecdsa_common.c:172-200): header EC_PRIVKEY (1), algorithm, curve;
// x < q or error; Y = [x]G on the device (x = 0 gives the key at infinity, as the reference's prj_pt_mul_blind does).
extern "C" int ec_structured_key_pair_import_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *priv_keys,
						   uint32_t key_len, int alg_type, uint8_t *priv_out, uint8_t *pub_prj_out, uint8_t *status)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!priv_keys || !pub_prj_out || !status))) {
		return fail("ec_structured_key_pair_import_batch: bad argument");
	}
	if (cv->curve_type <= 0) {
		return fail("ec_structured_key_pair_import_batch: the curve handle is not one of libecc's built-in curves");
	}
	const size_t ql = (size_t)cv->qlen, cl = (size_t)cv->clen;
	if (key_len <= 3 || key_len > 3 + 255) {
		return fail("ec_structured_key_pair_import_batch: key_len must be 3 + the private key length");
	}
	if (n == 0) {
		return 0;
	}
	const size_t xl = key_len - 3;
	std::vector<uint8_t> x((size_t)n * ql, 0), bad(n, 0), pts((size_t)n * 3 * cl), st(n);
	for (uint32_t i = 0; i < n; i++) {
		const uint8_t *k = priv_keys + (size_t)i * key_len;
		bool ok = k[0] == 1 && k[1] == (uint8_t)alg_type && k[2] == (uint8_t)cv->curve_type;
		const Big xv = big_from_be(k + 3, xl);       // nn_init_from_buf takes any length
		ok = ok && big_cmp(xv, cv->q) < 0;           // "Sanity check on key compliance"
		bad[i] = ok ? 0 : 1;
		if (ok) {
			big_to_be(&x[(size_t)i * ql], (int)ql, xv);
		}
		if (priv_out) {
			if (ok) {
				memcpy(priv_out + (size_t)i * ql, &x[(size_t)i * ql], ql);
			} else {
				memset(priv_out + (size_t)i * ql, 0, ql);
			}
		}
	}
	const int rc = ec_prj_pt_mul_batch_fmt(ctx, cv, n, x.data(), (uint32_t)ql, nullptr, ECAMD_PT_AFFINE, pts.data(), ECAMD_PT_PROJECTIVE, st.data());
	std::fill(x.begin(), x.end(), 0);   // private scalars
	if (rc) {
		return -1;
	}
	for (uint32_t i = 0; i < n; i++) {
		uint8_t *o = pub_prj_out + (size_t)i * 3 * cl;
		if (bad[i] || st[i] == ECAMD_ERR) {
			status[i] = ECAMD_ERR;
			memset(o, 0, 3 * cl);
		} else if (st[i] == ECAMD_INF) {
			status[i] = ECAMD_INF;          // x = 0: the key is the point at infinity (0 : 1 : 0)
			memset(o, 0, 3 * cl);
			o[2 * cl - 1] = 1;
		} else {
			status[i] = ECAMD_OK;
			memcpy(o, &pts[(size_t)i * 3 * cl], 3 * cl);
		}
	}
	return 0;
}

// ------------------------------------------------------------------------------------------
// structured public keys: ec_structured_pub_key_import_from_buf (sig/ec_key.c:312-345)
// ------------------------------------------------------------------------------------------
extern "C" int ec_structured_pub_key_import_batch(ecamd_ctx *ctx, const ecamd_curve *cv, uint32_t n, const uint8_t *keys,
						  uint32_t key_len, int alg_type, uint8_t *out_aff, uint8_t *status)
{
	if (!ctx || !cv || cv->ctx != ctx || (n && (!keys || !out_aff || !status))) {
		return fail("ec_structured_pub_key_import_batch: bad argument");
	}
	const size_t clen = (size_t)cv->clen, plen = 3 * clen, alen = 2 * clen;
	if (key_len != 3 + plen) {
		return fail("ec_structured_pub_key_import_batch: key_len must be 3 + 3 * coordinate length");
	}
	if (cv->curve_type <= 0) {
		return fail("ec_structured_pub_key_import_batch: the curve handle is not one of libecc's built-in curves");
	}
	if (n == 0) {
		return 0;
	}
	// header: EC_PUBKEY (0), the signature / ECDH algorithm, the curve type (sig/ec_key.h:31, lib_ecc_types.h)
	std::vector<uint8_t> hdr_bad(n), packed((size_t)n * plen);
	for (uint32_t i = 0; i < n; i++) {
		const uint8_t *k = keys + (size_t)i * key_len;
		hdr_bad[i] = (k[0] != 0 || k[1] != (uint8_t)alg_type || k[2] != (uint8_t)cv->curve_type) ? 1 : 0;
		memcpy(&packed[(size_t)i * plen], k + 3, plen);
	}
	// ec_pub_key_import_from_buf (:216-245): prj_pt_import_from_buf, then [q]Y = infinity when the cofactor is not 1
	if (pt_fmt_batch("ec_structured_pub_key_import_batch", ctx, cv, n, nullptr, 0, packed.data(), 1, out_aff, 0, status, false)) {
		return -1;
	}
	if (big_cmp(cv->order, cv->q) != 0) {
		std::vector<uint8_t> qb((size_t)n * cv->qlen), tmp((size_t)n * alen), st(n);
		for (uint32_t i = 0; i < n; i++) {
			big_to_be(&qb[(size_t)i * cv->qlen], cv->qlen, cv->q);
		}
		if (ec_prj_pt_mul_batch(ctx, cv, n, qb.data(), (uint32_t)cv->qlen, out_aff, tmp.data(), st.data())) {
			return -1;
		}
		for (uint32_t i = 0; i < n; i++) {
			if (status[i] == 0 && st[i] != 2) {
				status[i] = 1;  // not in the subgroup of the generator
			}
			if (status[i] == 2) {
				// infinity (0 : Y : 0) passes check_prj_pt_order; the degenerate (0 : 0 : 0) fails in its additions
				bool allzero = true;
				for (size_t b = 0; b < plen && allzero; b++) {
					allzero = packed[(size_t)i * plen + b] == 0;
				}
				if (allzero) {
					status[i] = 1;
				}
			}
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		if (hdr_bad[i]) {
			status[i] = 1;
		}
		if (status[i] != 0) {
			memset(out_aff + (size_t)i * alen, 0, alen);
		}
	}
	return 0;
}
