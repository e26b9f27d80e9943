// Host build of libecc_amd/csrc/ecamd_eddsa_sign.hip (and through it ecamd_eddsa_sign.h) over tests/hipstub (g++, no HIP): the three
// kernels of one-call EdDSA signing through their launchers, the lanes one after the other, for tests/test_eddsa_sign_host.py.
// With -DEDDSA_SIGN_MAIN: a stand-alone program (for -fsanitize=address,undefined) that runs the items of a text file, every buffer
// allocated at its exact size.  Test infrastructure, not product code.
#include <hip/hip_runtime.h>
#include <string.h>
thread_local dim3 blockIdx, threadIdx;
#include "../libecc_amd/csrc/ecamd_eddsa_sign.hip"

static void eds_set_dom(EcamdEddsaSignArgs *A, int alg, const uint8_t *adata, uint32_t adata_len)
{
	eced::Dom d;
	eced::dom_build(alg, adata, adata_len, &d);
	A->dom_len = d.len;
	memcpy(A->dom, d.b, sizeof(A->dom));
}

extern "C" int eds_dom(int alg, const uint8_t *adata, uint32_t adata_len, uint8_t *out)
{
	eced::Dom d;
	eced::dom_build(alg, adata, adata_len, &d);
	memcpy(out, d.b, sizeof(d.b));
	return (int)d.len;
}

extern "C" int eds_slot_ok(uint32_t len, uint32_t stride) { return eced::slot_ok(len, stride) ? 1 : 0; }

extern "C" int eds_expand(int alg, uint32_t n, const uint8_t *sk, const uint8_t *slots, uint32_t stride, const uint8_t *adata, uint32_t adata_len,
			  uint8_t *a, uint8_t *a_wide, uint8_t *r_hash, uint8_t *ph, uint8_t *bad)
{
	EcamdEddsaSignArgs A;
	memset(&A, 0, sizeof(A));
	A.sk = sk;
	A.slots = slots;
	A.stride = stride;
	A.a = a;
	A.a_wide = a_wide;
	A.r_hash = r_hash;
	A.ph = ph;
	A.bad = bad;
	A.n = n;
	eds_set_dom(&A, alg, adata, adata_len);
	return (int)ecamd_launch_eddsa_expand(alg, A, nullptr);
}

extern "C" int eds_hram(int alg, uint32_t n, const uint8_t *R, const uint8_t *Apub, const uint8_t *slots, uint32_t stride, uint8_t *ph,
			const uint8_t *adata, uint32_t adata_len, uint8_t *hram, uint8_t *sigs)
{
	EcamdEddsaSignArgs A;
	memset(&A, 0, sizeof(A));
	A.R = R;
	A.A = Apub;
	A.slots = slots;
	A.stride = stride;
	A.ph = ph;
	A.hram = hram;
	A.sigs = sigs;
	A.n = n;
	eds_set_dom(&A, alg, adata, adata_len);
	return (int)ecamd_launch_eddsa_hram(alg, A, nullptr);
}

extern "C" int eds_fin(int alg, uint32_t n, uint8_t *bad, const uint8_t *stR, const uint8_t *stA, const uint8_t *S, uint8_t *sigs, uint8_t *status)
{
	EcamdEddsaSignArgs A;
	memset(&A, 0, sizeof(A));
	A.bad = bad;
	A.stR = stR;
	A.stA = stA;
	A.S = S;
	A.sigs = sigs;
	A.status = status;
	A.n = n;
	return (int)ecamd_launch_eddsa_sign_fin(alg, A, nullptr);
}

#ifdef EDDSA_SIGN_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

static std::vector<uint8_t> unhex(const std::string &s)
{
	std::vector<uint8_t> v;
	if (s == "-") {
		return v;
	}
	for (size_t i = 0; i + 1 < s.size(); i += 2) {
		v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
	}
	return v;
}

// lines: alg adata msg sk R A want_a want_r_hash want_hram  (hex, "-" for an empty string).  Each item runs as a batch of one with
// a slot of exactly 4 + |msg| rounded up to a word, and heap buffers of the exact output sizes.
int main(int argc, char **argv)
{
	if (argc != 2) {
		return 2;
	}
	FILE *f = fopen(argv[1], "r");
	if (!f) {
		return 2;
	}
	static char w[9][16384];
	int items = 0, bad_items = 0;
	int alg;
	while (fscanf(f, "%d %16383s %16383s %16383s %16383s %16383s %16383s %16383s %16383s", &alg, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]) == 9) {
		const std::vector<uint8_t> adata = unhex(w[0]), msg = unhex(w[1]), sk = unhex(w[2]), R = unhex(w[3]), Apub = unhex(w[4]);
		const std::vector<uint8_t> want_a = unhex(w[5]), want_r = unhex(w[6]), want_h = unhex(w[7]);
		const size_t kl = eced::alg_is448(alg) ? 57 : 32, hl = 2 * kl;
		const uint32_t stride = 4 + (uint32_t)((msg.size() + 3) / 4 * 4);
		std::vector<uint8_t> slot(stride, 0);
		const uint32_t ml = (uint32_t)msg.size();
		memcpy(slot.data(), &ml, 4);
		if (ml) {
			memcpy(slot.data() + 4, msg.data(), ml);
		}
		std::vector<uint8_t> a(kl), aw(hl), rh(hl), ph(64), bad(1), hram(hl), sig(2 * kl);
		int rc = eds_expand(alg, 1, sk.data(), slot.data(), stride, adata.data(), (uint32_t)adata.size(), a.data(), aw.data(), rh.data(), ph.data(),
				    bad.data());
		rc |= eds_hram(alg, 1, R.data(), Apub.data(), slot.data(), stride, ph.data(), adata.data(), (uint32_t)adata.size(), hram.data(), sig.data());
		std::vector<uint8_t> want_aw(want_a);
		want_aw.resize(hl, 0);
		const bool ok = rc == 0 && bad[0] == 0 && a == want_a && aw == want_aw && rh == want_r && hram == want_h &&
				memcmp(sig.data(), R.data(), kl) == 0;
		items++;
		bad_items += ok ? 0 : 1;
	}
	fclose(f);
	printf("%d items, %d bad\n", items, bad_items);
	return bad_items ? 1 : 0;
}
#endif
