// tests/g29_dispatch_host_shim.cpp -- stand-alone host program around libecc_amd/csrc/ecamd_g29_dispatch.cpp (compiled beside it by
// tests/test_g29_dispatch_host.py): every per-unit entry point is a stub that records its own name and returns hipSuccess, so the
// program can print where each (|p|, flavour) pair is routed and what the geometry functions answer.  Nothing here calls into HIP.
#include <stdio.h>
#include "../libecc_amd/csrc/ecamd_internal.h"

static const char *g_reached;
static int g_calls;
static hipError_t reach(const char *name)
{
	g_reached = name;
	g_calls++;
	return hipSuccess;
}

// the units, written out here on their own (not through the dispatcher's list)
#define UNIT(TAG) \
	hipError_t ecamd_g29_upload_##TAG(int, const void *, size_t) { return reach("upload:" #TAG); } \
	hipError_t ecamd_g29_launch_##TAG(int, const EcamdSmulArgs &, hipStream_t, hipEvent_t *) { return reach("launch:" #TAG); } \
	hipError_t ecamd_g29_comb_build_##TAG(int, const uint8_t *, uint32_t, uint32_t, uint32_t *, hipStream_t) { return reach("comb_build:" #TAG); } \
	hipError_t ecamd_g29_msm_##TAG(int, int, const EcamdMsmArgs &, uint32_t *, const uint8_t *, const uint8_t *, uint8_t *, uint32_t *, hipStream_t) \
	{ \
		return reach("msm:" #TAG); \
	} \
	hipError_t ecamd_g29_prj_import_##TAG(int, const EcamdPrjInArgs &, hipStream_t) { return reach("prj_import:" #TAG); }
#define DENSE(TAG) \
	UNIT(TAG) \
	hipError_t ecamd_g29_ecdsa_prep_##TAG(int, const EcamdEcdsaPrepArgs &, uint32_t *, int, hipStream_t) { return reach("ecdsa_prep:" #TAG); }
DENSE(192)
DENSE(224)
DENSE(255)
DENSE(256)
DENSE(320)
DENSE(384)
DENSE(448)
DENSE(511)
DENSE(512)
DENSE(521)
UNIT(521m)
UNIT(255c)
UNIT(384n)
UNIT(256k)
UNIT(448g)
UNIT(224s)
UNIT(192s)
hipError_t ecamd_g29_ed_fin_255c(int, const EcamdEdFinArgs &, hipStream_t) { return reach("ed_fin:255c"); }
hipError_t ecamd_g29_ed_fin_448g(int, const EcamdEdFinArgs &, hipStream_t) { return reach("ed_fin:448g"); }

// one line per call: what was called, with which pair, what it returned, which stub it reached ("-": none) and how many
static void report(const char *fn, int pbits, int flavour, hipError_t e)
{
	printf("route %s %d %d %d %s %d\n", fn, pbits, flavour, (int)e, g_calls ? g_reached : "-", g_calls);
	g_reached = nullptr;
	g_calls = 0;
}

int main()
{
	static const int PBITS[] = {0, 160, 191, 192, 224, 255, 256, 257, 320, 384, 448, 511, 512, 521, 522};
	EcamdSmulArgs smul = {}, smul0 = {};
	EcamdMsmArgs msm = {};
	EcamdPrjInArgs prj = {};
	EcamdEcdsaPrepArgs prep = {};
	EcamdEdFinArgs fin = {};
	uint8_t img[4] = {0};
	smul.n = 1;
	printf("codes %d %d\n", (int)hipSuccess, (int)hipErrorInvalidValue);
	for (int pb : PBITS) {
		for (int fl = -1; fl <= 8; fl++) {
			report("upload", pb, fl, ecamd_g29_upload(pb, 0, img, sizeof(img), fl));
			report("launch", pb, fl, ecamd_launch_smul_g29(pb, 0, smul, nullptr, nullptr, fl));
			report("launch_n0", pb, fl, ecamd_launch_smul_g29(pb, 0, smul0, nullptr, nullptr, fl));
			report("msm", pb, fl, ecamd_launch_msm_g29(pb, 0, fl, 0, msm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
			report("prj_import", pb, fl, ecamd_g29_prj_import(pb, 0, prj, nullptr, fl));
			report("comb_build", pb, fl, ecamd_g29_comb_build(pb, 0, nullptr, 1, 0, nullptr, nullptr, fl));
			printf("geom %d %d %u %u %u %u %u %zu %u %u %d %u\n", pb, fl, ecamd_g29_table_words(pb, fl), ecamd_g29_affine_words(pb, fl),
			       ecamd_g29_comb_entry_words(pb, fl), ecamd_g29_bkt_point_words(pb, fl), ecamd_g29_msm_rec_words(pb, fl),
			       ecamd_g29_image_bytes(pb, fl), ecamd_g29_max_slen(pb), ecamd_g29_comb_max_slen(pb), ecamd_g29_nl(pb, fl),
			       ecamd_g29_comb_entries(pb));
		}
		report("ecdsa_prep", pb, 0, ecamd_g29_ecdsa_prep(pb, 0, prep, nullptr, 1, nullptr));
		printf("supported %d %d\n", pb, ecamd_g29_supported(pb));
	}
	for (int fl = -1; fl <= 8; fl++) {
		report("ed_fin", 0, fl, ecamd_launch_ed_fin_g29(fl, 0, fin, nullptr));
	}
	printf("slots %d\n", ecamd_g29_slots());
	return 0;
}
