// libecc_amd/csrc/ecamd_g29_dispatch.cpp -- host-side routing of the radix-2^29 units: (|p|, flavour) -> the entry points of the
// unit that ecamd_g29_kernel.hip was compiled as for it (libecc_amd/build.py), and the units' geometry (ecamd_g29_geom.h) for the
// host layer.  No kernel here.
#include "ecamd_internal.h"
#include "ecamd_g29_geom.h"

// Every unit once: X(tag, |p|, flavour).  A dense unit (flavour 0) serves any prime of its size; 'flavour' 1 selects the secp521r1
// (p = 2^521 - 1) instantiation, 2 the p = 2^255 - 19 one, 3 secp384r1's, 4 secp256k1's, 5 WEI448's, 6 secp224r1's, 7 secp192r1's.
#define G29_DENSE_UNITS(X) \
	X(192, 192, 0) X(224, 224, 0) X(255, 255, 0) X(256, 256, 0) X(320, 320, 0) X(384, 384, 0) X(448, 448, 0) X(511, 511, 0) X(512, 512, 0) X(521, 521, 0)
#define G29_FLAVOURED_UNITS(X) X(521m, 521, 1) X(255c, 255, 2) X(384n, 384, 3) X(256k, 256, 4) X(448g, 448, 5) X(224s, 224, 6) X(192s, 192, 7)
#define G29_UNITS(X) G29_DENSE_UNITS(X) G29_FLAVOURED_UNITS(X)

#define X(TAG, PB, FLAV) \
	hipError_t ecamd_g29_upload_##TAG(int slot, const void *img, size_t bytes); \
	hipError_t ecamd_g29_launch_##TAG(int gslot, const EcamdSmulArgs &a, hipStream_t s, hipEvent_t *ev); \
	hipError_t ecamd_g29_comb_build_##TAG(int gslot, const uint8_t *pts, uint32_t n, uint32_t clen, uint32_t *table, hipStream_t s); \
	hipError_t ecamd_g29_msm_##TAG(int gslot, int phase, const EcamdMsmArgs &a, uint32_t *tmp, const uint8_t *gen, const uint8_t *gen_status, \
				       uint8_t *verdict, uint32_t *sum_out, hipStream_t s); \
	hipError_t ecamd_g29_prj_import_##TAG(int gslot, const EcamdPrjInArgs &a, hipStream_t s);
G29_UNITS(X)
#undef X
// (the dense units alone have the mod-q preparation, the two Edwards units alone the EdDSA tail)
#define X(TAG, PB, FLAV) hipError_t ecamd_g29_ecdsa_prep_##TAG(int qgslot, const EcamdEcdsaPrepArgs &a, uint32_t *scratch, int kp, hipStream_t s);
G29_DENSE_UNITS(X)
#undef X
hipError_t ecamd_g29_ed_fin_255c(int gslot, const EcamdEdFinArgs &a, hipStream_t s);
hipError_t ecamd_g29_ed_fin_448g(int gslot, const EcamdEdFinArgs &a, hipStream_t s);

namespace {
struct G29Unit {
	int pbits, flavour;
	hipError_t (*upload)(int slot, const void *img, size_t bytes);
	hipError_t (*launch)(int gslot, const EcamdSmulArgs &a, hipStream_t s, hipEvent_t *ev);
	hipError_t (*comb_build)(int gslot, const uint8_t *pts, uint32_t n, uint32_t clen, uint32_t *table, hipStream_t s);
	hipError_t (*msm)(int gslot, int phase, const EcamdMsmArgs &a, uint32_t *tmp, const uint8_t *gen, const uint8_t *gen_status, uint8_t *verdict,
			  uint32_t *sum_out, hipStream_t s);
	hipError_t (*prj_import)(int gslot, const EcamdPrjInArgs &a, hipStream_t s);
};
const G29Unit g29_units[] = {
#define X(TAG, PB, FLAV) {PB, FLAV, ecamd_g29_upload_##TAG, ecamd_g29_launch_##TAG, ecamd_g29_comb_build_##TAG, ecamd_g29_msm_##TAG, ecamd_g29_prj_import_##TAG},
	G29_UNITS(X)
#undef X
};

// the unit of that prime when the flavour names one, else the dense unit of the size (a flavour that does not belong to the size
// falls there too), else none
const G29Unit *g29_unit(int pbits, int flavour)
{
	const G29Unit *dense = nullptr;
	for (const G29Unit &u : g29_units) {
		if (u.pbits != pbits) {
			continue;
		}
		if (u.flavour == 0) {
			dense = &u;
		} else if (u.flavour == flavour) {
			return &u;
		}
	}
	return dense;
}
}  // namespace

// the tail of an EdDSA verification on the 2^255 - 19 (flavour 2) or the Goldilocks (flavour 5) unit
hipError_t ecamd_launch_ed_fin_g29(int flavour, int gslot, const EcamdEdFinArgs &a, hipStream_t s)
{
	if (flavour == 2) {
		return ecamd_g29_ed_fin_255c(gslot, a, s);
	}
	if (flavour == 5) {
		return ecamd_g29_ed_fin_448g(gslot, a, s);
	}
	return hipErrorInvalidValue;
}

int ecamd_g29_supported(int pbits) { return g29_unit(pbits, 0) != nullptr; }   // (every size has its dense unit)
int ecamd_g29_nl(int pbits, int flavour) { return g29::nl_for_flavour(pbits, flavour); }
int ecamd_g29_slots(void) { return g29::geom_slots(); }
uint32_t ecamd_g29_table_words(int pbits, int flavour) { return g29::geom_table_words(pbits, flavour); }
uint32_t ecamd_g29_affine_words(int pbits, int flavour) { return g29::geom_affine_words(pbits, flavour); }
uint32_t ecamd_g29_max_slen(int pbits) { return g29::geom_max_slen(pbits); }
uint32_t ecamd_g29_comb_max_slen(int pbits) { return g29::geom_comb_max_slen(pbits); }
size_t ecamd_g29_image_bytes(int pbits, int flavour) { return g29::geom_image_bytes(pbits, flavour); }
uint32_t ecamd_g29_comb_entries(int pbits) { return g29::geom_comb_entries(pbits); }
uint32_t ecamd_g29_comb_entry_words(int pbits, int flavour) { return g29::geom_comb_entry_words(pbits, flavour); }
uint32_t ecamd_g29_bkt_point_words(int pbits, int flavour) { return g29::geom_bkt_point_words(pbits, flavour); }
uint32_t ecamd_g29_msm_rec_words(int pbits, int flavour) { return g29::geom_msm_rec_words(pbits, flavour); }

hipError_t ecamd_g29_upload(int pbits, int slot, const void *img, size_t bytes, int flavour)
{
	const G29Unit *u = g29_unit(pbits, flavour);
	return u ? u->upload(slot, img, bytes) : hipErrorInvalidValue;
}

hipError_t ecamd_launch_smul_g29(int pbits, int gslot, const EcamdSmulArgs &a, hipStream_t s, hipEvent_t *ev, int flavour)
{
	if (a.n == 0) {
		return hipSuccess;
	}
	const G29Unit *u = g29_unit(pbits, flavour);
	return u ? u->launch(gslot, a, s, ev) : hipErrorInvalidValue;
}

// k_ecdsa_prep_g on the dense unit of qbits bits (the order q in constant slot qgslot of that unit); scratch: n x ecamd_g29_nl(qbits, 0) words
hipError_t ecamd_g29_ecdsa_prep(int qbits, int qgslot, const EcamdEcdsaPrepArgs &a, uint32_t *scratch, int kp, hipStream_t s)
{
	switch (qbits) {
#define X(TAG, PB, FLAV) case PB: return ecamd_g29_ecdsa_prep_##TAG(qgslot, a, scratch, kp, s);
		G29_DENSE_UNITS(X)
#undef X
	default: return hipErrorInvalidValue;
	}
}

// the Schnorr-type multi-scalar multiplication on the unit (pbits, flavour)
hipError_t ecamd_launch_msm_g29(int pbits, int gslot, int flavour, int phase, const EcamdMsmArgs &a, uint32_t *tmp, const uint8_t *gen,
				const uint8_t *gen_status, uint8_t *verdict, uint32_t *sum_out, hipStream_t s)
{
	const G29Unit *u = g29_unit(pbits, flavour);
	return u ? u->msm(gslot, phase, a, tmp, gen, gen_status, verdict, sum_out, s) : hipErrorInvalidValue;
}

// k_prj_import_g on the unit (pbits, flavour)
hipError_t ecamd_g29_prj_import(int pbits, int gslot, const EcamdPrjInArgs &a, hipStream_t s, int flavour)
{
	const G29Unit *u = g29_unit(pbits, flavour);
	return u ? u->prj_import(gslot, a, s) : hipErrorInvalidValue;
}

hipError_t ecamd_g29_comb_build(int pbits, int gslot, const uint8_t *pts, uint32_t n, uint32_t clen, uint32_t *table,
				hipStream_t s, int flavour)
{
	const G29Unit *u = g29_unit(pbits, flavour);
	return u ? u->comb_build(gslot, pts, n, clen, table, s) : hipErrorInvalidValue;
}
