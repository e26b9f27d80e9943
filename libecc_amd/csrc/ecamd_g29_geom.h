// libecc_amd/csrc/ecamd_g29_geom.h -- the geometry of the radix-2^29 units as the host sees it: how many words of scratch an item takes,
// how long a scalar may be, how large a curve's constant image is, per (|p|, flavour).  ONE formula each: ecamd_g29_dispatch.cpp
// returns them to the host layer, which sizes its buffers with them, and every unit (ecamd_g29_kernel.hip) asserts at compile time
// that they are what its kernels index with.  Host and device code; nothing here depends on a unit's -D flags (the flavour is an
// argument: g29::nl_for_flavour, ecamd_u29g.h).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ecamd_u29g.h"

namespace g29 {

constexpr int geom_slots() { return 8; }   // constant slots per unit
// scratch words per item of the window kernels: the Jacobian table and the recoded scalar behind it
constexpr uint32_t geom_table_words(int pbits, int flavour)
{
	const uint32_t nw = (uint32_t)((pbits + 31) / 32);
	return 8u * (uint32_t)(((3 * nl_for_flavour(pbits, flavour) + 3) / 4) * 4) + ((2u * nw + 2u + 3u) / 4u) * 4u;
}
// affine window table of the mixed-addition pipeline: 8 entries of 2 NL digits, padded to 16 bytes
constexpr uint32_t geom_affine_words(int pbits, int flavour) { return 8u * (uint32_t)(((2 * nl_for_flavour(pbits, flavour) + 3) / 4) * 4); }
constexpr uint32_t geom_max_slen(int pbits) { return 8u * (uint32_t)((pbits + 31) / 32) + 4u; }
constexpr uint32_t geom_comb_max_slen(int pbits) { return 4u * (uint32_t)((pbits + 31) / 32); }
constexpr size_t geom_image_bytes(int pbits, int flavour) { return (size_t)((10 + NBIAS) * nl_for_flavour(pbits, flavour) + 4) * 4; }
// comb table geometry: 2 NW windows of 32768 entries + 1, entry = 2 NL digits padded to 4 words
constexpr uint32_t geom_comb_entries(int pbits) { return (uint32_t)(2 * ((pbits + 31) / 32)) * 32768u + 1u; }
constexpr uint32_t geom_comb_entry_words(int pbits, int flavour) { return (uint32_t)(((2 * nl_for_flavour(pbits, flavour) + 3) / 4) * 4); }
// the bucket evaluation's affine point record: the next power of two above its 2 NL digits
constexpr uint32_t geom_bkt_point_words(int pbits, int flavour)
{
	const uint32_t w = (uint32_t)(((2 * nl_for_flavour(pbits, flavour) + 3) / 4) * 4);
	return w <= 16 ? 16u : (w <= 32 ? 32u : (w <= 64 ? 64u : 128u));
}
// a Jacobian record of the multi-scalar kernels: a table entry and the "is infinity" word
constexpr uint32_t geom_msm_rec_words(int pbits, int flavour) { return (uint32_t)(((3 * nl_for_flavour(pbits, flavour) + 3) / 4) * 4) + 4u; }

}  // namespace g29
