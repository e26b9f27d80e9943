// libecc_amd/csrc/ecamd_eddsa_msgs.h -- the hashes of EdDSA per item with the message taken from a packed, ragged array (the format of
// ecamd_digest_msgs.h: msgs[offsets[i] .. offsets[i + 1])), for the five variants of ecamd_eddsa_sign.h.  The streamed SHA-512 / SHAKE256,
// the segments and the four steps are that header's; this one adds the item's validity rule, the stream of a verifier's hash with a
// fresh PH(M) in registers, and the per-item steps.  Compiles for the device (ecamd_eddsa_msgs.hip: one item per lane) and for the host
// (tests/eddsa_msgs_host_shim.cpp, tests/eddsa_msgs_asan_main.cpp).
//
// READS OF msgs.  The message is the segment (msgs + off0, off1 - off0) of eced::mem_word: an 8-octet load only where the word lies wholly
// inside the segment, octet by octet at its two ends.  No octet outside [off0, off1) is read for the item, whatever off0 mod 8 is; an
// unusable item (item_ok) reads none at all.
//
// SECRET DATA as in ecamd_eddsa_sign.h; message lengths and offsets are public.
#pragma once
#include "ecamd_eddsa_sign.h"

namespace eced_msgs {

using eced::u8;
using eced::u32;
using eced::u64;
using eced::Var;

enum : u32 { MAX_HASHED = 1u << 28 };   // echm_msgs::MAX_HASHED: stream lengths are u32 and SHA-512's bit count stays below 2^32

// The item is usable: off0 <= off1 <= total, and the longest input the call hashes for it is at most 2^28 octets -- the message alone for
// the PH variants (their other inputs are a few hundred octets), dom || R || A || M otherwise.
template <int ALG> ECR_FN bool item_ok(u64 off0, u64 off1, u64 total, u32 dlen)
{
	if (off0 > off1 || off1 > total) {
		return false;
	}
	const u64 mlen = off1 - off0, fixed = Var<ALG>::PH ? 0u : (u64)dlen + 2u * (u64)Var<ALG>::KLEN;
	return mlen <= (u64)MAX_HASHED && mlen + fixed <= (u64)MAX_HASHED;   // (the first test: the sum must not wrap)
}

// the item's message: *bad = 1 and an empty message at msgs itself for an unusable item
template <int ALG> ECR_FN const u8 *message(const u8 *msgs, u64 msgs_len, const u64 *offsets, u32 i, u32 dlen, u32 *mlen, u32 *bad)
{
	const u64 off0 = offsets[i], off1 = offsets[i + 1];
	const bool ok = item_ok<ALG>(off0, off1, msgs_len, dlen);
	*bad = ok ? 0u : 1u;
	*mlen = ok ? (u32)(off1 - off0) : 0u;
	return ok ? msgs + off0 : msgs;
}

// dom || R || A || PH(M) with PH(M) in registers: HStream's first three segments, then RStream's register tail
struct HRStream {
	const u8 *dom;
	u32 dlen;
	const u8 *R, *A;
	u32 klen;
	const u64 *ph;
	template <bool BE> ECR_FN u64 word(u32 g) const
	{
		return eced::mem_word<BE>(dom, 0, dlen, g) | eced::mem_word<BE>(R, dlen, klen, g) | eced::mem_word<BE>(A, dlen + klen, klen, g) |
		       eced::reg_word<BE, eced::PH_LEN / 8>(ph, dlen + 2 * klen, g);
	}
	ECR_FN u32 total() const { return dlen + 2 * klen + (u32)eced::PH_LEN; }
};

// A verifier's hram = H(dom || R || A || M), or H(dom || R || A || PH(M)) with PH(M) computed here and kept in registers: HLEN octets
template <int ALG, typename KT> ECR_FN void verify_hram(const u8 *dom, u32 dlen, const u8 *R, const u8 *A, const u8 *msg, u32 mlen, u8 *out, KT kt)
{
	if constexpr (Var<ALG>::PH) {
		u64 ph[eced::PH_LEN / 8];
		eced::prehash<ALG>(msg, mlen, ph, kt);
		const HRStream src = {dom, dlen, R, A, (u32)Var<ALG>::KLEN, ph};
		eced::hash_out<ALG>(src, out, kt);
	} else {
		eced::hram<ALG>(dom, dlen, R, A, msg, mlen, out, kt);
	}
}

// A signer's first hash, r_hash = H(dom || prefix || M-or-PH(M)): HLEN octets; the PH variants store PH(M) (64 octets, public) at ph_out
// for the second hash
template <int ALG, typename KT>
ECR_FN void sign_r_hash(const u8 *dom, u32 dlen, const u64 *prefix, const u8 *msg, u32 mlen, u8 *ph_out, u8 *out, KT kt)
{
	if constexpr (Var<ALG>::PH) {
		u64 ph[eced::PH_LEN / 8];
		eced::prehash<ALG>(msg, mlen, ph, kt);
		eced::words_out<!Var<ALG>::IS448>(ph, ph_out, eced::PH_LEN);
		eced::r_hash<ALG>(dom, dlen, prefix, nullptr, 0, ph, out, kt);
	} else {
		eced::r_hash<ALG>(dom, dlen, prefix, msg, mlen, nullptr, out, kt);
	}
}

}  // namespace eced_msgs
