// libecc_amd/csrc/ecamd_digest_msgs.h -- the digest of one item of a packed, ragged message array, over every hash of ecamd_hmac.h's
// trait.  Compiles for the device (ecamd_digest_msgs.hip: one item per lane) and for the host (tests/digest_msgs_host_shim.cpp).
//
// THE FORMAT.  msgs is one array of octets, offsets n + 1 u64 values: the message of item i is msgs[offsets[i] .. offsets[i + 1]).
// What is hashed for item i is three segments,
//     call_prefix || item_prefix[i] || msgs[off0 .. off1)
// call_prefix: 0 .. MAX_PREFIX octets, the same for every item, held as words (zero behind its last octet);
// item_prefix: item_prefix_len octets (0 .. MAX_PREFIX, one length per call) at any address, read octet by octet;
// msgs:        read as ALIGNED 32-bit words of the array, and only words that hold at least one octet of the item's own message: never
//              below msgs, never at or beyond round_up(total, 4).  An empty message reads nothing.
//
// Source is the functor echm::Hash<ID>::hash() asks for: word t of block b of that stream in memory order, zeros behind its last
// octet.  A segment boundary and the start of the message fall at any octet of a word; the word is the OR of up to three pieces, each
// the four octets of ONE segment at a signed index (zero outside the segment).  A word that lies inside the message -- all of them but
// two, for a long message -- is one aligned load when the message starts on a word of the array, otherwise two loads and a funnel
// shift.
//
// item_ok() decides whether an item is usable: off0 <= off1 <= total, and the whole input at most 2^28 octets (the Merkle-Damgard units
// keep the bit count in one 32-bit word).  digest() gives an item that fails it an all-zero digest and status 1 and reads no octet
// of msgs for it.
//
// Nothing here is secret: messages and prefixes are public inputs of a signature scheme.
#pragma once
#include <stdint.h>
#include "ecamd_hmac.h"

namespace echm_msgs {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum : u32 { MAX_PREFIX = 256, MAX_HASHED = 1u << 28 };

EHM_FN bool item_ok(u64 off0, u64 off1, u64 total, u32 call_prefix_len, u32 item_prefix_len)
{
	if (off0 > off1 || off1 > total || call_prefix_len > (u32)MAX_PREFIX || item_prefix_len > (u32)MAX_PREFIX) {
		return false;
	}
	const u64 mlen = off1 - off0;
	return mlen <= (u64)MAX_HASHED && mlen + call_prefix_len + item_prefix_len <= (u64)MAX_HASHED;
}

// the first `keep` (1 .. 3) octets of a word
EHM_FN u32 low_octets(u32 w, u32 keep) { return w & (0xffffffffu >> (8u * (4u - keep))); }

struct Source {
	const u32 *cp;       // the call prefix as words, readable up to the word that holds its last octet
	const u8 *ip;        // this item's prefix
	const u32 *mw;       // the message array as aligned words
	u64 off0, off1;      // the item's message in the array
	u32 cp_len, ip_len, m_len, len;   // len: the three together

	// the octets [i, i + 4) of the call prefix, i >= 0 and i < cp_len
	EHM_FN u32 cp4(u32 i) const
	{
		const u32 j = i >> 2, s = 8u * (i & 3u), last = (cp_len - 1u) >> 2;
		u32 w = cp[j] >> s;
		if (s != 0u && j < last) {
			w |= cp[j + 1u] << (32u - s);
		}
		const u32 rem = cp_len - i;
		return rem >= 4u ? w : low_octets(w, rem);
	}
	// the octets [i, i + 4) of the item prefix, -3 <= i < ip_len: zero outside the segment
	EHM_FN u32 ip4(int i) const
	{
		u32 w = 0;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const int x = i + k;
			if (x >= 0 && x < (int)ip_len) {
				w |= (u32)ip[x] << (8 * k);
			}
		}
		return w;
	}
	// the octets [i, i + 4) of the message, i >= 0 and i < m_len
	EHM_FN u32 msg4(u32 i) const
	{
		const u64 a = off0 + i, j = a >> 2;
		const u32 s = 8u * ((u32)a & 3u);
		u32 w = mw[j] >> s;
		if (s != 0u && 4u * (j + 1u) < off1) {   // the next word of the array holds an octet of this message
			w |= mw[j + 1u] << (32u - s);
		}
		const u32 rem = m_len - i;
		return rem >= 4u ? w : low_octets(w, rem);
	}

	EHM_FN u32 at(u32 pos) const
	{
		const u32 pre = cp_len + ip_len;
		if (pos >= len) {
			return 0u;
		}
		if (pos >= pre && pos + 4u <= len) {   // inside the message: every word of a long one but the first and the last
			return msg4(pos - pre);
		}
		u32 w = 0;
		if (pos < cp_len) {
			w = cp4(pos);
		}
		if (pos + 4u > cp_len && pos < pre) {
			w |= ip4((int)pos - (int)cp_len);
		}
		if (pos + 4u > pre && m_len != 0u) {
			// the message begins inside this word (at octet pre - pos) or covers it
			w |= pos >= pre ? msg4(pos - pre) : msg4(0u) << (8u * (pre - pos));
		}
		return w;
	}
};

// The digest of one item into out (H::HSIZE octets); returns the item's status: 0, or 1 (all-zero digest, msgs not read) when
// item_ok() refuses it.  cp: the call prefix as words; ip: the item's own prefix; mw: the message array (4-byte aligned).
template <class H, class Env>
EHM_FN int digest(const Env &env, const u32 *cp, u32 cp_len, const u8 *ip, u32 ip_len, const u32 *mw, u64 off0, u64 off1, u64 total, u8 *out)
{
	constexpr u32 BW = (u32)H::BW;
	u32 dw[H::DW];
	const bool ok = item_ok(off0, off1, total, cp_len, ip_len);
	if (!ok) {
#pragma unroll
		for (int t = 0; t < H::DW; t++) {
			dw[t] = 0;
		}
	} else {
		const u32 m_len = (u32)(off1 - off0);
		const Source src{cp, ip, mw, off0, off1, cp_len, ip_len, m_len, cp_len + ip_len + m_len};
		H::hash(env, [&](u32 b, u32 t) -> u32 { return src.at(4u * (b * BW + t)); }, src.len, dw);
	}
	echm::words_to_bytes<H::DW>(dw, out);
	return ok ? 0 : 1;
}

}  // namespace echm_msgs
