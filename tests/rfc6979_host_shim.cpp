// Host build of libecc_amd/csrc/ecamd_rfc6979.h (g++, no HIP) for tests/test_rfc6979_host.py: the HMAC of the header on a message of
// any length, and the generator item by item.  With -DRFC6979_MAIN it is a stand-alone program (its own main) that reads items from
// a text file -- one per line: hash_type qbits q x digest k retries, hex -- runs the generator and compares; that form is built under
// -fsanitize=address,undefined and run as a child process.  Test infrastructure, not product code.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../libecc_amd/csrc/ecamd_rfc6979.h"

static const uint32_t K256[64] = {ECAMD_SHA256_K};
static const uint64_t K512[80] = {ECAMD_SHA512_K};

template <int ALG> struct Tab;
template <> struct Tab<224> { static const uint32_t *get() { return K256; } };
template <> struct Tab<256> { static const uint32_t *get() { return K256; } };
template <> struct Tab<384> { static const uint64_t *get() { return K512; } };
template <> struct Tab<512> { static const uint64_t *get() { return K512; } };

// HMAC with a key of hsize octets over msg, through Hmac<ALG>::set_key and ::of_v_tail (vw = 0): the path steps d and f take
template <int ALG> static void hmac_any(const uint8_t *key, const uint8_t *msg, uint32_t len, uint8_t *out)
{
	typedef typename ecrfc::Alg<ALG>::W W;
	constexpr int VW = ecrfc::Hmac<ALG>::VW, WB = (int)sizeof(W);
	W K[8] = {0}, o[8];
	for (int t = 0; t < VW; t++) {
		for (int b = 0; b < WB; b++) {
			K[t] = (W)((K[t] << 8) | key[t * WB + b]);
		}
	}
	// exactly the words of_v_tail reads: the blocks of the padded message
	const uint32_t nb = (len + 1 + ecrfc::Alg<ALG>::LENF + ecrfc::Alg<ALG>::BLOCK - 1) / ecrfc::Alg<ALG>::BLOCK;
	std::vector<uint32_t> tb((size_t)nb * ecrfc::Alg<ALG>::BLOCK / 4, 0u);
	for (uint32_t i = 0; i < len; i++) {
		ecrfc::tb_or(tb.data(), 1, i, msg[i]);
	}
	ecrfc::tb_or(tb.data(), 1, len, 0x80u);
	ecrfc::Hmac<ALG> hm;
	hm.set_key(K, Tab<ALG>::get());
	hm.of_v_tail(K, 0, tb.data(), 1, len, o, Tab<ALG>::get());
	for (int t = 0; t < VW; t++) {
		for (int b = 0; b < WB; b++) {
			out[t * WB + b] = (uint8_t)(o[t] >> (8 * (WB - 1 - b)));
		}
	}
}

template <int ALG> static int nonce_one(const uint8_t *priv, const uint8_t *dig, const uint32_t *q, uint32_t qbits, uint8_t *k_be, uint32_t *retries)
{
	// the word buffer exactly as long as the header says it is, on the heap: the sanitized build sees every access past it
	std::vector<uint32_t> tb(ecrfc::TAIL_WORDS, 0xa5a5a5a5u);
	uint32_t k[ecrfc::NL];
	const int st = ecrfc::nonce<ALG>(priv, dig, q, qbits, tb.data(), 1, Tab<ALG>::get(), k, retries);
	ecrfc::limbs_to_be(k, k_be, (qbits + 7) / 8);
	for (uint32_t w : tb) {
		if (w != 0) {
			return -2;   // the buffer held secrets: it must come back zeroed
		}
	}
	return st;
}

extern "C" {
int r_hash_size(int hash_type) { return ecrfc::hash_size(hash_type); }
int r_slot_ok(uint32_t len, uint32_t stride) { return ecrfc::slot_ok(len, stride) ? 1 : 0; }
int r_hmac(int hash_type, const uint8_t *key, const uint8_t *msg, uint32_t len, uint8_t *out)
{
	switch (hash_type) {
	case 1: hmac_any<224>(key, msg, len, out); return 0;
	case 2: hmac_any<256>(key, msg, len, out); return 0;
	case 3: hmac_any<384>(key, msg, len, out); return 0;
	case 4: hmac_any<512>(key, msg, len, out); return 0;
	}
	return -1;
}
// q: 17 little-endian words; priv: qlen octets; dig: hsize octets; k_be: qlen octets out.  Returns the generator's status (-1: hash_type)
int r_nonce(int hash_type, const uint8_t *priv, const uint8_t *dig, const uint32_t *q, uint32_t qbits, uint8_t *k_be, uint32_t *retries)
{
	switch (hash_type) {
	case 1: return nonce_one<224>(priv, dig, q, qbits, k_be, retries);
	case 2: return nonce_one<256>(priv, dig, q, qbits, k_be, retries);
	case 3: return nonce_one<384>(priv, dig, q, qbits, k_be, retries);
	case 4: return nonce_one<512>(priv, dig, q, qbits, k_be, retries);
	}
	return -1;
}
}

#ifdef RFC6979_MAIN
static std::vector<uint8_t> unhex(const char *s)
{
	std::vector<uint8_t> v;
	for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
		unsigned b;
		sscanf(s + i, "%2x", &b);
		v.push_back((uint8_t)b);
	}
	return v;
}

int main(int argc, char **argv)
{
	if (argc != 2) {
		fprintf(stderr, "usage: %s items.txt\n", argv[0]);
		return 2;
	}
	FILE *f = fopen(argv[1], "r");
	if (!f) {
		return 2;
	}
	static char sq[512], sx[512], sd[512], sk[512];
	int ht, n = 0, bad = 0;
	unsigned qbits, want_retries;
	while (fscanf(f, "%d %u %500s %500s %500s %500s %u", &ht, &qbits, sq, sx, sd, sk, &want_retries) == 7) {
		// every input in a heap block of its exact size
		const std::vector<uint8_t> qb = unhex(sq), x = unhex(sx), d = unhex(sd), kw = unhex(sk);
		std::vector<uint32_t> q(ecrfc::NL, 0u);
		for (size_t i = 0; i < qb.size(); i++) {
			q[i / 4] |= (uint32_t)qb[qb.size() - 1 - i] << (8 * (i % 4));
		}
		std::vector<uint8_t> k((qbits + 7) / 8);
		uint32_t retries = 0;
		const int st = r_nonce(ht, x.data(), d.data(), q.data(), qbits, k.data(), &retries);
		if (st != 0 || k != kw || retries != want_retries) {
			bad++;
		}
		n++;
	}
	fclose(f);
	printf("%d items, %d bad\n", n, bad);
	return bad ? 1 : 0;
}
#endif
