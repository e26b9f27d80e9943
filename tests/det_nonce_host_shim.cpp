// Host build (g++, no HIP) of libecc_amd/csrc/ecamd_dbign_nonce.h and ecamd_bip0340_nonce.h for tests/test_det_nonce_host.py: the two
// generators on plain arrays (ts = 1), DBIGN's with the plain table and with ScanTab.  With -DDET_NONCE_MAIN it is a stand-alone
// program that runs a file of items (built under -fsanitize=address,undefined by the test).  Test infrastructure, not product code.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../libecc_amd/csrc/ecamd_dbign_nonce.h"
#include "../libecc_amd/csrc/ecamd_bip0340_nonce.h"

static const uint8_t belt_h[256] __attribute__((aligned(16))) = {ECAMD_BELT_H};
static const uint32_t k256[64] = {ECAMD_SHA256_K};
static const uint64_t k512[80] = {ECAMD_SHA512_K};

// DBIGN: q as 17 little-endian words; k out: qlen octets big-endian.  Returns the status, -1 for arguments out of range
extern "C" int dn_dbign_nonce(int scan, const uint8_t *priv, const uint32_t *q, uint32_t qbits, const uint8_t *dig, uint32_t hlen, const uint8_t *oid,
			      uint32_t oid_len, const uint8_t *t, uint32_t t_len, uint8_t *k_out, uint32_t *rejects)
{
	const uint32_t qlen = (qbits + 7) / 8;
	if (qlen == 0 || qlen > (uint32_t)ecdbign::MAX_QLEN || hlen == 0 || hlen > (uint32_t)ecdbign::MAX_DIGEST || oid_len > (uint32_t)ecdbign::MAX_OID ||
	    t_len > (uint32_t)ecdbign::MAX_T) {
		return -1;
	}
	uint32_t tb[ecdbign::IN_WORDS], k[ecdbign::NL];
	int st;
	if (scan) {
		uint32_t words[64];
		memcpy(words, belt_h, 256);
		const ecbelt::ScanTab H = {words};
		st = ecdbign::nonce(H, priv, dig, hlen, oid, oid_len, t, t_len, q, qbits, tb, 1, k, rejects);
	} else {
		const uint8_t *H = belt_h;
		st = ecdbign::nonce(H, priv, dig, hlen, oid, oid_len, t, t_len, q, qbits, tb, 1, k, rejects);
	}
	for (int w = 0; w < ecdbign::IN_WORDS; w++) {
		if (tb[w] != 0) {
			return -2;   // the buffer held the key: it must come back zeroed
		}
	}
	ecrfc::limbs_to_be(k, k_out, qlen);
	return st;
}

// F_key(x) through the unrolled and the rolled cipher, with the plain table and with ScanTab: 0 when all agree; out: the block
extern "C" int dn_belt_encrypt4(const uint8_t *key, const uint8_t *block, uint8_t *out)
{
	uint32_t kw[8], x[3][4], words[64];
	memcpy(kw, key, 32);
	memcpy(words, belt_h, 256);
	for (int v = 0; v < 3; v++) {
		memcpy(x[v], block, 16);
	}
	const uint8_t *H = belt_h;
	const ecbelt::ScanTab S = {words};
	ecbelt::encrypt(H, kw, x[0]);
	ecbelt::encrypt_rolled(H, kw, x[1]);
	ecbelt::encrypt(S, kw, x[2]);
	// the scanning table's single look-up, octet by octet
	int bad = 0;
	for (uint32_t i = 0; i < 256; i++) {
		bad |= S[i] != belt_h[i];
	}
	memcpy(out, x[0], 16);
	return bad || memcmp(x[0], x[1], 16) != 0 || memcmp(x[0], x[2], 16) != 0;
}

template <int ALG, typename KT> static void tags(KT Kt, typename ecrfc::Alg<ALG>::W *ta, typename ecrfc::Alg<ALG>::W *tn)
{
	ecbip::tag_hash<ALG>("BIP0340/aux", 11, ta, Kt);
	ecbip::tag_hash<ALG>("BIP0340/nonce", 13, tn, Kt);
}

template <int ALG, typename KT>
static int bip(KT Kt, const uint8_t *priv, const uint8_t *Y, uint32_t clen, const uint8_t *aux, const uint8_t *msg, uint32_t mlen, const uint32_t *q,
	       uint32_t qbits, uint32_t *k)
{
	typename ecrfc::Alg<ALG>::W ta[8], tn[8];
	tags<ALG>(Kt, ta, tn);
	uint32_t tb[ecbip::PRE_WORDS];
	const int st = ecbip::nonce<ALG>(priv, Y, clen, aux, ta, tn, msg, mlen, q, qbits, tb, 1, Kt, k);
	for (int w = 0; w < ecbip::PRE_WORDS; w++) {
		if (tb[w] != 0) {
			return -2;
		}
	}
	return st;
}

// BIP0340: Y = X || Y affine, clen octets each; k out: qlen octets big-endian.  Returns the status, -1 for arguments out of range
extern "C" int dn_bip_nonce(int hash_type, const uint8_t *priv, const uint8_t *Y, uint32_t clen, const uint8_t *aux, const uint8_t *msg, uint32_t mlen,
			    const uint32_t *q, uint32_t qbits, uint8_t *k_out)
{
	const uint32_t qlen = (qbits + 7) / 8;
	if (qlen == 0 || qlen > (uint32_t)ecbip::MAX_QLEN || clen == 0 || clen > (uint32_t)ecbip::MAX_CLEN) {
		return -1;
	}
	uint32_t k[ecbip::NL];
	int st;
	switch (hash_type) {
	case 1: st = bip<224>(k256, priv, Y, clen, aux, msg, mlen, q, qbits, k); break;
	case 2: st = bip<256>(k256, priv, Y, clen, aux, msg, mlen, q, qbits, k); break;
	case 3: st = bip<384>(k512, priv, Y, clen, aux, msg, mlen, q, qbits, k); break;
	case 4: st = bip<512>(k512, priv, Y, clen, aux, msg, mlen, q, qbits, k); break;
	default: return -1;
	}
	ecrfc::limbs_to_be(k, k_out, qlen);
	return st;
}

// H(tag) of the header's one-block hash: hsize octets
extern "C" int dn_tag_hash(int hash_type, const char *tag, uint32_t len, uint8_t *out)
{
	if (len > 55) {
		return -1;
	}
	if (hash_type == 1 || hash_type == 2) {
		uint32_t w[8];
		if (hash_type == 1) {
			ecbip::tag_hash<224>(tag, len, w, k256);
		} else {
			ecbip::tag_hash<256>(tag, len, w, k256);
		}
		for (int t = 0; t < (hash_type == 1 ? 7 : 8); t++) {
			for (int j = 0; j < 4; j++) {
				out[4 * t + j] = (uint8_t)(w[t] >> (24 - 8 * j));
			}
		}
		return 0;
	}
	if (hash_type == 3 || hash_type == 4) {
		uint64_t w[8];
		if (hash_type == 3) {
			ecbip::tag_hash<384>(tag, len, w, k512);
		} else {
			ecbip::tag_hash<512>(tag, len, w, k512);
		}
		for (int t = 0; t < (hash_type == 3 ? 6 : 8); t++) {
			for (int j = 0; j < 8; j++) {
				out[8 * t + j] = (uint8_t)(w[t] >> (56 - 8 * j));
			}
		}
		return 0;
	}
	return -1;
}

extern "C" int dn_slot_ok(uint32_t len, uint32_t stride, uint32_t hsize, uint32_t clen) { return ecbip::slot_ok(len, stride, hsize, clen) ? 1 : 0; }
extern "C" uint32_t dn_blocks(uint32_t hlen) { return ecdbign::blocks(hlen); }

#ifdef DET_NONCE_MAIN
// lines of hex fields ("-" for an empty string):
//   D <qbits> <q> <priv> <digest> <oid> <t> <status> <k> <rejects>
//   B <hash_type> <qbits> <q> <clen> <priv> <Y> <aux> <msg> <status> <k>
// every field becomes a heap block of its exact length, so that a read past one is seen
static uint8_t *field(FILE *f, uint32_t *len)
{
	static char h[8400];
	if (fscanf(f, "%8399s", h) != 1) {
		exit(2);
	}
	const uint32_t n = strcmp(h, "-") == 0 ? 0 : (uint32_t)strlen(h) / 2;
	uint8_t *out = (uint8_t *)malloc(n ? n : 1);
	for (uint32_t i = 0; i < n; i++) {
		unsigned v;
		sscanf(h + 2 * i, "%2x", &v);
		out[i] = (uint8_t)v;
	}
	*len = n;
	return out;
}

static unsigned number(FILE *f)
{
	unsigned v;
	if (fscanf(f, "%u", &v) != 1) {
		exit(2);
	}
	return v;
}

int main(int argc, char **argv)
{
	FILE *f = argc == 2 ? fopen(argv[1], "r") : NULL;
	if (!f) {
		return 2;
	}
	char kind[4];
	int items = 0, bad = 0;
	while (fscanf(f, "%3s", kind) == 1) {
		uint32_t q[17] = {0}, len[8], rej = 0;
		uint8_t *v[8];
		const bool dbign = kind[0] == 'D';
		const unsigned ht = dbign ? 0 : number(f), qbits = number(f);
		v[0] = field(f, &len[0]);                       // q
		for (uint32_t b = 0; b < len[0]; b++) {
			q[b / 4] |= (uint32_t)v[0][len[0] - 1 - b] << (8 * (b % 4));
		}
		const unsigned clen = dbign ? 0 : number(f);
		for (int j = 1; j <= 4; j++) {
			v[j] = field(f, &len[j]);               // D: priv, digest, oid, t;  B: priv, Y, aux, msg
		}
		const unsigned status = number(f);
		v[5] = field(f, &len[5]);                       // k
		uint8_t *k = (uint8_t *)malloc(len[0]);
		if (dbign) {
			const unsigned want_rej = number(f);
			for (int scan = 0; scan < 2; scan++) {
				const int st = dn_dbign_nonce(scan, v[1], q, qbits, v[2], len[2], v[3], len[3], v[4], len[4], k, &rej);
				bad += st != (int)status || memcmp(k, v[5], len[0]) != 0 || rej != want_rej;
			}
		} else {
			const int st = dn_bip_nonce((int)ht, v[1], v[2], clen, v[3], v[4], len[4], q, qbits, k);
			bad += st != (int)status || memcmp(k, v[5], len[0]) != 0;
		}
		free(k);
		for (int j = 0; j <= 5; j++) {
			free(v[j]);
		}
		items++;
	}
	fclose(f);
	printf("%d items, %d bad\n", items, bad);
	return bad ? 1 : 0;
}
#endif
