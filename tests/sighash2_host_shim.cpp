// tests/sighash2_host_shim.cpp -- libecc_amd/csrc/ecamd_sm3.h, ecamd_streebog.h and ecamd_sm2z.h compiled for the host (g++, no HIP), so
// that tests/test_sighash2_host.py can run the per-item hash code of k_sm3_slots, k_streebog_slots and k_sm2_z against the recorded
// reference answers without a GPU.  Built twice: as a shared library for ctypes, and with -DSIGHASH2_MAIN as a stand-alone program
// (its own main, for -fsanitize=address,undefined) that reads vectors from a text file:
//     H <hash_type> <message hex or -> <digest hex>
//     Z <hash_type> <id hex or -> <a hex> <b hex> <gx hex> <gy hex> <key hex> <Z hex>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../libecc_amd/csrc/ecamd_sm3.h"
#include "../libecc_amd/csrc/ecamd_streebog.h"
#include "../libecc_amd/csrc/ecamd_sm2z.h"

static const uint8_t k_pi[256] = {ECAMD_STREEBOG_PI};
static const uint64_t k_a[64] = {ECAMD_STREEBOG_A};
static const uint64_t k_c[96] = {ECAMD_STREEBOG_C};
static const uint32_t k_256[64] = {ECAMD_SHA256_K};
static const uint64_t k_512[80] = {ECAMD_SHA512_K};

// the table as the kernel builds it in LDS
static const uint64_t *table()
{
	static uint64_t T[ecsb::TABLE_WORDS];
	static bool built = false;
	if (!built) {
		for (uint32_t e = 0; e < (uint32_t)ecsb::TABLE_WORDS; e++) {
			T[e] = ecsb::table_entry(k_pi, k_a, e >> 8, e & 255u);
		}
		built = true;
	}
	return T;
}

// the message as the words of a slot: exactly the words that hold its octets (a read past them is the sanitizer's to find)
static std::vector<uint32_t> words_of(const uint8_t *msg, uint32_t len)
{
	std::vector<uint32_t> w((len + 3) / 4 + (len == 0 ? 1 : 0), 0);
	if (len) {
		memcpy(w.data(), msg, len);
	}
	return w;
}

extern "C" {

// hash_type 11, 13, 14: the one-shot of the slot kernels.  Returns the digest length, 0 for another hash_type.
int s2_hash(int hash_type, const uint8_t *msg, uint32_t len, uint8_t *out)
{
	const std::vector<uint32_t> w = words_of(msg, len);
	if (hash_type == 11) {
		uint32_t dg[8];
		ecsm3::hash_words(w.data(), len, dg);
		ecsm3::digest_bytes(dg, out);
		return 32;
	}
	uint64_t h[8];
	if (hash_type == 13) {
		ecsb::hash_words<256>(table(), k_c, w.data(), len, h);
		ecsb::digest_bytes<256>(h, out);
		return 32;
	}
	if (hash_type == 14) {
		ecsb::hash_words<512>(table(), k_c, w.data(), len, h);
		ecsb::digest_bytes<512>(h, out);
		return 64;
	}
	return 0;
}

// SM3 through the streamed form: whole blocks absorbed, the rest finished
int s2_sm3_streamed(const uint8_t *msg, uint32_t len, uint8_t *out)
{
	uint32_t st[8];
	ecsm3::init(st);
	uint32_t off = 0;
	for (; off + 64 <= len; off += 64) {
		ecsm3::absorb(st, msg + off);
	}
	const uint8_t *rest = msg + off;
	ecsm3::finish(st, off, len - off, [rest](uint32_t pos) { return rest[pos]; });
	ecsm3::digest_bytes(st, out);
	return 32;
}

// one entry of the combined table, for the test that pins its definition
uint64_t s2_table_entry(uint32_t j, uint32_t b) { return table()[256 * j + b]; }

// SM2's Z as the host and the kernel split it: prefix_init, then z_item.  Returns the digest length, -1 where prefix_init refuses.
int s2_sm2_z(int hash_type, const uint8_t *id, uint32_t id_len, const uint8_t *a, const uint8_t *b, const uint8_t *gx, const uint8_t *gy,
	     uint32_t clen, const uint8_t *key, uint8_t *out, uint32_t *absorbed, uint32_t *tail_len)
{
	ecsm2z::Prefix P;
	if (ecsm2z::prefix_init(P, hash_type, id, id_len, a, b, gx, gy, clen, k_256, k_512)) {
		return -1;
	}
	if (absorbed) {
		*absorbed = P.absorbed;
	}
	if (tail_len) {
		*tail_len = P.tail_len;
	}
	ecsm2z::z_item(P, key, 2 * clen, out, k_256, k_512);
	return ecsm2z::hash_size(hash_type);
}

}  // extern "C"

#ifdef SIGHASH2_MAIN
static std::vector<uint8_t> unhex(const std::string &s)
{
	std::vector<uint8_t> out;
	if (s == "-") {
		return out;
	}
	for (size_t i = 0; i + 1 < s.size(); i += 2) {
		out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
	}
	return out;
}

int main(int argc, char **argv)
{
	if (argc != 2) {
		fprintf(stderr, "usage: %s vectors.txt\n", argv[0]);
		return 2;
	}
	FILE *f = fopen(argv[1], "r");
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	static char line[32768];
	int checked = 0, bad = 0;
	while (fgets(line, sizeof(line), f)) {
		std::vector<std::string> tok;
		for (char *t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) {
			tok.push_back(t);
		}
		if (tok.empty()) {
			continue;
		}
		uint8_t out[64];
		int dl = 0;
		std::vector<uint8_t> want;
		if (tok[0] == "H" && tok.size() == 4) {
			// heap copies of exactly the vector's size, so that the sanitizer sees every read past them
			const std::vector<uint8_t> msg = unhex(tok[2]);
			want = unhex(tok[3]);
			const int ht = atoi(tok[1].c_str());
			dl = s2_hash(ht, msg.data(), (uint32_t)msg.size(), out);
			if (ht == 11) {
				uint8_t o2[32];
				s2_sm3_streamed(msg.data(), (uint32_t)msg.size(), o2);
				bad += memcmp(o2, out, 32) != 0;
			}
		} else if (tok[0] == "Z" && tok.size() == 9) {
			const std::vector<uint8_t> id = unhex(tok[2]), a = unhex(tok[3]), b = unhex(tok[4]), gx = unhex(tok[5]), gy = unhex(tok[6]), key = unhex(tok[7]);
			want = unhex(tok[8]);
			dl = s2_sm2_z(atoi(tok[1].c_str()), id.empty() ? nullptr : id.data(), (uint32_t)id.size(), a.data(), b.data(), gx.data(), gy.data(),
				      (uint32_t)a.size(), key.data(), out, nullptr, nullptr);
		} else {
			fprintf(stderr, "bad line: %s\n", tok[0].c_str());
			return 2;
		}
		checked++;
		if (dl <= 0 || (size_t)dl != want.size() || memcmp(out, want.data(), (size_t)dl) != 0) {
			bad++;
		}
	}
	fclose(f);
	printf("checked %d bad %d\n", checked, bad);
	return bad ? 1 : (checked ? 0 : 3);
}
#endif
