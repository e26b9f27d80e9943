// tests/hash_table_host_shim.cpp -- libecc_amd/csrc/ecamd_keccak.h, ecamd_sha512t.h, ecamd_rmd160.h and ecamd_bash.h compiled for the
// host (g++, no HIP), so that tests/test_hash_table_host.py can run the per-item code of k_sha3_slots, k_sha512t_slots, k_rmd160_slots
// and k_bash_slots against the recorded reference answers and hashlib without a GPU.  Built twice: as a shared library for ctypes, and
// with -DHASH_TABLE_MAIN as a stand-alone program (its own main, for -fsanitize=address,undefined) that reads vectors from a text file:
//     H <hash_type> <stride> <length field> <message hex or -> <digest hex>
// The slot of a vector is a heap array of exactly `stride` octets: the length field, the message, zeros.  A length field larger than
// stride - 4 is a slot that does not fit; its digest is all zeros.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../libecc_amd/csrc/ecamd_keccak.h"
#include "../libecc_amd/csrc/ecamd_sha512t.h"
#include "../libecc_amd/csrc/ecamd_rmd160.h"
#include "../libecc_amd/csrc/ecamd_bash.h"

static const uint64_t k_keccak_rc[24] = {ECAMD_KECCAK_RC};
static const uint64_t k_bash_rc[24] = {ECAMD_BASH_RC};
static const uint64_t k_512[80] = {ECAMD_SHA512_K};

extern "C" {

// digest octets of hash_type (5 .. 10, 15, 17 .. 20), 0 for another; block: the block / rate in octets
int ht_sizes(int hash_type, int *block)
{
	const int hs[4] = {eckk::hash_size(hash_type), ecs5t::hash_size(hash_type), ecrmd::hash_size(hash_type), ecbash::hash_size(hash_type)};
	const int bs[4] = {eckk::block_size(hash_type), ecs5t::block_size(hash_type), ecrmd::block_size(hash_type), ecbash::block_size(hash_type)};
	for (int k = 0; k < 4; k++) {
		if (hs[k]) {
			if (block) {
				*block = bs[k];
			}
			return hs[k];
		}
	}
	return 0;
}

// one slot of `stride` octets (a multiple of 4, aligned to 4) as the kernels digest it.  Returns the digest length, 0 for another hash_type.
int ht_slot(int hash_type, const uint8_t *slot, uint32_t stride, uint8_t *out)
{
	switch (hash_type) {
	case 5: eckk::slot_digest<28>(k_keccak_rc, slot, stride, out); break;
	case 6: eckk::slot_digest<32>(k_keccak_rc, slot, stride, out); break;
	case 7: eckk::slot_digest<48>(k_keccak_rc, slot, stride, out); break;
	case 8: eckk::slot_digest<64>(k_keccak_rc, slot, stride, out); break;
	case 9: ecs5t::slot_digest<224>(k_512, slot, stride, out); break;
	case 10: ecs5t::slot_digest<256>(k_512, slot, stride, out); break;
	case 15: ecrmd::slot_digest(slot, stride, out); break;
	case 17: ecbash::slot_digest<224>(k_bash_rc, slot, stride, out); break;
	case 18: ecbash::slot_digest<256>(k_bash_rc, slot, stride, out); break;
	case 19: ecbash::slot_digest<384>(k_bash_rc, slot, stride, out); break;
	case 20: ecbash::slot_digest<512>(k_bash_rc, slot, stride, out); break;
	default: return 0;
	}
	return ht_sizes(hash_type, nullptr);
}

// the message in the smallest slot that holds it
int ht_hash(int hash_type, const uint8_t *msg, uint32_t len, uint8_t *out)
{
	const uint32_t stride = (4u + len + 3u) & ~3u;
	std::vector<uint32_t> slot(stride / 4u, 0);
	slot[0] = len;
	if (len) {
		memcpy(slot.data() + 1, msg, len);
	}
	return ht_slot(hash_type, (const uint8_t *)slot.data(), stride, out);
}

// round constant t of bash-f as the unit holds it
uint64_t ht_bash_rc(uint32_t t) { return k_bash_rc[t % 24u]; }

}  // extern "C"

#ifdef HASH_TABLE_MAIN
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
		if (tok[0] != "H" || tok.size() != 6) {
			fprintf(stderr, "bad line: %s\n", tok[0].c_str());
			return 2;
		}
		const int ht = atoi(tok[1].c_str());
		const uint32_t stride = (uint32_t)strtoul(tok[2].c_str(), nullptr, 10), field = (uint32_t)strtoul(tok[3].c_str(), nullptr, 10);
		const std::vector<uint8_t> msg = unhex(tok[4]), want = unhex(tok[5]);
		if (stride < 4 || (stride & 3u) || msg.size() > stride - 4) {
			fprintf(stderr, "bad vector\n");
			return 2;
		}
		// a heap slot of exactly the stride, so that the sanitizer sees every read past it
		uint32_t *slot = (uint32_t *)calloc(stride / 4u, 4);
		slot[0] = field;
		if (!msg.empty()) {
			memcpy(slot + 1, msg.data(), msg.size());
		}
		uint8_t out[64];
		const int dl = ht_slot(ht, (const uint8_t *)slot, stride, out);
		free(slot);
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
