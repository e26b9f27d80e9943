// Host build of libecc_amd/csrc/ecamd_detnonce.hip over tests/hipstub (g++, no HIP; compile with -D__shared__=static: the stand-in runs
// the lanes one after the other, and each lane owns its column of the word buffer): k_dbign_nonce<SCAN> and k_bip0340_nonce<ALG>
// themselves -- the lane's column, the slot check, the stores -- through their launchers, for tests/test_det_nonce_host.py.  Test
// infrastructure, not product code.
#include <hip/hip_runtime.h>
#include <string.h>
thread_local dim3 blockIdx, threadIdx;
#include "../libecc_amd/csrc/ecamd_detnonce.hip"

extern "C" int dk_dbign_batch(int scan, uint32_t n, const uint8_t *privs, const uint8_t *digests, uint32_t hlen, const uint8_t *oid, uint32_t oid_len,
			      const uint8_t *t, uint32_t t_len, const uint32_t *q, uint32_t qbits, uint8_t *nonces, uint8_t *status)
{
	EcamdDbignNonceArgs A;
	memset(&A, 0, sizeof(A));
	A.privs = privs;
	A.digests = digests;
	A.nonces = nonces;
	A.status = status;
	A.n = n;
	A.qbits = qbits;
	A.qlen = (qbits + 7) / 8;
	A.hlen = hlen;
	A.oid_len = oid_len;
	A.t_len = t_len;
	A.scan = scan;
	if (oid_len > 64 || t_len > 64) {
		return (int)hipErrorInvalidValue;
	}
	memcpy(A.oid, oid, oid_len);
	memcpy(A.t, t, t_len);
	for (int w = 0; w < 17; w++) {
		A.q[w] = q[w];
	}
	return (int)ecamd_launch_dbign_nonce(A, nullptr);
}

template <int ALG, typename KT> static void tags(EcamdBip0340NonceArgs &A, KT Kt)
{
	typename ecrfc::Alg<ALG>::W w[8];
	ecbip::tag_hash<ALG>("BIP0340/aux", 11, w, Kt);
	for (int t = 0; t < 8; t++) {
		A.tag_aux[t] = (uint64_t)w[t];
	}
	ecbip::tag_hash<ALG>("BIP0340/nonce", 13, w, Kt);
	for (int t = 0; t < 8; t++) {
		A.tag_nonce[t] = (uint64_t)w[t];
	}
}

extern "C" int dk_bip_batch(int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *keys, const uint8_t *kst, const uint8_t *aux,
			    const uint8_t *slots, uint32_t stride, uint32_t clen, const uint32_t *q, uint32_t qbits, uint8_t *nonces, uint8_t *status)
{
	EcamdBip0340NonceArgs A;
	memset(&A, 0, sizeof(A));
	A.privs = privs;
	A.keys = keys;
	A.kst = kst;
	A.aux = aux;
	A.slots = slots;
	A.nonces = nonces;
	A.status = status;
	A.n = n;
	A.qbits = qbits;
	A.qlen = (qbits + 7) / 8;
	A.clen = clen;
	A.stride = stride;
	for (int w = 0; w < 17; w++) {
		A.q[w] = q[w];
	}
	switch (hash_type) {
	case 1: tags<224>(A, (const uint32_t *)c_dn_k256); break;
	case 2: tags<256>(A, (const uint32_t *)c_dn_k256); break;
	case 3: tags<384>(A, (const uint64_t *)c_dn_k512); break;
	case 4: tags<512>(A, (const uint64_t *)c_dn_k512); break;
	default: break;
	}
	return (int)ecamd_launch_bip0340_nonce(hash_type, A, nullptr);
}
