// Host build of libecc_amd/csrc/ecamd_rfc6979.hip over tests/hipstub (g++, no HIP; compile with -D__shared__=static: the stand-in runs
// the lanes one after the other, and each lane owns its column of the word buffer): k_rfc6979_nonce<ALG> itself -- the lane's column,
// the slot check, the stores -- through its launcher, for tests/test_rfc6979_host.py.  Test infrastructure, not product code.
#include <hip/hip_runtime.h>
thread_local dim3 blockIdx, threadIdx;
#include "../libecc_amd/csrc/ecamd_rfc6979.hip"

extern "C" int rk_nonce_batch(int hash_type, uint32_t n, const uint8_t *privs, const uint8_t *digests, const uint8_t *slots, uint32_t stride,
			      const uint32_t *q, uint32_t qbits, uint8_t *nonces, uint8_t *status)
{
	EcamdRfc6979Args A;
	A.privs = privs;
	A.digests = digests;
	A.slots = slots;
	A.stride = stride;
	A.nonces = nonces;
	A.status = status;
	A.n = n;
	A.qbits = qbits;
	A.qlen = (qbits + 7) / 8;
	for (int w = 0; w < 17; w++) {
		A.q[w] = q[w];
	}
	return (int)ecamd_launch_rfc6979_nonce(hash_type, A, nullptr);
}
