// host build of libecc_amd/csrc/ecamd_hash.hip for tests/test_belt_kernel_host.py (test infrastructure): k_belt_slots itself, launcher
// and length clamp included, run lane by lane through the stand-in runtime of tests/hipstub (which has no LDS: the kernel then reads
// the table where it lies)
#include <hip/hip_runtime.h>
#include <cstring>
thread_local dim3 blockIdx, threadIdx;
#include "../libecc_amd/csrc/ecamd_hash.hip"
extern "C" int belt_slots_host(const uint8_t *slots, uint32_t stride, uint32_t n, uint8_t *out, uint32_t out_stride)
{
	return (int)ecamd_launch_belt_slots(slots, stride, n, out, out_stride, nullptr);
}
