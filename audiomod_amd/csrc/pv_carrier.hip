// pv_carrier.hip -- the generator kernel of the carrier setting (include/audiomod_pv.h "Carrier setting"): the channel
// vocoder's carrier of the stream pools' slots, written from pv_carrier.h's closed form.  One thread per sample; a
// launch serves a table of windows (one per carrier slot of a launch group).
#include <cstdint>

#include <hip/hip_runtime.h>

#include "pv_carrier.h"
#include "pv_kernels.h"

namespace pv {

// Sample i of job j: each voice's residue is (r + i) mod len in 32 bits (r < len <= 2^31 / 2 and i < 2^31: no wrap
// that matters -- the host refuses tables beyond kCarrierMaxFloats), the write lands inside the job's row whatever
// pos + i is (masked).
__global__ __launch_bounds__(kCarrierThreads) void pv_carrier_kernel(const CarrierArgs a) {
    const CarrierJob j = a.jobs[blockIdx.y];
    const uint32_t i = blockIdx.x * (uint32_t)kCarrierThreads + threadIdx.x;
    if ((int64_t)i >= (int64_t)j.n) return;
    uint32_t r0, r1 = 0, r2 = 0;
    if (j.chord) {
        r0 = (j.r[0] + i) % (uint32_t)a.len[1];
        r1 = (j.r[1] + i) % (uint32_t)a.len[2];
        r2 = (j.r[2] + i) % (uint32_t)a.len[3];
    } else {
        r0 = (j.r[0] + i) % (uint32_t)a.len[0];
    }
    a.out[j.out_off + (int64_t)((j.pos + i) & a.mask)] = carrier_sample(a.tab, a.off, j.chord, r0, r1, r2);
}

void launch_carrier(const CarrierArgs &a, int njobs, int max_n, hipStream_t st) {
    if (njobs <= 0 || max_n <= 0) return;
    hipLaunchKernelGGL(pv_carrier_kernel, dim3((max_n + kCarrierThreads - 1) / kCarrierThreads, njobs), dim3(kCarrierThreads),
                       0, st, a);
}

} // namespace pv
