// pv_whisper.hip -- the generator kernel of the voice setting (include/audiomod_pv.h "Voice setting"): the WHISPER
// phases of the slot-table paths, drawn on the device by pv_whisper.h's step.  One wave per job (= per whisper slot
// of a launch group); the ring of words lives in LDS.
#include <cstdint>

#include <hip/hip_runtime.h>

#include "pv_kernels.h"
#include "pv_whisper.h"

namespace pv {

// Single wave per workgroup: the barriers order a step's LDS writes before the next step's reads (and tell the
// compiler so); they cost one s_barrier each, against 23 LDS reads and multiply-adds.
__global__ __launch_bounds__(kWhisperLanes) void pv_whisper_kernel(uint32_t *__restrict__ state, float *__restrict__ out,
                                                                   const WhisperJob *__restrict__ jobs) {
    __shared__ uint32_t ring[kWhisperRing];
    const WhisperJob j = jobs[blockIdx.x];
    if (j.count <= 0) return; // (workgroup-uniform)
    const int lane = (int)threadIdx.x;
    for (int i = lane; i < kWhisperHist; i += kWhisperLanes) ring[i] = state[j.src_off + i];
    __syncthreads();
    // draw i = 64 s + lane of the launch goes to row q = i / per, column r = i % per
    int64_t q = lane / j.per;
    int32_t r = lane % j.per;
    const int64_t nsteps = (j.count + kWhisperLanes - 1) / kWhisperLanes;
    for (int64_t s = 0; s < nsteps; ++s) {
        const int64_t i = s * kWhisperLanes + lane;
        const uint32_t pos = (uint32_t)i + (uint32_t)kWhisperHist; // (mod 2^32: only pos mod kWhisperRing is used)
        const uint32_t w = whisper_word(ring, pos);
        if (i < j.count) out[j.out_off + q * j.pitch + r] = whisper_phase(ring[(uint32_t)i & (uint32_t)(kWhisperRing - 1)]);
        ring[pos & (uint32_t)(kWhisperRing - 1)] = w;
        __syncthreads();
        r += kWhisperLanes;
        while (r >= j.per) r -= j.per, ++q;
    }
    // what the launch leaves: words [count, count + kWhisperHist)
    if (j.dst_off < 0) return;
    for (int i = lane; i < kWhisperHist; i += kWhisperLanes)
        state[j.dst_off + i] = ring[(uint32_t)(j.count + i) & (uint32_t)(kWhisperRing - 1)];
}

void launch_whisper(uint32_t *state, float *out, const WhisperJob *jobs, int njobs, int census_set, int nc, hipStream_t st) {
    if (njobs <= 0) return;
    census_voice(census_set, nc);
    hipLaunchKernelGGL(pv_whisper_kernel, dim3(njobs), dim3(kWhisperLanes), 0, st, state, out, jobs);
}

} // namespace pv
