// pv_pcm.h -- the reference WAV reader's and writer's sample conversions (main/wavfile.cc:733-755 and :1295-1306,
// 1508-1527, as audiomod_pv_cli.cc WavIn::read / WavOut16::write state them), one definition for host and device:
// the mixed batch's PCM wire (pv_kernels.hip pv_mb_pcm_ingest_kernel / pv_mb_pcm_egress_kernel), the int16 wire
// (pv_wire.h) and the host test that sweeps them against the reader's double expressions (tests/native/host_pcm.cc).
// Compiles with a plain C++ compiler as well as with hipcc.
//
// The reader computes (float)(integer * 2^-k) (8 bit: minus one) in double.  For 8, 16 and 24 bits the integer, and so
// the product, is exact in float: an int-to-float conversion and a float multiply by the power of two give the same
// value.  For 32 bits the double product is exact and the cast rounds it to nearest even once; the int-to-float
// conversion rounds the integer the same way, and the power-of-two multiply that follows is exact (the smallest
// non-zero result, 2^-31, is a normal number).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PV_PCM_HD __host__ __device__ __forceinline__
#else
#define PV_PCM_HD inline
#endif

PV_PCM_HD float pv_pcm_u8_to_f32(uint8_t p) { return (float)((int32_t)p - 128) * (1.0f / 128.0f); }
PV_PCM_HD float pv_pcm_i16_to_f32(int16_t s) { return (float)s * (1.0f / 32768.0f); }
// s: the 24-bit sample, sign-extended
PV_PCM_HD float pv_pcm_i24_to_f32(int32_t s) { return (float)s * (1.0f / 8388608.0f); }
PV_PCM_HD float pv_pcm_i32_to_f32(int32_t s) { return (float)s * (1.0f / 2147483648.0f); }

// one little-endian sample of `bps` bytes (1 ... 4) at p
PV_PCM_HD float pv_pcm_load(const unsigned char *p, int bps) {
    if (bps == 1) return pv_pcm_u8_to_f32(p[0]);
    if (bps == 2) return pv_pcm_i16_to_f32((int16_t)(uint16_t)(p[0] | (p[1] << 8)));
    if (bps == 3) {
        uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        if (u & 0x00800000u) u |= 0xff000000u;
        return pv_pcm_i24_to_f32((int32_t)u);
    }
    return pv_pcm_i32_to_f32((int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)));
}

// the writer: (short)saturate(x * 32768.0f, -32768.0f, 32767.0f), truncation toward zero (NaN: not defined, as there)
PV_PCM_HD int16_t pv_pcm_f32_to_i16(float x) {
    float v = x * 32768.0f;
    if (v > 32767.0f) v = 32767.0f;
    else if (v < -32768.0f) v = -32768.0f;
    return (int16_t)(int)v;
}
