// pv_wire.h -- the int16 wire of the device-side conversions (include/audiomod_pv.h PV_WIRE_I16): the reference's WAV
// reader and writer, one definition for every kernel that converts on load or on store (pv_hostio.hip's row kernels,
// pv_kernels.hip's pool ingest and egress).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

// main/wavfile.cc:733-755: float = (float)(int16 * (1.0 / 32768.0)) -- exact, so one float multiply gives the same
__device__ __forceinline__ float pv_wire_i16_to_f32(int16_t v) { return (float)v * (1.0f / 32768.0f); }
// main/wavfile.cc:1295-1306,1334-1342: (short)saturate(x * 32768.0f, -32768.0f, 32767.0f), truncation toward zero
__device__ __forceinline__ int16_t pv_wire_f32_to_i16(float x) {
    float v = x * 32768.0f;
    if (v > 32767.0f) v = 32767.0f;
    else if (v < -32768.0f) v = -32768.0f;
    return (int16_t)(int)v;
}
