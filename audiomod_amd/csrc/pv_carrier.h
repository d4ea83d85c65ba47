// pv_carrier.h -- the channel vocoder's carrier in closed form (include/audiomod_pv.h "Carrier setting").
//
// CarrierGen (pv_plan.cc) walks each voice's counter over 0 ... period inclusive and its step is a pure function of
// that counter, so sample n of a voice is table[n mod (period + 1)] with a table of period + 1 floats built once by
// CarrierGen's own arithmetic: float reciprocals, a double argument rounded to float, cosf.  The single voice's table
// already holds (float)(step * 0.3); the chord's three tables hold step / 3, and a chord sample is the float sum
// ((0 + a) + b) + c of its three entries times 0.3 in double -- the reference's order.  Nothing is generated
// sequentially, carried between calls or saved: a stream's carrier follows from its sample position alone.
//
// At sample rates where a voice's opening phase has zero length (n1 == 0, e.g. 16 kHz) entry 0 is 0 * inf = NaN, as
// the reference and CarrierGen produce it.
//
// The sample function is __host__ __device__: pv_plan_carrier and pv_carrier_kernel (pv_carrier.hip) share it.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef PV_HD
#define PV_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef PV_HD
#define PV_HD inline
#endif
#endif

namespace pv {

constexpr int kCarrierTabs = 4;        // the single voice's table, then the chord's three
constexpr int kCarrierThreads = 256;   // samples per workgroup of pv_carrier_kernel
constexpr int kCarrierMaxFloats = 1 << 16; // tables a feed's descriptor block carries at the most (all four together)

// The tables of one sample rate, one behind the other: [single | chord 0 | chord 1 | chord 2]; table i is len[i]
// floats from off[i] on.  len[i] = period + 1 of its voice.
struct CarrierTables {
    int32_t off[kCarrierTabs], len[kCarrierTabs];
    std::vector<float> v;
};

// one voice's period table (CarrierGen::init and CarrierGen::step): `chord` selects what the table holds
inline void carrier_voice_table(float sample_rate, float freq, bool chord, std::vector<float> &out) {
    const float alpha = 0.01f, beta = 0.06f;
    const int period = (int)std::round(1.f / freq * sample_rate);
    const int n1 = (int)std::round(alpha * period);
    const int n2 = (int)std::round(beta * period);
    const float inv_n1 = 1.f / static_cast<float>(n1);
    const float inv_2n2 = (float)(0.5 / static_cast<float>(n2));
    for (int n = 0; n <= period; ++n) {
        float s;
        if (n <= n1) s = (float)(0.5 * (1 - cosf((float)(M_PI * n * inv_n1))));
        else if (n - n1 <= n2) s = cosf((float)(M_PI * (n - n1) * inv_2n2));
        else s = 0;
        out.push_back(chord ? s / 3 : (float)(s * 0.3));
    }
}

inline void carrier_tables(int32_t sample_rate, CarrierTables &t) {
    static const float kTriad[3] = {440, 523.251f, 659.255f};
    t.v.clear();
    for (int i = 0; i < kCarrierTabs; ++i) {
        t.off[i] = (int32_t)t.v.size();
        carrier_voice_table((float)sample_rate, kTriad[i == 0 ? 0 : i - 1], i != 0, t.v);
        t.len[i] = (int32_t)t.v.size() - t.off[i];
    }
}

// One carrier sample from the tables: r[0] indexes the single voice's table (chord == 0), r[0 .. 2] the chord's three
// (chord != 0), each already reduced modulo its table's length.
PV_HD float carrier_sample(const float *tab, const int32_t *off, int chord, uint32_t r0, uint32_t r1, uint32_t r2) {
    if (!chord) return tab[off[0] + r0];
    float mix = 0;
    mix += tab[off[1] + r0];
    mix += tab[off[2] + r1];
    mix += tab[off[3] + r2];
    return (float)(mix * 0.3);
}

// One window of one stream for pv_carrier_kernel: samples [first, first + n) of the carrier go to
// out[out_off + ((pos + i) & mask)], i = 0 .. n - 1.  r[v]: `first` modulo the length of the voice's table, reduced on
// the host in 64 bits -- the device adds i (< 2^31) and reduces in 32.
struct CarrierJob {
    int64_t out_off;
    uint32_t pos;
    int32_t n;
    int32_t chord;
    uint32_t r[3];
};
static_assert(sizeof(CarrierJob) == 32, "CarrierJob has no implicit padding");

struct CarrierArgs {
    float *out;
    const float *tab;                // the tables of carrier_tables, in device memory
    int32_t off[kCarrierTabs], len[kCarrierTabs];
    uint32_t mask;                   // ring length - 1 (all ones: out is linear)
    const CarrierJob *jobs;
};

// the job of window [first, first + n) of carrier `chord` (first >= 0)
inline CarrierJob carrier_job(const CarrierTables &t, bool chord, int64_t first, int32_t n, int64_t out_off, uint32_t pos) {
    CarrierJob j{};
    j.out_off = out_off;
    j.pos = pos;
    j.n = n;
    j.chord = chord ? 1 : 0;
    for (int v = 0; v < 3; ++v) j.r[v] = chord ? (uint32_t)(first % t.len[v + 1]) : v == 0 ? (uint32_t)(first % t.len[0]) : 0u;
    return j;
}

} // namespace pv
