// host_pcm.cc -- pv_pcm.h (the conversions the mixed batch's PCM kernels use) against the WAV reader's and writer's own
// expressions as audiomod_pv_cli.cc states them, in double where the reader computes in double:
//   8, 16, 24 bits: every value;
//   32 bits: every value within 4 of a multiple of 2^k for k = 7 ... 31, both signs, the extremes, 2^26 random values;
//   writer: k / 32768 for k = -32769 ... 32768 with both float neighbours, +-0, denormals, +-1.5, +-3e38, +-inf.
// NaN is left out: the writer's cast of it is not defined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "pv_pcm.h"

static uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static unsigned long long checked = 0, bad = 0;
static void same(float got, float want, const char *what, long long v) {
    ++checked;
    if (bits_of(got) != bits_of(want)) {
        if (bad++ < 10) printf("MISMATCH %s %lld: %a vs %a\n", what, v, (double)got, (double)want);
    }
}

// the reader's expressions (WavIn::read)
static float ref_u8(uint8_t p) { return (float)(p * (1.0 / 128.0) - 1.0); }
static float ref_i16(int16_t s) { return (float)(s * (1.0 / 32768.0)); }
static float ref_i24(int32_t s) { return (float)(s * (1.0 / 8388608.0)); }
static float ref_i32(int32_t s) { return (float)(s * (1.0 / 2147483648.0)); }
// the writer's (WavOut16::write)
static int16_t ref_out(float x) {
    float v = x * 32768.0f;
    if (v > 32767.0f) v = 32767.0f;
    else if (v < -32768.0f) v = -32768.0f;
    return (int16_t)(int)v;
}

static void check32(int64_t v) {
    if (v < INT32_MIN || v > INT32_MAX) return;
    const int32_t s = (int32_t)v;
    same(pv_pcm_i32_to_f32(s), ref_i32(s), "i32", v);
    const uint32_t u = (uint32_t)s;
    const unsigned char le[4] = {(unsigned char)u, (unsigned char)(u >> 8), (unsigned char)(u >> 16), (unsigned char)(u >> 24)};
    same(pv_pcm_load(le, 4), ref_i32(s), "i32 bytes", v);
}
static void check_out(float x) {
    ++checked;
    if (pv_pcm_f32_to_i16(x) != ref_out(x)) {
        if (bad++ < 10) printf("MISMATCH out %a: %d vs %d\n", (double)x, pv_pcm_f32_to_i16(x), ref_out(x));
    }
}

int main() {
    for (int p = 0; p < 256; ++p) {
        const unsigned char b = (unsigned char)p;
        same(pv_pcm_u8_to_f32(b), ref_u8(b), "u8", p);
        same(pv_pcm_load(&b, 1), ref_u8(b), "u8 bytes", p);
    }
    for (int s = -32768; s <= 32767; ++s) {
        const unsigned char le[2] = {(unsigned char)(s & 255), (unsigned char)((s >> 8) & 255)};
        same(pv_pcm_i16_to_f32((int16_t)s), ref_i16((int16_t)s), "i16", s);
        same(pv_pcm_load(le, 2), ref_i16((int16_t)s), "i16 bytes", s);
    }
    for (int s = -8388608; s <= 8388607; ++s) {
        const unsigned char le[3] = {(unsigned char)(s & 255), (unsigned char)((s >> 8) & 255), (unsigned char)((s >> 16) & 255)};
        same(pv_pcm_i24_to_f32(s), ref_i24(s), "i24", s);
        same(pv_pcm_load(le, 3), ref_i24(s), "i24 bytes", s);
    }
    for (int k = 7; k <= 31; ++k)
        for (int64_t m = (int64_t)1 << k; m <= ((int64_t)1 << 31); m += (int64_t)1 << k)
            for (int d = -4; d <= 4; ++d) check32(m + d), check32(-m + d);
    for (int d = -4; d <= 4; ++d) check32(d);
    check32(INT32_MIN), check32(INT32_MIN + 1), check32(INT32_MAX), check32(INT32_MAX - 1);
    uint64_t x = 0x9E3779B97F4A7C15ull; // xorshift64*, seeded
    for (int i = 0; i < (1 << 26); ++i) {
        x ^= x >> 12, x ^= x << 25, x ^= x >> 27;
        check32((int32_t)(uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 32));
    }
    for (int k = -32769; k <= 32768; ++k) {
        const float f = (float)k / 32768.0f;
        check_out(f);
        check_out(std::nextafterf(f, INFINITY));
        check_out(std::nextafterf(f, -INFINITY));
    }
    const float inf = std::numeric_limits<float>::infinity(), den = std::numeric_limits<float>::denorm_min();
    const float specials[] = {0.0f, -0.0f, den, -den, 1e-40f, -1e-40f, 1.17549421e-38f, -1.17549421e-38f,
                              1.5f, -1.5f, 3e38f, -3e38f, inf, -inf};
    for (float f : specials) check_out(f);
    printf("%llu values checked, %llu mismatches\n", checked, bad);
    return bad ? 1 : 0;
}
