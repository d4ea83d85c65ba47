// pv_whisper.h -- the WHISPER voice's random phases, drawn on the device: glibc's rand() made parallel over a wave.
//
// rand() (TYPE_3) is the additive feedback generator x[i] = x[i-3] + x[i-31] (mod 2^32) with output x >> 1
// (pv_plan.cc WhisperRng: seeding and warm-up).  With E the shift operator the recurrence reads E^31 = E^28 + 1, and
// since the two terms commute, E^(31k) = (E^28 + 1)^k = sum_j C(k, j) E^(28j):
//     x[m] = sum_{j = 0..k} C(k, j) * x[m - 31k + 28j]   (mod 2^32),
// whose nearest term is x[m - 3k].  With k = 22 the nearest lag is 66, so the 64 lanes of a wave produce 64
// consecutive words from words that all exist already: 23 integer multiply-adds per word (largest coefficient
// C(22, 11) = 705432) over a history of 31 * 22 = 682 full 32-bit words.
//
// State of a stream: the NEXT kWhisperHist words it will draw, x[m .. m + 682), as full words -- a fixed 2728 bytes
// whatever the stream's age.  A launch loads them into a ring of kWhisperRing words, and each step s
//   - turns words [64 s, 64 s + 64) of the launch into phases (they are in the ring: state, or made by earlier steps),
//   - makes words [682 + 64 s, 682 + 64 s + 64) from the ring (whisper_word) and adds them to it;
// after ceil(count / 64) steps the ring holds words [count, count + 682): the state the launch leaves.
//
// The functions are __host__ __device__ so that tests/native/host_whisper.cc runs the same step on the CPU, lane by
// lane, against WhisperRng (which tests/test_host.py pins to libc rand()).
#pragma once

#include <cstdint>

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

constexpr int kWhisperK = 22;                // power of the recurrence a step applies
constexpr int kWhisperHist = 31 * kWhisperK; // 682: words of state, and the farthest lag of a step
constexpr int kWhisperLanes = 64;            // words per step (<= 3 * kWhisperK = 66, the nearest lag)
constexpr int kWhisperRing = 1024;           // ring of words a launch works in (power of two)
constexpr int kWhisperStatePitch = 684;      // words between state rows in device memory (16-byte multiple)
static_assert(kWhisperLanes <= 3 * kWhisperK, "a step may only read words that exist");
// a step reads words [64 s, 64 s + 680) and writes [64 s + 682, 64 s + 746): distinct ring entries, and the words
// [count, count + 682) of the final state are all among the newest 746
static_assert(kWhisperHist + kWhisperLanes <= kWhisperRing, "the ring holds a step's reads and writes side by side");

struct WhisperCoeff { // C(22, j)
    static constexpr uint32_t c[kWhisperK + 1] = {1,      22,     231,    1540,   7315,   26334,  74613,  170544,
                                                  319770, 497420, 646646, 705432, 646646, 497420, 319770, 170544,
                                                  74613,  26334,  7315,   1540,   231,    22,     1};
};

// word `pos` of the launch (pos >= kWhisperHist) from the ring, word i of the launch living at ring[i % kWhisperRing]
PV_HD uint32_t whisper_word(const uint32_t *ring, uint32_t pos) {
    uint32_t acc = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j <= kWhisperK; ++j)
        acc += WhisperCoeff::c[j] * ring[(pos - (uint32_t)kWhisperHist + 28u * (uint32_t)j) & (uint32_t)(kWhisperRing - 1)];
    return acc;
}

// whisperSlice's phase of a draw: two_pi * (float)rand() / (float)RAND_MAX, one float product and one float quotient
// ((float)RAND_MAX is 2^31, so the quotient is exact whichever way it is formed)
PV_HD float whisper_phase(uint32_t word) {
    const float two_pi = (float)(2 * 3.14159265358979323846);
    const float num = two_pi * (float)(word >> 1);
    return num / (float)2147483647;
}

// where draw i of a launch goes: draws come slice-major, channel, bin 0 .. hs (`per` = hs + 1 of them), rows of the
// phase table are `pitch` floats apart
PV_HD int64_t whisper_out_index(int64_t i, int32_t per, int32_t pitch) { return (i / per) * pitch + i % per; }

// one generator launch of one stream (pv_whisper_kernel): word offsets into the state buffer, float offset into the
// phase buffer.  src_off != dst_off: the stream starts here, from the pool's constant fresh state
struct WhisperJob {
    int64_t src_off, dst_off; // state row read, state row written (dst_off < 0: the state the launch leaves is dropped)
    int64_t out_off;          // first phase of the launch
    int64_t count;            // draws (0: nothing is read or written)
    int32_t per, pitch;       // whisper_out_index
};

// Jump-ahead on the host, for a long table drawn by many waves at once (the mixed batch's): the state D draws on.
// With f(x) = x^31 - x^28 - 1 the recurrence's characteristic polynomial, x^D = sum_i c[i] x^i (mod f, coefficients
// mod 2^32) gives x[n + D] = sum_{i < 31} c[i] * x[n + i] for every n -- the ring Z / 2^32 is commutative, which is
// all the identity needs.
inline void whisper_poly_mulmod(const uint32_t *a, const uint32_t *b, uint32_t *out) {
    uint32_t prod[61] = {0};
    for (int i = 0; i < 31; ++i)
        for (int j = 0; j < 31; ++j) prod[i + j] += a[i] * b[j];
    for (int d = 60; d >= 31; --d) { // x^d = x^(d - 31) * (x^28 + 1)
        prod[d - 3] += prod[d];
        prod[d - 31] += prod[d];
    }
    for (int i = 0; i < 31; ++i) out[i] = prod[i];
}
inline void whisper_jump_poly(uint64_t D, uint32_t c[31]) {
    uint32_t base[31] = {0}, acc[31] = {0}, t[31];
    base[1] = 1, acc[0] = 1;
    for (; D; D >>= 1) {
        if (D & 1) {
            whisper_poly_mulmod(acc, base, t);
            for (int i = 0; i < 31; ++i) acc[i] = t[i];
        }
        whisper_poly_mulmod(base, base, t);
        for (int i = 0; i < 31; ++i) base[i] = t[i];
    }
    for (int i = 0; i < 31; ++i) c[i] = acc[i];
}
// the state kWhisperHist words x[m + D ..] from the state x[m ..] (both kWhisperHist words; they may not overlap)
inline void whisper_state_jump(const uint32_t *state, const uint32_t c[31], uint32_t *next) {
    for (int t = 0; t < 31; ++t) {
        uint32_t acc = 0;
        for (int i = 0; i < 31; ++i) acc += c[i] * state[t + i];
        next[t] = acc;
    }
    for (int t = 31; t < kWhisperHist; ++t) next[t] = next[t - 3] + next[t - 31];
}

} // namespace pv
