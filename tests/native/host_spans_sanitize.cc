// tests/native/host_spans_sanitize.cc -- the span arithmetic of the batch engine (audiomod_amd/csrc/pv_plan.cc:
// batch_chunk_slices, batch_launches, batch_span) over a few hundred seeded random jobs under AddressSanitizer +
// UndefinedBehaviorSanitizer (CPU build, stand-alone), asserting the contract of include/audiomod_pv.h
// pv_batch_span_info for every division into spans of 1, 2, 3 and all launches.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
//            -Iinclude -Iaudiomod_amd/csrc tests/native/host_spans_sanitize.cc audiomod_amd/csrc/pv_plan.cc
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pv_plan.h"

using namespace pv;

static uint32_t g_seed = 12345u;
static uint32_t rnd() { // xorshift32
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 17;
    g_seed ^= g_seed << 5;
    return g_seed;
}
static int pick(int n) { return (int)(rnd() % (uint32_t)n); }

#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::printf("line %d: %s (fft %d hop %d frames %lld Tc %d span %d+%d)\n", __LINE__, #cond, d.N, d.hop, \
                        (long long)frames, Tc, first, n);                                 \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

// one division of the job's launches into spans of `per`
static int check_division(const Derived &d, const BatchPlan &bp, int64_t frames, int Tc, int per,
                          std::vector<pv_batch_span_info> *keep) {
    const int64_t L = batch_launches(bp, Tc), T = (int64_t)bp.slices.size();
    int64_t k = 0;
    pv_batch_span_info prev{};
    bool have_prev = false;
    for (int64_t f = 0; f < L; f += per) {
        const int first = (int)f, n = (int)(L - f < per ? L - f : per);
        pv_batch_span_info o;
        REQUIRE(batch_span(d, bp, frames, Tc, first, n, o) == PV_OK);
        REQUIRE(o.first_launch == first && o.launches == n);
        REQUIRE(o.slice_begin == f * Tc && o.slice_end == ((f + n) * Tc < T ? (f + n) * Tc : T));
        REQUIRE(o.out_begin == k && o.out_end >= k && o.out_end <= bp.out_frames);
        k = o.out_end;
        int64_t in_max, out_max; // a window sized from the constants alone holds every span of n launches
        batch_span_bounds(d, Tc, n, in_max, out_max);
        REQUIRE(o.in_end - o.in_begin <= in_max && o.out_end - o.out_begin <= out_max);
        REQUIRE(0 <= o.in_begin && o.in_begin <= o.in_end && o.in_end <= frames && (o.in_begin & 3) == 0);
        if (have_prev)
            REQUIRE(o.in_begin >= prev.in_begin && o.in_end >= prev.in_end && o.out_begin >= prev.out_begin &&
                    o.out_end >= prev.out_end);
        prev = o;
        have_prev = true;
        for (int64_t t = o.slice_begin; t < o.slice_end; ++t) {
            const int64_t a0 = t * d.hop;
            int64_t lo, hi;
            if (a0 + d.N + 4 <= frames) lo = a0 - (a0 & 3), hi = lo + d.N + 4; // the wave kernels' aligned pieces
            else lo = a0 < frames ? a0 : frames, hi = a0 + d.N < frames ? a0 + d.N : frames;
            if (hi > lo) REQUIRE(o.in_begin <= lo && hi <= o.in_end);
        }
        if (keep) keep->push_back(o);
    }
    const int first = 0, n = 0;
    REQUIRE(k == bp.out_frames);
    return 0;
}

static int check_job(const pv_config &cfg, int nstreams, int64_t frames, int block, bool flush, bool fast, int *ran) {
    Derived d;
    if (derive(cfg, d) != PV_OK) return 0;
    BatchPlan bp;
    if (plan_batch(d, frames, block, flush, bp) != PV_OK) return 0;
    const int Tc = batch_chunk_slices(cfg, nstreams, fast);
    int first = 0, n = 0;
    REQUIRE(Tc >= 4 && Tc <= 1024);
    const int64_t L = batch_launches(bp, Tc);
    ++*ran;
    pv_batch_span_info o;
    if (L == 0) {
        REQUIRE(batch_span(d, bp, frames, Tc, 0, 0, o) == PV_OK && o.launches == 0 && o.in_end == 0 && o.out_end == 0);
        REQUIRE(bp.out_frames == 0);
        REQUIRE(batch_span(d, bp, frames, Tc, 0, 1, o) == PV_ERR_INVALID_ARG);
        return 0;
    }
    REQUIRE(batch_span(d, bp, frames, Tc, 0, 0, o) == PV_ERR_INVALID_ARG);
    REQUIRE(batch_span(d, bp, frames, Tc, -1, 1, o) == PV_ERR_INVALID_ARG);
    REQUIRE(batch_span(d, bp, frames, Tc, (int32_t)L, 1, o) == PV_ERR_INVALID_ARG);
    REQUIRE(batch_span(d, bp, frames, Tc, 0, (int32_t)L + 1, o) == PV_ERR_INVALID_ARG);
    std::vector<pv_batch_span_info> one;
    if (check_division(d, bp, frames, Tc, 1, &one)) return 1;
    const int pers[] = {2, 3, (int)L};
    for (int per : pers) {
        std::vector<pv_batch_span_info> sp;
        if (check_division(d, bp, frames, Tc, per, &sp)) return 1;
        for (const pv_batch_span_info &s : sp) { // the hull of its parts; its out boundary is one of theirs
            const pv_batch_span_info &a = one[(size_t)s.first_launch], &b = one[(size_t)(s.first_launch + s.launches - 1)];
            first = s.first_launch, n = s.launches;
            REQUIRE(s.in_begin == a.in_begin && s.in_end == b.in_end && s.out_begin == a.out_begin && s.out_end == b.out_end);
            REQUIRE(s.slice_begin == a.slice_begin && s.slice_end == b.slice_end);
        }
    }
    return 0;
}

int main() {
    int bad = 0, n = 0, ran = 0;
    const int modes[] = {PV_MODE_CONSTANT, PV_MODE_NORMAL_SHIFT, PV_MODE_GENDER_CHANGE, PV_MODE_FORMANT_PRESERVE,
                         PV_MODE_VOCODER_ROSENBERG, PV_MODE_NORMAL_STRETCH, PV_MODE_ROBOTIC, PV_MODE_WHISPER};
    const int ffts[] = {128, 256, 512, 1000, 1024, 2048, 4096, 8192};
    const int rates[] = {44100, 48000, 96000};
    const char *knobs[] = {"4", "5", "8", "16", nullptr};
    for (int i = 0; i < 400; ++i) {
        const int mode = modes[pick(8)];
        const bool stretch = mode == PV_MODE_NORMAL_STRETCH;
        pv_config cfg{rates[pick(3)], 1 + pick(2), stretch ? 0.5f + (float)pick(2001) / 1000.f : 1.f,
                      stretch ? 0.f : -12.f + (float)pick(28001) / 1000.f, mode, pick(3), ffts[pick(8)],
                      pick(4) == 0 ? 64 + pick(400) : 0};
        const int64_t frames = 1 + pick(pick(4) == 0 ? 300 : 40000);
        const int block = 1 + pick(2000);
        const char *knob = knobs[pick(5)];
        if (knob) setenv("AUDIOMOD_PV_CHUNK_SLICES", knob, 1);
        else unsetenv("AUDIOMOD_PV_CHUNK_SLICES");
        bad += check_job(cfg, 1 + pick(300), frames, block, !stretch && pick(4) != 0, pick(2) != 0, &ran);
        ++n;
    }
    std::printf("%d jobs, %d planned, %d failures\n", n, ran, bad);
    return bad != 0 || ran < 200;
}
