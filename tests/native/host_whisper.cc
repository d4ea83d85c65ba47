// tests/native/host_whisper.cc -- CPU check of the device generator's step (audiomod_amd/csrc/pv_whisper.h).
// Runs the __host__ __device__ code the way pv_whisper_kernel runs it -- a ring of kWhisperRing words, 64 emulated
// lanes per step, the state carried between launches as kWhisperHist full words -- and compares every word and every
// phase, bit for bit, with WhisperRng (which tests/test_host.py pins to libc rand()).
// Build: g++ -O2 -std=c++17 -ffp-contract=off -Iinclude -Iaudiomod_amd/csrc tests/native/host_whisper.cc \
//            audiomod_amd/csrc/pv_plan.cc -o /tmp/host_whisper
// The same file builds with -fsanitize=address,undefined (tests/test_voice_host.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pv_plan.h"
#include "pv_whisper.h"

using namespace pv;

// one launch, as the kernel does it: words[i], phases at whisper_out_index(i, per, pitch); state advanced in place
static void emulate_launch(uint32_t *state, int64_t count, int32_t per, int32_t pitch, std::vector<uint32_t> &words,
                           std::vector<float> &out) {
    if (count <= 0) return;
    std::vector<uint32_t> ring(kWhisperRing, 0xdeadbeefu);
    for (int i = 0; i < kWhisperHist; ++i) ring[(size_t)i] = state[i];
    const int64_t nsteps = (count + kWhisperLanes - 1) / kWhisperLanes;
    for (int64_t s = 0; s < nsteps; ++s) {
        uint32_t w[kWhisperLanes];
        // every lane reads before any lane writes, as lanes of one instruction do
        for (int lane = 0; lane < kWhisperLanes; ++lane) {
            const int64_t i = s * kWhisperLanes + lane;
            const uint32_t pos = (uint32_t)i + (uint32_t)kWhisperHist;
            w[lane] = whisper_word(ring.data(), pos);
            if (i < count) {
                const uint32_t x = ring[(size_t)((uint32_t)i & (uint32_t)(kWhisperRing - 1))];
                words.push_back(x);
                out[(size_t)whisper_out_index(i, per, pitch)] = whisper_phase(x);
            }
        }
        for (int lane = 0; lane < kWhisperLanes; ++lane) {
            const uint32_t pos = (uint32_t)(s * kWhisperLanes + lane) + (uint32_t)kWhisperHist;
            ring[(size_t)(pos & (uint32_t)(kWhisperRing - 1))] = w[lane];
        }
    }
    for (int i = 0; i < kWhisperHist; ++i) state[i] = ring[(size_t)((uint32_t)(count + i) & (uint32_t)(kWhisperRing - 1))];
}

static void fresh_state(uint32_t *state) {
    WhisperRng rng;
    for (int i = 0; i < kWhisperHist; ++i) state[i] = rng.next_word();
}

// `total` draws in launches of the given sizes (the last launch takes what is left), against WhisperRng
static int check_split(int64_t total, const std::vector<int64_t> &sizes, const char *label) {
    std::vector<uint32_t> want_w((size_t)total);
    std::vector<float> want_p((size_t)total);
    {
        WhisperRng a, b;
        for (int64_t i = 0; i < total; ++i) want_w[(size_t)i] = a.next_word();
        for (int64_t i = 0; i < total; ++i) want_p[(size_t)i] = b.next_phase();
    }
    uint32_t state[kWhisperHist];
    fresh_state(state);
    std::vector<uint32_t> words;
    std::vector<float> phases;
    int64_t done = 0;
    for (size_t k = 0; done < total; ++k) {
        int64_t n = k < sizes.size() ? sizes[k] : total - done;
        if (n > total - done) n = total - done;
        std::vector<float> out((size_t)n);
        emulate_launch(state, n, n > 0 ? (int32_t)n : 1, 0, words, out);
        phases.insert(phases.end(), out.begin(), out.end());
        done += n;
    }
    int bad = 0;
    if ((int64_t)words.size() != total || (int64_t)phases.size() != total) ++bad;
    for (int64_t i = 0; i < total && !bad; ++i) {
        if (words[(size_t)i] != want_w[(size_t)i]) ++bad;
        if (memcmp(&phases[(size_t)i], &want_p[(size_t)i], sizeof(float)) != 0) ++bad;
        if (bad) printf("%s: first difference at draw %lld\n", label, (long long)i);
    }
    // the state a launch leaves is the next kWhisperHist words of the stream
    {
        WhisperRng c;
        for (int64_t i = 0; i < total; ++i) (void)c.next_word();
        for (int i = 0; i < kWhisperHist && !bad; ++i)
            if (state[i] != c.next_word()) {
                printf("%s: state word %d differs\n", label, i);
                ++bad;
            }
    }
    return bad ? 1 : 0;
}

// the plane layout: draws of [slices][C][hs + 1] into rows of HP floats, untouched padding
static int check_layout() {
    const int slices = 3, C = 2, per = 257, HP = 264;
    const int64_t count = (int64_t)slices * C * per;
    uint32_t state[kWhisperHist];
    fresh_state(state);
    std::vector<uint32_t> words;
    std::vector<float> out((size_t)slices * C * HP, -1.f);
    emulate_launch(state, count, per, HP, words, out);
    WhisperRng rng;
    int bad = 0;
    for (int r = 0; r < slices * C; ++r)
        for (int k = 0; k < HP; ++k) {
            const float got = out[(size_t)r * HP + k];
            if (k < per) {
                const float want = rng.next_phase();
                if (memcmp(&got, &want, sizeof(float)) != 0) ++bad;
            } else if (got != -1.f) {
                ++bad;
            }
        }
    if (bad) printf("layout: %d differences\n", bad);
    return bad ? 1 : 0;
}

// the host's jump-ahead: the state D draws on, by the polynomial and chained, against WhisperRng run that far
static int check_jump() {
    int bad = 0;
    static const uint64_t jumps[] = {0, 1, 30, 31, 32, 682, 65600, 1000003};
    uint32_t fresh[kWhisperHist];
    fresh_state(fresh);
    for (uint64_t D : jumps) {
        uint32_t c[31], got[kWhisperHist];
        whisper_jump_poly(D, c);
        whisper_state_jump(fresh, c, got);
        WhisperRng rng;
        for (uint64_t i = 0; i < D; ++i) (void)rng.next_word();
        for (int i = 0; i < kWhisperHist; ++i)
            if (got[i] != rng.next_word()) {
                if (!bad) printf("jump %llu: word %d differs\n", (unsigned long long)D, i);
                ++bad;
            }
    }
    // chained, as the table's chunks are: three jumps of 65600 from the fresh state
    uint32_t c[31], a[kWhisperHist], b[kWhisperHist];
    whisper_jump_poly(65600, c);
    memcpy(a, fresh, sizeof a);
    for (int k = 0; k < 3; ++k) {
        whisper_state_jump(a, c, b);
        memcpy(a, b, sizeof a);
    }
    WhisperRng rng;
    for (int i = 0; i < 3 * 65600; ++i) (void)rng.next_word();
    for (int i = 0; i < kWhisperHist; ++i)
        if (a[i] != rng.next_word()) ++bad;
    if (bad) printf("jump: %d differences\n", bad);
    return bad ? 1 : 0;
}

int main() {
    int failures = 0, cases = 0;
    const int64_t total = 200000;
    ++cases, failures += check_split(total, {}, "one launch");
    static const int64_t cuts[] = {1, 63, 64, 65, 681, 682, 683, 2050, 4101};
    for (int64_t c : cuts) {
        char label[64];
        snprintf(label, sizeof label, "split at %lld", (long long)c);
        ++cases, failures += check_split(total, {c}, label);
    }
    ++cases, failures += check_split(total, {1, 63, 64, 65, 681, 682, 683, 2050, 4101, 0, 1}, "all cuts in a row");
    ++cases, failures += check_split(30000, std::vector<int64_t>(400, 75), "launches of 75");
    ++cases, failures += check_layout();
    ++cases, failures += check_jump();
    printf("host_whisper: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
