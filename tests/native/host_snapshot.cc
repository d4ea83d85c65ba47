// tests/native/host_snapshot.cc -- the GPU-free codec of a stream-pool snapshot (audiomod_amd/csrc/pv_snapshot.h)
// driven on the CPU: for a few hundred configurations a Planner and an overlap-add builder's live list run a random
// number of calls, their state goes through a blob into fresh objects, and original and copy continue side by side --
// every later SliceRec, available value and live list must be equal.  Then the validator: every proper prefix of a
// valid blob and several thousand single-byte and single-bit flips of it must be refused, from exactly sized heap
// copies, so that a read past the end shows under AddressSanitizer.
// With an argument: also writes one blob of known fields (zero device rows) to that file, for pv_pool_blob_info.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -Iinclude -Iaudiomod_amd/csrc tests/native/host_snapshot.cc
//            audiomod_amd/csrc/pv_plan.cc      (and the same with -O1 -g -fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

#include "pv_plan.h"
#include "pv_snapshot.h"

using namespace pv;

// the carried part of the engine's ChainBuilder: frames that may still cover samples not yet finalised
struct LiveList {
    std::deque<snap::LiveFrame> live;
    void add(const SliceRec &r, int N) {
        live.push_back(snap::LiveFrame{r.P, r.flags, 0});
        const int64_t Pn = r.P + r.adv;
        while (!live.empty() && live.front().P + N <= Pn) live.pop_front();
    }
    bool operator==(const LiveList &o) const {
        if (live.size() != o.live.size()) return false;
        for (size_t i = 0; i < live.size(); ++i)
            if (live[i].P != o.live[i].P || live[i].flags != o.live[i].flags) return false;
        return true;
    }
};

struct Stream {
    const Derived &d;
    Planner pl;
    LiveList ll;
    int64_t fed = 0, slices = 0;
    explicit Stream(const Derived &dd) : d(dd), pl(dd) {}
    // one transactional call, as pv_pool_feed makes it; returns the planner's status
    int call(int64_t n, int32_t take, std::vector<SliceRec> &out) {
        const Planner::State before = pl.save();
        out.clear();
        const int st = pl.feed(n, out);
        if (st != PV_OK) {
            pl.restore(before);
            out.clear();
            return st;
        }
        for (const SliceRec &r : out) ll.add(r, d.N);
        fed += n;
        slices += (int64_t)out.size();
        pl.retrieve(take < pl.available() ? take : pl.available());
        return st;
    }
};

static int phase_stage(const pv_config &c) {
    return c.mode == PV_MODE_ROBOTIC ? -1 : (c.coremode == 1 || c.coremode == 2) ? c.coremode : 0;
}

static snap::Header geometry(const pv_config &cfg, const Derived &d, int arith) {
    snap::Header h{};
    h.sample_rate = cfg.sample_rate, h.channels = cfg.channels;
    h.time_ratio = cfg.time_ratio, h.pitch_semitones = cfg.pitch_semitones;
    h.mode = cfg.mode, h.coremode = cfg.coremode, h.fftsize = cfg.fftsize, h.hopsize = cfg.hopsize;
    h.arith = arith;
    h.phase_stage = phase_stage(cfg);
    h.N = d.N, h.hs = d.hs;
    h.ring = 1024, h.TR = 3; // (any valid geometry serves the codec: small, so that the blobs stay small)
    h.HP = d.hs + 8;
    h.PKP = ((d.hs / 3 + 2) + 7) & ~7;
    h.AR = d.N + 4;
    h.stream_len = d.resample ? 2048 : 0;
    return h;
}

static std::vector<uint8_t> encode(const pv_config &cfg, const Derived &d, const Stream &s, std::mt19937 &rng, bool zero_rows) {
    snap::HostState hs;
    hs.plan = s.pl.save();
    hs.fed = s.fed, hs.uploaded = s.fed, hs.slices = s.slices;
    hs.acc_half = (int32_t)(s.slices & 1);
    hs.live.assign(s.ll.live.begin(), s.ll.live.end());
    const int64_t pending = s.pl.available();
    std::vector<std::vector<float>> pend((size_t)cfg.channels, std::vector<float>((size_t)pending));
    std::vector<const float *> pp;
    for (auto &v : pend) {
        for (float &x : v) x = (float)(rng() & 0xffff) / 65536.f;
        pp.push_back(v.data());
    }
    snap::Header h = geometry(cfg, d, (int)(rng() & 1));
    snap::fill_sizes(h, (int32_t)hs.live.size(), pending);
    std::vector<uint8_t> blob((size_t)h.total_bytes);
    snap::encode_head(h, hs, pp.data(), pending, blob.data());
    uint8_t *q = blob.data() + snap::payload_offset(h);
    for (int64_t i = 0; i < snap::device_bytes(h); ++i) q[i] = zero_rows ? 0 : (uint8_t)rng();
    snap::seal(blob.data(), h);
    return blob;
}

static int64_t draw_size(std::mt19937 &rng) {
    switch (rng() % 10) {
    case 0: return 0;
    case 1: return 1;
    case 2: return 13;
    case 3: return 479;
    case 4: return 4097;
    case 5: return 60000 + (int64_t)(rng() % 100000); // larger than the reference's output ring: slices are dropped
    default: return 200 + (int64_t)(rng() % 701);
    }
}

static int round_trip(const pv_config &cfg, std::mt19937 &rng) {
    Derived d;
    if (derive(cfg, d) != PV_OK) return 0;
    Stream a(d);
    std::vector<SliceRec> ra, rb;
    const int before = (int)(rng() % 13);
    for (int i = 0; i < before; ++i) a.call(draw_size(rng), (rng() % 4) ? INT32_MAX : (int32_t)(rng() % 300), ra);
    const std::vector<uint8_t> blob = encode(cfg, d, a, rng, false);
    snap::Header h;
    if (const char *why = snap::validate(blob.data(), (int64_t)blob.size(), &h)) {
        std::printf("a fresh blob is refused: %s\n", why);
        return 1;
    }
    snap::HostState hs;
    snap::decode_host(blob.data(), h, hs);
    Stream b(d);
    b.pl.restore(hs.plan);
    b.ll.live.assign(hs.live.begin(), hs.live.end());
    b.fed = hs.fed, b.slices = hs.slices;
    if (b.fed != a.fed || b.slices != a.slices || !(b.ll == a.ll) || b.pl.available() != a.pl.available() ||
        h.pending != a.pl.available() || hs.acc_half != (int32_t)(a.slices & 1) || h.time_ratio != cfg.time_ratio ||
        h.pitch_semitones != cfg.pitch_semitones) {
        std::printf("decoded state differs: mode %d fft %d\n", cfg.mode, cfg.fftsize);
        return 1;
    }
    for (int i = 0; i < 14; ++i) {
        const int64_t n = draw_size(rng);
        const int32_t take = (rng() % 4) ? INT32_MAX : (int32_t)(rng() % 300);
        const int sa = a.call(n, take, ra), sb = b.call(n, take, rb);
        bool same = sa == sb && ra.size() == rb.size() && a.pl.available() == b.pl.available() && a.ll == b.ll &&
                    a.pl.dropped() == b.pl.dropped() && a.pl.outputs() == b.pl.outputs();
        for (size_t k = 0; same && k < ra.size(); ++k)
            same = ra[k].shift == rb[k].shift && ra[k].phase_inc == rb[k].phase_inc && ra[k].P == rb[k].P &&
                   ra[k].K0 == rb[k].K0 && ra[k].cnt == rb[k].cnt && ra[k].adv == rb[k].adv && ra[k].flags == rb[k].flags;
        if (!same) {
            std::printf("continuation differs at call %d: mode %d core %d fft %d semis %g ratio %g\n", i, cfg.mode,
                        cfg.coremode, cfg.fftsize, cfg.pitch_semitones, cfg.time_ratio);
            return 1;
        }
    }
    return 0;
}

static bool refused(const std::vector<uint8_t> &b, size_t len) {
    // an exactly sized heap copy: a read past `len` is a heap overflow the sanitizer reports
    uint8_t *copy = static_cast<uint8_t *>(std::malloc(len ? len : 1));
    if (len) std::memcpy(copy, b.data(), len);
    snap::Header h;
    const bool r = snap::validate(copy, (int64_t)len, &h) != nullptr;
    std::free(copy);
    return r;
}

static int validator(std::mt19937 &rng) {
    const pv_config cfg{48000, 2, 1.f, 4.f, PV_MODE_NORMAL_SHIFT, 1, 512, 0};
    Derived d;
    if (derive(cfg, d) != PV_OK) return 1;
    Stream a(d);
    std::vector<SliceRec> r;
    for (int i = 0; i < 5; ++i) a.call(300 + 100 * i, i == 4 ? 50 : INT32_MAX, r);
    const std::vector<uint8_t> blob = encode(cfg, d, a, rng, false);
    int bad = 0;
    if (refused(blob, blob.size())) {
        std::printf("validator: the valid blob is refused\n");
        return 1;
    }
    for (size_t len = 0; len < blob.size(); ++len)
        if (!refused(blob, len)) {
            if (!bad) std::printf("validator: a prefix of %zu of %zu bytes is accepted\n", len, blob.size());
            ++bad;
        }
    if (snap::validate(nullptr, 100, nullptr) == nullptr || snap::validate(blob.data(), -5, nullptr) == nullptr) ++bad;
    std::vector<uint8_t> m = blob;
    for (int i = 0; i < 8000; ++i) {
        // half of them in the header and the host state, where every field matters on its own
        const size_t span = (i & 1) ? blob.size() : sizeof(snap::Header) + 64;
        const size_t at = rng() % span;
        const uint8_t x = (i & 2) ? (uint8_t)(1u << (rng() % 8)) : (uint8_t)(1 + rng() % 255);
        m[at] ^= x;
        if (!refused(m, m.size())) {
            if (!bad) std::printf("validator: byte %zu ^ %02x is accepted\n", at, x);
            ++bad;
        }
        m[at] ^= x;
    }
    return bad;
}

int main(int argc, char **argv) {
    std::mt19937 rng(20240607u);
    int bad = 0, n = 0;
    const int modes[] = {PV_MODE_NORMAL_SHIFT, PV_MODE_GENDER_CHANGE, PV_MODE_FORMANT_PRESERVE, PV_MODE_NORMAL_STRETCH,
                         PV_MODE_ROBOTIC};
    const float semis[] = {-12.f, -7.f, -3.5f, 4.f, 12.f};
    const float ratios[] = {0.8f, 1.2f, 1.5f, 2.f};
    const int ffts[] = {512, 1024, 2048, 4096};
    for (int mode : modes)
        for (int core = 0; core < 3; ++core)
            for (int fft : ffts)
                for (int k = 0; k < 5; ++k) {
                    if (mode == PV_MODE_ROBOTIC && (core != 1 || k > 1)) continue;
                    pv_config cfg{48000, 1 + (k & 1), 1.f, semis[k], mode, core, fft, 0};
                    if (mode == PV_MODE_NORMAL_STRETCH) cfg.pitch_semitones = 0.f, cfg.time_ratio = ratios[k % 4];
                    if (mode == PV_MODE_ROBOTIC) cfg.pitch_semitones = 0.f;
                    bad += round_trip(cfg, rng);
                    ++n;
                }
    // a mixed pool's slots: pitch and time ratio at once
    for (int k = 0; k < 40; ++k) {
        pv_config cfg{44100, 2, ratios[k % 4], semis[k % 5], PV_MODE_NORMAL_SHIFT, k % 3, ffts[k % 4], 0};
        bad += round_trip(cfg, rng);
        ++n;
    }
    bad += validator(rng);
    if (argc > 1) {
        const pv_config cfg{44100, 2, 1.25f, -3.5f, PV_MODE_NORMAL_SHIFT, 1, 1024, 0};
        Derived d;
        if (derive(cfg, d) != PV_OK) return 2;
        Stream a(d);
        std::vector<SliceRec> r;
        for (int i = 0; i < 6; ++i) a.call(700, i < 5 ? INT32_MAX : 0, r);
        const std::vector<uint8_t> blob = encode(cfg, d, a, rng, true);
        snap::Header h;
        if (snap::validate(blob.data(), (int64_t)blob.size(), &h)) return 2;
        FILE *f = std::fopen(argv[1], "wb");
        if (!f || std::fwrite(blob.data(), 1, blob.size(), f) != blob.size()) return 2;
        std::fclose(f);
        std::printf("blob: arith %d slices %lld pending %lld payload %lld total %lld\n", h.arith, (long long)h.slices,
                    (long long)h.pending, (long long)snap::device_bytes(h), (long long)h.total_bytes);
    }
    std::printf("%d configurations, %d failures\n", n, bad);
    return bad != 0;
}
