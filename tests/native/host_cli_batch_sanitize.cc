// host_cli_batch_sanitize.cc -- pv_cli_batch.h (manifest parser, WAV reader and writer, grouping and sub-batch
// arithmetic of audiomod-pv-exe batch) on hostile input, built with -fsanitize=address,undefined.  argv[1]: a
// directory to write the WAV files into.  Prints "<n> checks, <m> failures".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pv_cli_batch.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        ++checks;                                                    \
        if (!(cond)) ++failures, printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    } while (0)

using namespace pvcli;

static bool parse(const std::string &text, bool amount, std::vector<ManifestJob> &jobs, int &line) {
    std::string err;
    line = -1;
    const bool ok = parse_manifest(text, amount, jobs, line, err);
    CHECK(ok ? !jobs.empty() : (jobs.empty() && !err.empty()));
    return ok;
}

static void manifests() {
    std::vector<ManifestJob> j;
    int line;
    CHECK(parse("a.wav\tb.wav\n", true, j, line) && j.size() == 1 && j[0].in == "a.wav" && j[0].out == "b.wav" && !j[0].has_amount);
    CHECK(parse("# c\n\n  \nmy in.wav\tmy out.wav\t-3.5\r\nc.wav\td.wav", true, j, line) && j.size() == 2 &&
          j[0].in == "my in.wav" && j[0].has_amount && j[0].amount == -3.5 && j[0].line == 4 && j[1].line == 5);
    CHECK(!parse("", true, j, line) && line == 0);
    CHECK(!parse("# only a comment\n\n", true, j, line) && line == 0);
    CHECK(!parse("a.wav b.wav\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\n\nc.wav\n", true, j, line) && line == 3);
    CHECK(!parse("a.wav\tb.wav\t1\t2\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\t\n", true, j, line) && line == 1);
    CHECK(!parse("\tb.wav\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\tx\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\t1.5x\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\t\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\tnan\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\tinf\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\t1e300\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\t2\n", false, j, line) && line == 1);
    CHECK(!parse("a.wav\tb.wav\nc.wav\tb.wav\n", true, j, line) && line == 2);
    CHECK(!parse("a.wav\tb.wav\nb.wav\tc.wav\n", true, j, line) && line == 1);
    CHECK(!parse("a.wav\ta.wav\n", true, j, line) && line == 1);
    CHECK(!parse(std::string("a.wav\tb\0.wav\n", 13), true, j, line) && line == 1);
    std::string big;
    for (int i = 0; i < 3000; ++i) big += "in" + std::to_string(i) + ".wav\tout" + std::to_string(i) + ".wav\t0.25\n";
    CHECK(parse(big, true, j, line) && j.size() == 3000);
    std::string noise; // bytes of every value, tabs and newlines included
    uint32_t x = 12345;
    for (int i = 0; i < 20000; ++i) x = x * 1664525u + 1013904223u, noise.push_back((char)(x >> 24));
    (void)parse(noise, true, j, line);
    (void)parse(std::string(5000, '\t'), true, j, line);
    (void)parse(std::string(5000, '\n'), true, j, line);
}

// tests/test_cli_wav.py's hostile headers, restated
static std::string wav(uint32_t fmt_len = 16, bool pad_fmt = false, int block_align = -1, int64_t claim_data = -1,
                       size_t samples = 4000, int ch = 2, int bits = 16, uint32_t rate = 48000) {
    auto le = [](uint32_t v, int n) {
        std::string s;
        for (int i = 0; i < n; ++i) s.push_back((char)((v >> (8 * i)) & 255));
        return s;
    };
    const int ba = block_align >= 0 ? block_align : ch * bits / 8;
    std::string fmt = le(1, 2) + le((uint32_t)ch, 2) + le(rate, 4) + le(rate * (uint32_t)ba, 4) + le((uint32_t)ba, 2) + le((uint32_t)bits, 2);
    fmt += std::string(fmt_len > 16 && fmt_len < 100 ? fmt_len - 16 : 0, '\0');
    std::string body = "WAVEfmt " + le(fmt_len, 4) + fmt + (pad_fmt ? std::string(1, '\0') : std::string());
    body += "data" + le(claim_data >= 0 ? (uint32_t)claim_data : (uint32_t)samples, 4) + std::string(samples, '\1');
    return "RIFF" + le((uint32_t)body.size(), 4) + body;
}

static std::string dir;
static int open_wav(const std::string &blob, bool load, long *frames = nullptr, int *bits = nullptr) {
    const std::string path = dir + "/hostile.wav";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return -1;
    fwrite(blob.data(), 1, blob.size(), f);
    fclose(f);
    try {
        WavIn w(path.c_str(), load);
        if (frames) *frames = w.frames;
        if (bits) *bits = w.bits;
        if (load) {
            std::vector<std::vector<float>> rows(w.channels, std::vector<float>(64));
            std::vector<float *> p;
            for (auto &r : rows) p.push_back(r.data());
            long got = 0;
            for (int n; (n = w.read(p.data(), 64)) > 0;) got += n;
            CHECK(got == w.frames);
        }
        return 1;
    } catch (const std::exception &) {
        return 0;
    }
}

static void wavs() {
    long fa = -1, fb = -1;
    for (int load = 0; load < 2; ++load) {
        CHECK(open_wav(wav(), load, load ? &fa : &fb) == 1);
        CHECK(open_wav(wav(17, true), load) == 1);                       // odd fmt chunk with its pad byte
        long fr = -1;
        CHECK(open_wav(wav(16, false, -1, 0xFFFFFFF0ll), load, &fr) == 1 && fr == 1000); // data length claims 4 GB
        CHECK(open_wav(wav(16, false, 3), load) == 0);                   // block align contradicts channels * bits
        std::string g = wav();
        g[16] = 0, g[17] = 0, g[18] = 0, g[19] = 0x40;                   // fmt chunk claims 1 GB
        CHECK(open_wav(g, load) == 0);
        CHECK(open_wav(wav().substr(0, 30), load) == 0);                 // truncated inside the format chunk
        CHECK(open_wav(wav().substr(0, 44 + 6), load, &fr) == 1 && fr == 1); // truncated inside the samples
        CHECK(open_wav(wav().substr(0, 44), load, &fr) == 1 && fr == 0);
        CHECK(open_wav("RIFF", load) == 0);
        CHECK(open_wav("", load) == 0);
        CHECK(open_wav(wav(16, false, -1, -1, 4000, 0), load) == 0);     // no channels
        CHECK(open_wav(wav(16, false, -1, -1, 4000, 2, 12), load) == 0); // 12 bits
        CHECK(open_wav(wav(16, false, -1, -1, 4000, 65535, 32, 0xFFFFFFFFu), load) == 0); // block align does not fit 16 bits
        CHECK(open_wav(wav(16, false, -1, -1, 4001, 3, 24, 0x80000000u), load, &fr) == 1 && fr == 444);
        CHECK(open_wav(wav(16, false, -1, -1, 999, 1, 8), load, &fr) == 1 && fr == 999);
        CHECK(open_wav(wav(16, false, -1, -1, 4000, 2, 32), load, &fr) == 1 && fr == 500);
        std::string junk = wav();
        junk.insert(12, std::string("LIST\x03\x00\x00\x00" "abc\0", 12)); // an odd chunk before fmt, with its pad byte
        CHECK(open_wav(junk, load, &fr) == 1 && fr == 1000);
        std::string far = wav();
        far.insert(12, std::string("LIST\xff\xff\xff\x7f", 8));          // a chunk that claims to reach past the file
        CHECK(open_wav(far, load) == 0);
    }
    CHECK(fa == 1000 && fb == 1000);
    // the writer: both entries give the same file
    const std::string pa = dir + "/a.wav", pb = dir + "/b.wav";
    {
        float l[5] = {0.f, 0.5f, -0.5f, 2.f, -2.f}, r[5] = {1e-9f, -1e-9f, 0.25f, 0.99999f, -1.f};
        float *rows[2] = {l, r};
        int16_t pcm[10];
        for (int i = 0; i < 5; ++i)
            for (int c = 0; c < 2; ++c) {
                float v = rows[c][i] * 32768.0f;
                v = v > 32767.0f ? 32767.0f : v < -32768.0f ? -32768.0f : v;
                pcm[2 * i + c] = (int16_t)(int)v;
            }
        WavOut16 a(pa.c_str(), 44100, 2), b(pb.c_str(), 44100, 2);
        a.write(rows, 5);
        b.write_pcm16(pcm, 5);
    }
    auto slurp = [](const std::string &p) {
        std::string s;
        if (FILE *f = fopen(p.c_str(), "rb")) {
            char buf[256];
            for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
            fclose(f);
        }
        return s;
    };
    CHECK(slurp(pa).size() == 56 + 20 && slurp(pa) == slurp(pb));
    long fr = -1;
    int bits = 0;
    CHECK(open_wav(slurp(pa), true, &fr, &bits) == 1 && fr == 5 && bits == 16);
}

static void arithmetic() {
    CHECK(block_size(48000) == 480 && block_size(44100) == 480 && block_size(96000) == 960 && block_size(0) == 480 &&
          block_size(-5) == 480);
    auto g = group_jobs({{48000, 2}, {44100, 2}, {48000, 2}, {48000, 1}, {44100, 2}});
    CHECK(g.size() == 3 && g[0] == std::vector<size_t>({0, 2}) && g[1] == std::vector<size_t>({1, 4}) &&
          g[2] == std::vector<size_t>({3}));
    CHECK(group_jobs({}).empty());
    CHECK(clip_estimate(ClipSize{1000, 1500, 2}, 2) == 2 * (1500 * 20 + 1000 * 6));
    CHECK(clip_estimate(ClipSize{INT64_MAX, INT64_MAX, 4}, 65535) == INT64_MAX);
    CHECK(clip_estimate(ClipSize{-1, -1, 2}, 2) == 0);
    const ClipSize c{1000, 1000, 2}; // 26 000 bytes per channel
    std::vector<ClipSize> v(7, c);
    auto cuts = cut_subbatches(v, 1, 3 * 26000);
    CHECK(cuts.size() == 3 && cuts[0] == std::make_pair((size_t)0, (size_t)3) && cuts[1] == std::make_pair((size_t)3, (size_t)6) &&
          cuts[2] == std::make_pair((size_t)6, (size_t)7));
    cuts = cut_subbatches(v, 1, 1);   // every clip exceeds the budget: each runs alone
    CHECK(cuts.size() == 7);
    cuts = cut_subbatches(v, 1, INT64_MAX);
    CHECK(cuts.size() == 1 && cuts[0].second == 7);
    cuts = cut_subbatches(v, 1, 0);
    CHECK(cuts.size() == 7);
    cuts = cut_subbatches(v, 1, -5);
    CHECK(cuts.size() == 7);
    CHECK(cut_subbatches({}, 2, 100).empty());
    std::vector<ClipSize> many(70000, ClipSize{1, 1, 1});
    cuts = cut_subbatches(many, 2, INT64_MAX); // 65535 / 2 clips at most
    CHECK(cuts.size() == 3 && cuts[0].second == 32767 && cuts[1].second == 65534 && cuts[2].second == 70000);
    cuts = cut_subbatches(many, 70000, INT64_MAX);
    CHECK(cuts.size() == 70000);
    cuts = cut_subbatches(many, 0, INT64_MAX);
    CHECK(cuts.size() == 70000);
    std::vector<ClipSize> huge(3, ClipSize{INT64_MAX / 2, INT64_MAX / 2, 4});
    cuts = cut_subbatches(huge, 2, INT64_MAX);
    size_t covered = 0;
    for (auto &r : cuts) {
        CHECK(r.first == covered && r.second > r.first);
        covered = r.second;
    }
    CHECK(covered == 3);
    std::vector<ClipSize> mixed = {c, ClipSize{100000, 100000, 2}, c, c};
    cuts = cut_subbatches(mixed, 1, 2 * 26000); // the long clip alone, in manifest order
    CHECK(cuts.size() == 3 && cuts[1] == std::make_pair((size_t)1, (size_t)2) && cuts[2] == std::make_pair((size_t)2, (size_t)4));
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    dir = argv[1];
    manifests();
    wavs();
    arithmetic();
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
