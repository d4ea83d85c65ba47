// pv_cli_batch.h -- what audiomod-pv-exe does without the engine: the RIFF/WAVE reader and the 16-bit writer (the
// reference's sample conversions and header layout, see audiomod_pv_cli.cc), the parser of the `batch` command's
// manifest, and the arithmetic that groups its jobs and cuts a group into sub-batches.  No GPU, no library: a
// stand-alone program can include this file alone (tests/native/host_cli_batch_sanitize.cc runs it under sanitizers).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace pvcli {

struct WavIn {
    int channels = 0, rate = 0, bits = 0;
    long frames = 0;
    std::vector<unsigned char> data; // raw little-endian PCM of the 'data' chunk (empty when only the header was asked for)
    long pos = 0;                    // bytes consumed

    // load = false: the header alone; `frames` is what a full read would find (the data chunk's length, or what the
    // file holds of it)
    explicit WavIn(const char *path, bool load = true) {
        FILE *f = fopen(path, "rb");
        if (!f) throw std::runtime_error(std::string("cannot open ") + path);
        unsigned char h[12];
        if (fread(h, 1, 12, f) != 12 || memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) {
            fclose(f);
            throw std::runtime_error("not a RIFF/WAVE file");
        }
        // chunk lengths come from the file: never allocate or skip by more than the file still holds
        long file_size = 0;
        if (fseek(f, 0, SEEK_END) == 0) file_size = ftell(f);
        fseek(f, 12, SEEK_SET);
        bool have_fmt = false, have_data = false;
        int block_align = 0;
        size_t data_bytes = 0;
        while (!have_data) {
            unsigned char ch[8];
            if (fread(ch, 1, 8, f) != 8) break;
            const uint32_t len = ch[4] | (ch[5] << 8) | (ch[6] << 16) | ((uint32_t)ch[7] << 24);
            const long here = ftell(f);
            const long remaining = here >= 0 && file_size > here ? file_size - here : 0;
            if (!memcmp(ch, "fmt ", 4)) {
                if (len < 16 || len > 4096 || (long)len > remaining) break; // a format chunk is 16-40 bytes
                std::vector<unsigned char> b(len);
                if (fread(b.data(), 1, len, f) != len) break;
                if (len & 1) fseek(f, 1, SEEK_CUR); // chunks are word aligned: skip the pad byte
                const int fmt = b[0] | (b[1] << 8);
                channels = b[2] | (b[3] << 8);
                rate = (int)(b[4] | (b[5] << 8) | (b[6] << 16) | ((uint32_t)b[7] << 24));
                block_align = b[12] | (b[13] << 8);
                bits = b[14] | (b[15] << 8);
                if (fmt != 1) {
                    fclose(f);
                    throw std::runtime_error("only PCM WAV files are supported");
                }
                have_fmt = true;
            } else if (!memcmp(ch, "data", 4)) {
                const size_t want = (long)len > remaining ? (size_t)remaining : (size_t)len; // a truncated file: what is there
                if (load) {
                    data.resize(want);
                    const size_t got = want ? fread(data.data(), 1, want, f) : 0;
                    data.resize(got);
                    data_bytes = got;
                } else {
                    data_bytes = want;
                }
                have_data = true;
            } else {
                const long skip = (long)len + (len & 1);
                if (skip > remaining || fseek(f, skip, SEEK_CUR) != 0) break;
            }
        }
        fclose(f);
        if (!have_fmt || !have_data || channels < 1 || (bits != 8 && bits != 16 && bits != 24 && bits != 32) ||
            block_align != channels * bits / 8)
            throw std::runtime_error("unsupported, inconsistent or truncated WAV file");
        frames = (long)(data_bytes / (size_t)(channels * bits / 8));
    }

    // planar read of up to n frames; returns frames read (reference WavInFile::read(float**, int))
    int read(float *const *buf, int n) {
        const int bps = bits / 8;
        const long left = (long)(data.size() - (size_t)pos) / (channels * bps);
        if (n > left) n = (int)left;
        const unsigned char *p = data.data() + pos;
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < channels; ++c, p += bps) {
                float v;
                if (bps == 1) {
                    v = (float)(p[0] * (1.0 / 128.0) - 1.0);
                } else if (bps == 2) {
                    const int16_t s = (int16_t)(p[0] | (p[1] << 8));
                    v = (float)(s * (1.0 / 32768.0));
                } else if (bps == 3) {
                    int32_t s = p[0] | (p[1] << 8) | (p[2] << 16);
                    if (s & 0x00800000) s |= (int32_t)0xff000000;
                    v = (float)(s * (1.0 / 8388608.0));
                } else {
                    const int32_t s = (int32_t)(p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24));
                    v = (float)(s * (1.0 / 2147483648.0));
                }
                buf[c][i] = v;
            }
        pos += (long)n * channels * bps;
        return n;
    }
};

struct WavOut16 {
    FILE *f = nullptr;
    int channels, rate;
    uint32_t bytes = 0;
    WavOut16(const char *path, int rate_, int channels_) : channels(channels_), rate(rate_) {
        f = fopen(path, "wb");
        if (!f) throw std::runtime_error(std::string("cannot open ") + path + " for writing");
        header();
    }
    WavOut16(const WavOut16 &) = delete;
    void operator=(const WavOut16 &) = delete;
    static void put32(unsigned char *p, uint32_t v) {
        p[0] = v & 255;
        p[1] = (v >> 8) & 255;
        p[2] = (v >> 16) & 255;
        p[3] = (v >> 24) & 255;
    }
    static void put16(unsigned char *p, uint32_t v) {
        p[0] = v & 255;
        p[1] = (v >> 8) & 255;
    }
    // 56-byte header: RIFF(12) + fmt(24) + fact(12) + data(8), the layout the reference writes
    void header() {
        unsigned char h[56];
        const uint32_t bpf = (uint32_t)(2 * channels);
        memcpy(h, "RIFF", 4);
        put32(h + 4, bytes + 56 - 12 + 4);
        memcpy(h + 8, "WAVE", 4);
        memcpy(h + 12, "fmt ", 4);
        put32(h + 16, 16);
        put16(h + 20, 1);
        put16(h + 22, (uint32_t)channels);
        put32(h + 24, (uint32_t)rate);
        put32(h + 28, bpf * (uint32_t)rate);
        put16(h + 32, bpf);
        put16(h + 34, 16);
        memcpy(h + 36, "fact", 4);
        put32(h + 40, 4);
        put32(h + 44, bytes / bpf);
        memcpy(h + 48, "data", 4);
        put32(h + 52, bytes);
        fseek(f, 0, SEEK_SET);
        fwrite(h, 1, 56, f);
        fseek(f, 0, SEEK_END);
    }
    void write(float *const *buf, int n) {
        std::vector<unsigned char> tmp((size_t)n * channels * 2);
        unsigned char *p = tmp.data();
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < channels; ++c, p += 2) {
                float v = buf[c][i] * 32768.0f;
                if (v > 32767.0f) v = 32767.0f;
                else if (v < -32768.0f) v = -32768.0f;
                const int16_t s = (int16_t)(int)v; // truncation toward zero, like the reference
                put16(p, (uint16_t)s);
            }
        fwrite(tmp.data(), 1, tmp.size(), f);
        bytes += (uint32_t)tmp.size();
    }
    // samples that are converted and interleaved already ([n][channels] int16: the mixed batch's PCM output)
    void write_pcm16(const int16_t *pcm, size_t n) {
        std::vector<unsigned char> tmp(n * (size_t)channels * 2);
        for (size_t i = 0; i < n * (size_t)channels; ++i) put16(tmp.data() + 2 * i, (uint16_t)pcm[i]);
        fwrite(tmp.data(), 1, tmp.size(), f);
        bytes += (uint32_t)tmp.size();
    }
    ~WavOut16() {
        if (f) {
            header();
            fclose(f);
        }
    }
};

// ---------------------------------------------------------------- the manifest
// One job per line, fields separated by tabs: in.wav, out.wav and optionally an amount (semitones, or the time ratio
// for time_stretch) that overrides the command's.  Blank lines and lines that start with '#' are skipped.
struct ManifestJob {
    std::string in, out, amount_text;
    bool has_amount = false;
    double amount = 0;
    int line = 0; // 1-based
};

// false: `error` says what is wrong and `error_line` where (0: the manifest as a whole)
inline bool parse_manifest(const std::string &text, bool model_takes_amount, std::vector<ManifestJob> &jobs, int &error_line,
                           std::string &error) {
    jobs.clear();
    auto fail = [&](int line, const std::string &what) {
        jobs.clear();
        error_line = line;
        error = what;
        return false;
    };
    int line_no = 0;
    for (size_t at = 0; at < text.size();) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        std::string line = text.substr(at, end - at);
        at = end + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.find_first_not_of(" \t") == std::string::npos || line[0] == '#') continue;
        std::vector<std::string> fields;
        for (size_t a = 0;;) {
            const size_t t = line.find('\t', a);
            fields.push_back(line.substr(a, t == std::string::npos ? std::string::npos : t - a));
            if (t == std::string::npos) break;
            a = t + 1;
        }
        if (fields.size() < 2 || fields.size() > 3) return fail(line_no, "expected in.wav<TAB>out.wav[<TAB>amount]");
        if (fields[0].empty() || fields[1].empty()) return fail(line_no, "empty path");
        if (fields[0].find('\0') != std::string::npos || fields[1].find('\0') != std::string::npos)
            return fail(line_no, "a path holds a NUL byte");
        ManifestJob j;
        j.in = fields[0], j.out = fields[1], j.line = line_no;
        if (fields.size() == 3) {
            if (!model_takes_amount) return fail(line_no, "this model takes no amount");
            const char *s = fields[2].c_str();
            char *e = nullptr;
            j.amount = strtod(s, &e);
            if (e == s || (size_t)(e - s) != fields[2].size() || !std::isfinite(j.amount) || !std::isfinite((float)j.amount))
                return fail(line_no, "the amount is not a finite number");
            j.has_amount = true;
            j.amount_text = fields[2];
        }
        jobs.push_back(j);
    }
    if (jobs.empty()) return fail(0, "the manifest holds no job");
    for (size_t i = 0; i < jobs.size(); ++i)
        for (size_t k = 0; k < jobs.size(); ++k) {
            if (k < i && jobs[k].out == jobs[i].out)
                return fail(jobs[i].line, "output path already used by line " + std::to_string(jobs[k].line));
            if (jobs[k].in == jobs[i].out)
                return fail(jobs[i].line, "output path is the input path of line " + std::to_string(jobs[k].line));
        }
    return true;
}

// ---------------------------------------------------------------- grouping and sub-batches
// jobs of equal (sample rate, channels) form a group; groups in order of first appearance, manifest order within
inline std::vector<std::vector<size_t>> group_jobs(const std::vector<std::pair<int, int>> &rate_channels) {
    std::vector<std::vector<size_t>> groups;
    std::vector<std::pair<int, int>> keys;
    for (size_t i = 0; i < rate_channels.size(); ++i) {
        size_t g = 0;
        while (g < keys.size() && keys[g] != rate_channels[i]) ++g;
        if (g == keys.size()) keys.push_back(rate_channels[i]), groups.emplace_back();
        groups[g].push_back(i);
    }
    return groups;
}

inline int block_size(int rate) { return rate / 100 < 480 ? 480 : rate / 100; } // main.cc:149

struct ClipSize {
    int64_t frames = 0, out_frames = 0;
    int bytes_per_sample = 2;
    int64_t table_bytes = 0; // whisper: the clip's own phases, slices x channels x (fftsize / 2 + 8) floats -- an upper
                             // bound of its share: a sub-batch holds one table, the longest clip's
};
constexpr int64_t kDescriptorBytesPerOutFrame = 14; // per output frame and stream

// Device bytes a clip costs in a sub-batch, estimated before anything is allocated: per channel its output frames'
// descriptors, float and int16 samples, and its input frames' float and PCM samples.  Saturates instead of overflowing.
inline int64_t clip_estimate(const ClipSize &c, int channels) {
    const int64_t top = INT64_MAX;
    auto mul = [&](int64_t a, int64_t b) {
        int64_t r;
        return a < 0 || b < 0 ? (int64_t)0 : __builtin_mul_overflow(a, b, &r) ? top : r;
    };
    auto add = [&](int64_t a, int64_t b) {
        int64_t r;
        return __builtin_add_overflow(a, b, &r) ? top : r;
    };
    const int64_t per_channel =
        add(mul(c.out_frames, kDescriptorBytesPerOutFrame + 4 + 2), mul(c.frames, 4 + (int64_t)c.bytes_per_sample));
    return add(mul(per_channel, channels), c.table_bytes < 0 ? 0 : c.table_bytes);
}

// [begin, end) ranges in order: none holds more than 65535 / channels clips, none exceeds `budget_bytes` by
// clip_estimate unless it is a single clip (one that exceeds the budget on its own runs alone)
inline std::vector<std::pair<size_t, size_t>> cut_subbatches(const std::vector<ClipSize> &clips, int channels,
                                                             int64_t budget_bytes) {
    std::vector<std::pair<size_t, size_t>> out;
    const size_t max_clips = channels >= 1 && channels <= 65535 ? (size_t)(65535 / channels) : 1;
    size_t begin = 0;
    int64_t sum = 0;
    for (size_t i = 0; i < clips.size(); ++i) {
        const int64_t e = clip_estimate(clips[i], channels);
        const bool fits = i - begin < max_clips && e <= budget_bytes && sum <= budget_bytes - e;
        if (i > begin && !fits) {
            out.emplace_back(begin, i);
            begin = i;
            sum = 0;
        }
        sum = e > INT64_MAX - sum ? INT64_MAX : sum + e;
    }
    if (begin < clips.size()) out.emplace_back(begin, clips.size());
    return out;
}

} // namespace pvcli
