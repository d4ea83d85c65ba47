// audiomod_pv_cli.cc -- command-line driver for the phase-vocoder effects, same argv grammar and drive
// loops as the reference CLI for these effects (reference main/main.cc:24-93 usage, :196-286 argument
// parsing, :471-510 offline loops) over the drop-in audiomod::phasevocoder class, plus a from-scratch RIFF/WAVE
// reader/writer with the reference's sample conversions (pv_cli_batch.h; reference main/wavfile.cc:733-755 int16 ->
// float * 1/32768; :1295-1306,1508-1527 float -> int16 saturate then truncate toward zero; header with a 'fact'
// chunk, wavfile.h:62-106, wavfile.cc:1135-1182).
//
//   audiomod-pv-exe time_stretch       in.wav out.wav <time_ratio> <coremode> <fftsize>
//   audiomod-pv-exe normal_pitchshift  in.wav out.wav <semitones>  <coremode> <fftsize>
//   audiomod-pv-exe formant_pitchshift in.wav out.wav <semitones>  <coremode> <fftsize>
//   audiomod-pv-exe gender_change      in.wav out.wav <semitones>  <coremode> <fftsize>
//   audiomod-pv-exe formant_cepstral   in.wav out.wav <semitones>  <coremode> <fftsize>   (extension of this engine)
//   audiomod-pv-exe robotic | whisper | vocoder | vocoder_chord   in.wav out.wav
//   audiomod-pv-exe constant           in.wav out.wav      (real-time processBlock loop, main.cc:561-572)
// Effects of the reference that are not phase-vocoder modes are not provided here.
// An extension of this engine: time_stretch and normal_pitchshift take a trailing  --formant <semitones>, the formant
// setting of audiomod_pv.h (0: the formants stay where they are whatever the pitch does).
//
// An extension of this engine: a folder of files in one process,
//   audiomod-pv-exe batch <dafx_name> <manifest> [<amount> <coremode> <fftsize>] [--mem-gb G] [--formant <semitones>]
// The manifest has one job per line, in.wav<TAB>out.wav[<TAB>amount]; every output file is byte for byte what the
// single-file command writes for that file and amount.  Jobs of equal sample rate and channel count run together
// through the mixed batch's PCM wire (pv_mbatch_run_pcm_host) wherever the mixed batch serves the configuration, and
// one by one through the single-file route below where it does not.  --formant is one value for all jobs.  stdout: one line per job, in manifest order,
// ok<TAB>out.wav<TAB>frames or failed<TAB>in.wav<TAB>reason.  Exit status 0, 1 if a job failed, 2 for a bad manifest.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "audiomod_pv.h"
#include "phasevocoder.h"
#include "pv_cli_batch.h"

namespace {

using pvcli::WavIn;
using pvcli::WavOut16;

int usage() {
    fprintf(stderr,
            "usage: audiomod-pv-exe dafx_name infile outfile <args> (dafx: constant, time_stretch, normal_pitchshift, "
            "formant_pitchshift, gender_change, vocoder, vocoder_chord, robotic, whisper)\n"
            "       audiomod-pv-exe batch dafx_name manifest [<amount> <coremode> <fftsize>] [--mem-gb G] [--formant st]\n"
            "       time_stretch and normal_pitchshift take a trailing --formant <semitones>\n");
    return -1;
}

// what the model name selects: the class's mode, whether the command line carries <amount> <coremode> <fftsize>, and
// whether the amount is the time ratio (time_stretch: no flush, main.cc:471-478) instead of the pitch
struct Model {
    const char *name;
    int mode;
    bool takes_args, stretch;
};
const Model kModels[] = {
    {"time_stretch", NORMAL_STRETCH, true, true},
    {"normal_pitchshift", NORMAL_SHIFT, true, false},
    {"formant_pitchshift", FORMANT_PRESERVE, true, false},
    {"gender_change", GENDER_CHANGE, true, false},
    {"formant_cepstral", FORMANT_CEPSTRAL, true, false}, // extension, see PV_MODE_FORMANT_CEPSTRAL
    {"robotic", ROBOTIC, false, false},
    {"whisper", WHISPER, false, false},
    {"vocoder", VOCODER_ROSENBERG, false, false},
    {"vocoder_chord", VOCODER_CHORD, false, false},
    {"constant", CONSTANT, false, false},
};
const Model *find_model(const std::string &name) {
    for (const Model &m : kModels)
        if (name == m.name) return &m;
    return nullptr;
}

// --formant <semitones>: the formant setting, for the two plain modes
struct Formant {
    bool on = false;
    float semitones = 0.f;
};
// argv[i] is "--formant": reads its value into fx; false (with a line on stderr) for a missing or bad one, or a model
// the setting does not apply to
bool parse_formant(const std::string &model, int argc, char **argv, int i, Formant &fx) {
    char *e = nullptr;
    const double v = i + 1 < argc ? strtod(argv[i + 1], &e) : 0.0;
    if (i + 1 >= argc || e == argv[i + 1] || *e != 0 || !(v >= -48.0 && v <= 48.0)) {
        fprintf(stderr, "audiomod-pv-exe: --formant needs a number of semitones within +-48\n");
        return false;
    }
    if (model != "time_stretch" && model != "normal_pitchshift") {
        fprintf(stderr, "audiomod-pv-exe: --formant applies to time_stretch and normal_pitchshift only\n");
        return false;
    }
    fx.on = true;
    fx.semitones = (float)v;
    return true;
}

// The single-file command: one fresh engine, the reference's drive loop.  args: what follows the two paths on the
// command line.  Throws what the reader, the writer and the class throw; *written: frames written to out_path.
int run_single(const std::string &model, const char *in_path, const char *out_path, int nargs, const char *const *args,
               long *written, const Formant &fx) {
    WavIn in(in_path);
    const int ch = in.channels, sr = in.rate;
    const long file_length = in.frames;
    std::unique_ptr<audiomod::phasevocoder> pv;
    bool flush = true;
    if (model == "time_stretch") {
        if (nargs < 3) { fprintf(stderr, "err: not enough para (time_ratio, coremode, fftsize)\n"); return -1; }
        pv.reset(new audiomod::phasevocoder(sr, ch, (float)atof(args[0]), 0, NORMAL_STRETCH, atoi(args[1]), atoi(args[2])));
        flush = false; // the reference's time_stretch loop has no flush (main.cc:471-478)
    } else if (model == "normal_pitchshift" || model == "formant_pitchshift" || model == "gender_change" ||
               model == "formant_cepstral") { // formant_cepstral: extension, see PV_MODE_FORMANT_CEPSTRAL
        if (nargs < 3) { fprintf(stderr, "err: not enough para (pitchshift_amount, coremode, fftsize)\n"); return -1; }
        const int mode = model == "normal_pitchshift"    ? NORMAL_SHIFT
                         : model == "formant_pitchshift" ? FORMANT_PRESERVE
                         : model == "formant_cepstral"   ? FORMANT_CEPSTRAL
                                                         : GENDER_CHANGE;
        pv.reset(new audiomod::phasevocoder(sr, ch, 1, (float)atof(args[0]), mode, atoi(args[1]), atoi(args[2])));
    } else if (model == "robotic" || model == "whisper" || model == "vocoder" || model == "vocoder_chord" ||
               model == "constant") {
        const int mode = model == "robotic" ? ROBOTIC : model == "whisper" ? WHISPER : model == "vocoder" ? VOCODER_ROSENBERG
                         : model == "vocoder_chord" ? VOCODER_CHORD : CONSTANT;
        pv.reset(new audiomod::phasevocoder(sr, ch, 1, 0, mode));
    } else {
        fprintf(stderr, "fx not supported by the MI355X phase-vocoder driver: %s\n", model.c_str());
        return usage();
    }
    if (fx.on) pv->setParams({{"formant_semitones", fx.semitones}});
    modbase_offline *off = pv.get();
    WavOut16 out(out_path, sr, ch);
    const int block = pvcli::block_size(sr);
    if (model == "constant") { // "everything else - real time application" (main.cc:560-572)
        modbase *rt = pv.get();
        std::vector<std::vector<float>> bs(ch, std::vector<float>(block));
        std::vector<float *> buff(ch);
        for (int c = 0; c < ch; ++c) buff[c] = bs[c].data();
        for (long i = 0; i < file_length; i += block) {
            const int n = in.read(buff.data(), block);
            rt->processBlock(buff.data(), n);
            if (rt->outputReady()) out.write(buff.data(), n);
        }
        if (written) *written = (long)(out.bytes / (2u * (uint32_t)ch));
        return 0;
    }
    std::vector<std::vector<float>> bs(ch, std::vector<float>(block)), os(ch, std::vector<float>(block * 4));
    std::vector<float *> buff(ch), outbuff(ch);
    for (int c = 0; c < ch; ++c) {
        buff[c] = bs[c].data();
        outbuff[c] = os[c].data();
    }
    long produced = 0;
    for (long i = 0; i < file_length; i += block) {
        const int n = in.read(buff.data(), block);
        off->processInData(buff.data(), n);
        const int got = off->getOutSamples();
        off->getOutData(outbuff.data(), got);
        out.write(outbuff.data(), got);
        produced += got;
    }
    if (flush) {
        for (int c = 0; c < ch; ++c) memset(buff[c], 0, sizeof(float) * block);
        while (produced < file_length) {
            off->processInData(buff.data(), block);
            const int got = off->getOutSamples();
            off->getOutData(outbuff.data(), got);
            const int w = (file_length - produced > got) ? got : (int)(file_length - produced);
            out.write(outbuff.data(), w);
            produced += w;
        }
    }
    if (written) *written = (long)(out.bytes / (2u * (uint32_t)ch));
    return 0;
}

// ---------------------------------------------------------------- batch
struct BatchJob {
    pvcli::ManifestJob m;
    int rate = 0, channels = 0, bits = 0;
    long frames = 0;
    int64_t out_frames = 0; // as pv_mbatch_layout plans it (batch route)
    bool batch_route = false, failed = false, done = false;
    std::string reason;
    int64_t slices = 0; // (mixed-batch route: the stream's slices, for the whisper table's estimate)
    long written = 0;
    void fail(const std::string &why) {
        if (!failed && !done) failed = true, reason = why;
    }
};

struct PinnedBuf { // page-locked host memory that grows
    void *p = nullptr;
    size_t n = 0;
    ~PinnedBuf() { pv_host_free(p); }
    bool reserve(size_t bytes) {
        if (bytes <= n && p) return true;
        pv_host_free(p);
        n = bytes + bytes / 8 + 16;
        p = pv_host_alloc(n);
        if (!p) n = 0;
        return p != nullptr;
    }
};

std::string engine_error(int st) { return std::string(pv_strerror(st)) + ": " + pv_last_error(); }

// one group (equal rate and channels) of jobs the mixed batch accepts, sub-batch by sub-batch
void run_group_batched(const Model &model, const pv_config &cfg, std::vector<BatchJob *> &jobs, float amount, int64_t budget,
                       int device, const Formant &fx, bool whisper) {
    const int C = cfg.channels, block = pvcli::block_size(cfg.sample_rate), flush = model.stretch ? 0 : 1;
    std::vector<pvcli::ClipSize> sizes;
    for (const BatchJob *j : jobs)
        sizes.push_back(pvcli::ClipSize{j->frames, j->out_frames, j->bits / 8,
                                        whisper ? j->slices * C * (int64_t)(cfg.fftsize / 2 + 8) * 4 : 0});
    pv_mbatch *mb = nullptr;
    size_t mb_clips = 0;
    PinnedBuf h_in, h_out;
    const std::vector<std::pair<size_t, size_t>> cuts = pvcli::cut_subbatches(sizes, C, budget);
    int redrawn = 0;
    for (const auto &range : cuts) {
        const size_t n = range.second - range.first;
        BatchJob *const *sub = jobs.data() + range.first;
        auto fail_all = [&](const std::string &why) {
            for (size_t i = 0; i < n; ++i) sub[i]->fail(why);
        };
        std::vector<pv_mbatch_stream> streams(n);
        std::vector<int32_t> bits(n);
        for (size_t i = 0; i < n; ++i) {
            const float a = sub[i]->m.has_amount ? (float)sub[i]->m.amount : amount;
            streams[i] = pv_mbatch_stream{sub[i]->frames, model.stretch ? a : 1.0f, model.stretch ? 0.0f : a};
            bits[i] = sub[i]->bits;
        }
        int st;
        if (mb && mb_clips == n) { // consecutive sub-batches of equal clip count: the object is re-drawn in place
            st = pv_mbatch_redraw(mb, streams.data());
            ++redrawn;
        } else {
            pv_mbatch_destroy(mb);
            mb = nullptr;
            st = pv_mbatch_create(&cfg, streams.data(), (int32_t)n, block, flush, device, &mb);
            mb_clips = n;
        }
        if (st == PV_OK && fx.on) { // (a re-drawn object is back to off, like a new one)
            const std::vector<float> knob(n, fx.semitones);
            st = pv_mbatch_set_formant(mb, knob.data());
        }
        if (st == PV_OK && whisper) { // (likewise: a re-drawn object is all robotic)
            const std::vector<int32_t> voice(n, PV_VOICE_WHISPER);
            st = pv_mbatch_set_voice(mb, voice.data());
        }
        if (st != PV_OK) {
            fail_all(engine_error(st));
            pv_mbatch_destroy(mb);
            mb = nullptr;
            continue;
        }
        std::vector<int64_t> in_off(n), out_off(n);
        int64_t in_bytes = 0, out_bytes = 0;
        if ((st = pv_mbatch_pcm_layout(mb, bits.data(), in_off.data(), out_off.data(), &in_bytes, &out_bytes)) != PV_OK) {
            fail_all(engine_error(st));
            continue;
        }
        if (!h_in.reserve((size_t)in_bytes) || !h_out.reserve((size_t)out_bytes)) {
            fail_all("no page-locked host memory for the sub-batch");
            continue;
        }
        for (size_t i = 0; i < n; ++i) {
            BatchJob &j = *sub[i];
            const size_t want = (size_t)j.frames * (size_t)C * (size_t)(j.bits / 8);
            unsigned char *dst = static_cast<unsigned char *>(h_in.p) + in_off[i];
            try {
                WavIn w(j.m.in.c_str());
                if (w.frames != j.frames || w.bits != j.bits || w.channels != C || w.data.size() < want)
                    throw std::runtime_error("the file changed while the batch ran");
                memcpy(dst, w.data.data(), want);
            } catch (const std::exception &e) {
                j.fail(e.what());
                memset(dst, j.bits == 8 ? 0x80 : 0, want); // its slot runs on silence; nothing is written for it
            }
        }
        if ((st = pv_mbatch_run_pcm_host(mb, bits.data(), h_in.p, h_out.p)) != PV_OK) {
            fail_all(engine_error(st));
            continue;
        }
        for (size_t i = 0; i < n; ++i) {
            BatchJob &j = *sub[i];
            if (j.failed) continue;
            try {
                const int64_t frames = pv_mbatch_out_frames(mb, (int32_t)i);
                WavOut16 out(j.m.out.c_str(), cfg.sample_rate, C);
                out.write_pcm16(reinterpret_cast<const int16_t *>(static_cast<const char *>(h_out.p) + out_off[i]),
                                (size_t)frames);
                j.written = (long)frames;
                j.done = true;
            } catch (const std::exception &e) {
                j.fail(e.what());
            }
        }
    }
    pv_mbatch_destroy(mb);
    fprintf(stderr, "audiomod-pv-exe: batch: %d Hz, %d ch: %zu clips, %zu sub-batches, %d re-drawn in place\n", cfg.sample_rate,
            C, jobs.size(), cuts.size(), redrawn);
}

int batch_main(int argc, char **argv) {
    if (argc < 4) return usage();
    const std::string model_name = argv[2];
    const Model *model = find_model(model_name);
    if (!model) {
        fprintf(stderr, "fx not supported by the MI355X phase-vocoder driver: %s\n", model_name.c_str());
        return usage();
    }
    std::vector<const char *> pos;
    double mem_gb = 16.0;
    Formant fx;
    for (int i = 4; i < argc; ++i) {
        if (!strcmp(argv[i], "--formant")) {
            if (!parse_formant(model_name, argc, argv, i, fx)) return usage();
            ++i;
        } else if (!strcmp(argv[i], "--mem-gb")) {
            char *e = nullptr;
            if (i + 1 >= argc || (mem_gb = strtod(argv[i + 1], &e), *e != 0) || !(mem_gb > 0) || mem_gb > 1e6) {
                fprintf(stderr, "audiomod-pv-exe: --mem-gb needs a positive number of GiB\n");
                return usage();
            }
            ++i;
        } else {
            pos.push_back(argv[i]);
        }
    }
    if (model->takes_args && pos.size() < 3) {
        fprintf(stderr, "err: not enough para (%s, coremode, fftsize)\n", model->stretch ? "time_ratio" : "pitchshift_amount");
        return -1;
    }
    const int64_t budget = (int64_t)(mem_gb * 1073741824.0);

    // the manifest: everything wrong with it is reported before any file is opened and before any device call
    std::string text;
    {
        FILE *f = fopen(argv[3], "rb");
        if (!f) {
            fprintf(stderr, "audiomod-pv-exe: cannot open manifest %s\n", argv[3]);
            return 2;
        }
        char buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
        fclose(f);
    }
    std::vector<pvcli::ManifestJob> parsed;
    int err_line = 0;
    std::string err;
    if (!pvcli::parse_manifest(text, model->takes_args, parsed, err_line, err)) {
        fprintf(stderr, "audiomod-pv-exe: manifest %s: line %d: %s\n", argv[3], err_line, err.c_str());
        return 2;
    }
    if (pv_device_count() < 1) {
        fprintf(stderr, "audiomod-pv-exe: %s\n", pv_strerror(PV_ERR_NO_DEVICE));
        return 1;
    }
    int device = 0;
    if (const char *env = getenv("AUDIOMOD_PV_DEVICE")) device = atoi(env);

    std::vector<BatchJob> jobs(parsed.size());
    std::vector<std::pair<int, int>> keys;
    std::vector<size_t> readable;
    for (size_t i = 0; i < parsed.size(); ++i) {
        BatchJob &j = jobs[i];
        j.m = parsed[i];
        try {
            WavIn w(j.m.in.c_str(), false);
            j.rate = w.rate, j.channels = w.channels, j.bits = w.bits, j.frames = w.frames;
            keys.emplace_back(j.rate, j.channels);
            readable.push_back(i);
        } catch (const std::exception &e) {
            j.fail(e.what());
        }
    }
    const float amount = model->takes_args ? (float)atof(pos[0]) : 0.0f;
    for (const std::vector<size_t> &group : pvcli::group_jobs(keys)) {
        const BatchJob &first = jobs[readable[group[0]]];
        // the configuration the drop-in class builds for the single-file command (its defaults for the names
        // without arguments: include/dafx/phasevocoder.h)
        pv_config cfg;
        cfg.sample_rate = first.rate;
        cfg.channels = first.channels;
        cfg.time_ratio = model->stretch ? amount : 1.0f;
        cfg.pitch_semitones = model->stretch ? 0.0f : amount;
        // whisper: a ROBOTIC mixed batch with every stream's voice set (the voice setting) -- the same streams, bit for bit
        const bool whisper = model->mode == WHISPER;
        cfg.mode = whisper ? ROBOTIC : model->mode;
        cfg.coremode = model->takes_args ? atoi(pos[1]) : PHASE_LOCKED;
        cfg.fftsize = model->takes_args ? atoi(pos[2]) : 2048;
        cfg.hopsize = 0;
        const int block = pvcli::block_size(cfg.sample_rate), flush = model->stretch ? 0 : 1;
        std::vector<BatchJob *> batched;
        for (size_t g : group) {
            BatchJob &j = jobs[readable[g]];
            const float a = j.m.has_amount ? (float)j.m.amount : amount;
            const pv_mbatch_stream s{j.frames, model->stretch ? a : 1.0f, model->stretch ? 0.0f : a};
            // a job the mixed batch's layout refuses (a mode or size outside its scope, no frames, a pitch whose
            // filter does not fit) takes the single-file route
            if (pv_mbatch_layout(&cfg, &s, 1, block, flush, &j.out_frames, &j.slices, nullptr, nullptr, nullptr, nullptr) == PV_OK) {
                j.batch_route = true;
                batched.push_back(&j);
            }
        }
        if (!batched.empty()) run_group_batched(*model, cfg, batched, amount, budget, device, fx, whisper);
    }
    for (BatchJob &j : jobs) {
        if (j.failed || j.done || j.batch_route) continue;
        const std::string a = j.m.has_amount ? j.m.amount_text : std::string(model->takes_args ? pos[0] : "");
        const char *args[3] = {a.c_str(), model->takes_args ? pos[1] : "", model->takes_args ? pos[2] : ""};
        try {
            const int rc = run_single(model_name, j.m.in.c_str(), j.m.out.c_str(), model->takes_args ? 3 : 0, args, &j.written, fx);
            if (rc == 0) j.done = true;
            else j.fail("the single-file route refused the job");
        } catch (const std::exception &e) {
            j.fail(e.what());
        }
    }
    int status = 0;
    for (const BatchJob &j : jobs) {
        if (j.done) {
            printf("ok\t%s\t%ld\n", j.m.out.c_str(), j.written);
        } else {
            std::string why = j.reason.empty() ? std::string("not run") : j.reason;
            for (char &c : why)
                if (c == '\t' || c == '\n') c = ' ';
            printf("failed\t%s\t%s\n", j.m.in.c_str(), why.c_str());
            status = 1;
        }
    }
    return status;
}

} // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "batch")) {
        try {
            return batch_main(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "audiomod-pv-exe: %s\n", e.what());
            return 1;
        }
    }
    if (argc < 4) return usage();
    Formant fx;
    std::vector<const char *> args;
    for (int i = 4; i < argc; ++i) {
        if (!strcmp(argv[i], "--formant")) {
            if (!parse_formant(argv[1], argc, argv, i, fx)) return usage();
            ++i;
        } else {
            args.push_back(argv[i]);
        }
    }
    try {
        return run_single(argv[1], argv[2], argv[3], (int)args.size(), args.data(), nullptr, fx);
    } catch (const std::exception &e) {
        fprintf(stderr, "audiomod-pv-exe: %s\n", e.what());
        return 1;
    }
}
